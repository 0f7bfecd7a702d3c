"""What tests/test_vecchia_cpu.py, tests/test_gpu_knn_before.py and tests/test_gpu_vecchia.py share: the numpy references of the
predecessor-constrained search and of the Vecchia likelihood, a numpy model of the device kernel's own algorithm, the data sets of the GPU
tests and the raw C-ABI calls.  A plain module: importing it needs no GPU.

    N(i) = the min(m, i) columns j < i of X with the smallest key (dist2(i, j), j), ascending       (local_ref.dist2_matrix's formula)
    cond_i = log p(y_i | y_N(i)) = logp(N(i) then i) - logp(N(i))                                  (ard_grad_ref.logp_grad, twice)
    log p_V(y) = sum_i cond_i,  its gradient the sum of the differences of the two models' gradients

The model of the kernel (model_cond): for the points [N(i) in neighbour order, then i last], p + 1 of them, K_y = L L^T only, then
z = L^-1 y, w = L^-T e_p, a = L^-T z, a' = a - z_p w (a'_p = 0), G = a a^T - a' a'^T - w w^T,
    cond_i = -log L_pp - 1/2 z_p^2 - 1/2 log 2 pi,    d cond_i / d theta_k = 1/2 sum_rs G_rs dK_rs / d theta_k,    d cond_i / d noise = 1/2 sum_r G_rr
in float64 or np.longdouble (the kernel matrix and its derivatives are kernel_ref's float64 ones in both).
"""
import ctypes as C
import math

import numpy as np

import ard_grad_ref
import local_ref as LR
from case_checks import LOGP_CASES
from gprc_amd import _native as nat
from gprc_amd.fit import grad_dict
from kernel_ref import kernel, kernel_derivs, matern_value_and_h

CASES = LR.PREDICT_CASES
N, NOISE = 300, 0.1
M_CONDS = (1, 15, 16, 17, 63, 64, 127)
CHUNK = 16384                      # include/gprc_native.h GPRC_VECCHIA_CHUNK
BEFORE_MS = LR.KNN_MS
BEFORE_WINDOWS = ((31, 2), (32, 1), (1000, 65))     # with (0, n) and (n - 1, 1)

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- the search -------------------------------------------------------------------------------------------------------------------------
def knn_before_ref(X, m, scale=None, block=512):
    """(idx[n, m], dist2[n, m]): row i the m smallest keys (dist2, j) among j < i, ascending; -1 and +inf at the ranks >= i"""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[1]
    idx, dist = np.full((n, m), -1, dtype=np.int64), np.full((n, m), np.inf)
    for i0 in range(0, n, block):
        i1 = min(n, i0 + block)
        D = LR.dist2_matrix(X[:, :i1], X[:, i0:i1], scale)                  # (i1 - i0) x i1
        D[np.arange(i1)[None, :] >= np.arange(i0, i1)[:, None]] = np.inf    # j >= i is no candidate
        index = np.broadcast_to(np.arange(i1), D.shape)
        order = np.lexsort((index, D), axis=1)[:, :m]
        k = order.shape[1]
        got = np.take_along_axis(D, order, axis=1)
        fill = np.arange(k)[None, :] < np.arange(i0, i1)[:, None]           # rank r of point i is filled iff r < i
        idx[i0:i1, :k] = np.where(fill, order, -1)
        dist[i0:i1, :k] = np.where(fill, got, np.inf)
    return idx, dist


def before_reference(d, n, scaled):
    """knn_before_ref at m = 129 (the ranks 0 .. 128: one more than the widest search) of local_ref.knn_data(d, n)'s X, computed once: a
    smaller m is its first m columns"""
    return _cached(("before", d, n, scaled), lambda: knn_before_ref(LR.knn_data(d, n)[0], 129, LR.knn_scale(d) if scaled else None))


def smallest_prefix_gap(sorted_dist, m):
    """the smallest relative gap (b - a) / b between consecutive FINITE sorted distances a <= b among the ranks 0 .. m of every row"""
    S = np.asarray(sorted_dist)[:, :m + 1]
    a, b = S[:, :-1], S[:, 1:]
    ok = np.isfinite(b)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(b > 0, (b - a) / b, 0.0)
    return float(g[ok].min()) if ok.any() else 1.0


# ---- the likelihood -----------------------------------------------------------------------------------------------------------------------
def cond_ref(name, theta, X, y, noise, nb, i):
    """(cond_i, grad_i) as the difference of two marginals; nb: the conditioning set (may be empty)"""
    pts = list(nb) + [i]
    full, gfull = ard_grad_ref.logp_grad(name, theta, X[:, pts], y[pts], noise)
    if len(nb) == 0:
        return full, gfull
    sub, gsub = ard_grad_ref.logp_grad(name, theta, X[:, list(nb)], y[list(nb)], noise)
    return full - sub, gfull - gsub


def _cholesky(A):
    """lower Cholesky factor in A's dtype (np.linalg has no longdouble): column by column"""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            raise np.linalg.LinAlgError("not positive definite")
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return L


def _forward(L, b):
    x = np.zeros_like(b)
    for k in range(len(b)):
        x[k] = (b[k] - L[k, :k] @ x[:k]) / L[k, k]
    return x


def _backward(L, b):
    x = np.zeros_like(b)
    for k in range(len(b) - 1, -1, -1):
        x[k] = (b[k] - L[k + 1:, k] @ x[k + 1:]) / L[k, k]
    return x


def model_cond(name, theta, X, y, noise, nb, i, dtype=np.float64):
    """(cond_i, grad_i) by the kernel's own algorithm (module docstring) in dtype"""
    pts = list(nb) + [i]
    p = len(nb)
    Xm = X[:, pts]
    K = kernel(name, theta, Xm)
    Ky = (K + noise * np.eye(p + 1)).astype(dtype)
    yv = y[pts].astype(dtype)
    if dtype is np.float64:
        from scipy.linalg import solve_triangular
        L = np.linalg.cholesky(Ky)
        e = np.zeros(p + 1)
        e[p] = 1.0
        z = solve_triangular(L, yv, lower=True)
        w = solve_triangular(L, e, lower=True, trans="T")
        a = solve_triangular(L, z, lower=True, trans="T")
    else:
        L = _cholesky(Ky)
        e = np.zeros(p + 1, dtype=dtype)
        e[p] = 1
        z, w = _forward(L, yv), _backward(L, e)
        a = _backward(L, z)
    ap = a - z[p] * w
    ap[p] = 0
    G = np.outer(a, a) - np.outer(ap, ap) - np.outer(w, w)
    half = dtype(0.5)
    cond = -np.log(L[p, p]) - half * z[p] * z[p] - half * dtype(math.log(2.0 * math.pi))
    grad = [half * np.sum(G * dK.astype(dtype)) for dK in kernel_derivs(name, theta, Xm, K)]
    grad.append(half * np.trace(G))
    return cond, np.array(grad, dtype=dtype)


def vecchia_sum(per_point, name, theta, X, y, noise, idx):
    """(cond[n], grad[n, n_params + 1]) of per_point (cond_ref or model_cond) over the stored neighbours idx (-1 ends a row)"""
    n = X.shape[1]
    out = [per_point(name, theta, X, y, noise, [j for j in idx[i] if j >= 0] if idx.shape[1] else [], i) for i in range(n)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


# ---- the data sets ------------------------------------------------------------------------------------------------------------------------
def case(name_of_case, n=N):
    """(name, theta, X, y, noise) of a case of local_ref.PREDICT_CASES at size n"""
    name, theta, X, y, noise, _ = LR.predict_case(name_of_case, n)
    return name, theta, X, y, noise


def case_neighbours(name_of_case, m, n=N):
    """(idx, dist2) of knn_before_ref at m (clamped to n - 1) in the case's metric, computed once at 127 per case"""
    def make():
        name, theta, X, _, _ = case(name_of_case, n)
        return knn_before_ref(X, min(127, n - 1), LR.metric_of(name, theta))
    idx, dist = _cached(("nb", name_of_case, n), make)
    k = min(m, n - 1)
    return idx[:, :k], dist[:, :k]


def case_reference(name_of_case, m, n=N):
    """(cond[n], grad[n, n_params + 1]) of the difference-of-marginals reference, computed once"""
    def make():
        name, theta, X, y, noise = case(name_of_case, n)
        return vecchia_sum(cond_ref, name, theta, X, y, noise, case_neighbours(name_of_case, m, n)[0])
    return _cached(("ref", name_of_case, m, n), make)


def block_also(name_of_case):
    return LOGP_CASES[name_of_case][4]


def bits_data():
    """(X 2 x (2 CHUNK + 257), y): points that straddle launch chunks and groups of 256"""
    rng = np.random.default_rng(5150)
    n = 2 * CHUNK + 257
    X = np.asfortranarray(rng.uniform(-1, 1, (2, n)))
    return X, np.sin(3 * X[0]) * np.cos(2 * X[1]) + 0.1 * rng.standard_normal(n)


def optimiser_data(n, d=2, seed=41, ell=(0.35, 0.8), noise=0.05):
    """(X d x n, y, noise): y drawn from the matern52_ard GP with length scales ell and that noise"""
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(rng.uniform(-1, 1, (d, n)))
    L = np.linalg.cholesky(kernel("matern52_ard", np.array(ell), X) + noise * np.eye(n))
    return X, L @ rng.standard_normal(n), noise


class ArdVecchia:
    """The numpy model, every point of a set at once, for the ARD kernels: value_and_grad(theta, noise) hook of fit.optimize_local
    with a .prepare(theta, noise) that searches the conditioning sets in the metric 1 / theta (and counts its calls)."""

    def __init__(self, name, X, y, m):
        assert name.endswith("_ard")
        self.name, self.X, self.y, self.m = name, np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), m
        self.prepares, self.idx = 0, None

    def prepare(self, theta, noise):
        self.prepares += 1
        self.idx = knn_before_ref(self.X, min(self.m, self.X.shape[1] - 1), 1.0 / np.asarray(theta, dtype=np.float64))[0]

    def _kernel(self, theta, diff):
        rho2 = ((diff / theta) ** 2).sum(-1)
        if self.name == "sqrexp_ard":
            k = np.exp(-0.5 * rho2)
            return k, k
        return matern_value_and_h(self.name, rho2, np.float64)

    def _batch(self, theta, noise, pts):
        """pts: B x P indices, the point itself last: (cond[B], grad[B, d + 1])"""
        P = pts.shape[1]
        Xg, yg = self.X.T[pts], self.y[pts]                        # B x P x d, B x P
        diff = Xg[:, :, None, :] - Xg[:, None, :, :]
        K, h = self._kernel(theta, diff)
        L = np.linalg.cholesky(K + noise * np.eye(P))
        e = np.zeros((len(pts), P, 1))
        e[:, P - 1] = 1.0
        Lt = np.swapaxes(L, 1, 2)
        z = np.linalg.solve(L, yg[:, :, None])
        a, w = np.linalg.solve(Lt, z)[:, :, 0], np.linalg.solve(Lt, e)[:, :, 0]
        zp = z[:, P - 1, 0]
        ap = a - zp[:, None] * w
        ap[:, P - 1] = 0.0
        G = a[:, :, None] * a[:, None, :] - ap[:, :, None] * ap[:, None, :] - w[:, :, None] * w[:, None, :]
        cond = -np.log(L[:, P - 1, P - 1]) - 0.5 * zp * zp - 0.5 * math.log(2.0 * math.pi)
        gl = 0.5 * np.einsum("brs,brs,brsc->bc", G, h, diff * diff) / theta ** 3
        return cond, np.concatenate([gl, 0.5 * np.trace(G, axis1=1, axis2=2)[:, None]], axis=1)

    def __call__(self, theta, noise):
        theta = np.asarray(theta, dtype=np.float64)
        n, k = self.idx.shape
        value, grad = 0.0, np.zeros(theta.size + 1)
        for p in range(min(k, n)):                                 # the first points, one size each
            c, g = self._batch(theta, noise, np.concatenate([self.idx[p, :p], [p]])[None, :])
            value, grad = value + c[0], grad + g[0]
        if n > k:
            c, g = self._batch(theta, noise, np.concatenate([self.idx[k:], np.arange(k, n)[:, None]], axis=1))
            value, grad = value + c.sum(), grad + g.sum(0)
        return float(value), grad


# ---- the raw calls --------------------------------------------------------------------------------------------------------------------
_addr = LR._addr


def call_knn_before(X, d, n, m, scale=None, first=0, count=None, ld=None, idx=None, dist=None, want_dist=True, ctx=None):
    """the raw gprc_dev_knn_before: (rc, idx, dist); host arrays count x ld that start as -7 unless the caller brings his own"""
    count = n - first if count is None else count
    ld = m if ld is None else ld
    if idx is None:
        idx = np.full((max(count, 1), max(ld, 1)), -7, dtype=np.intc)
    if dist is None and want_dist:
        dist = np.full((max(count, 1), max(ld, 1)), -7.0)
    sc = None if scale is None else np.ascontiguousarray(np.asarray(scale, dtype=np.float64))
    ctx = ctx or nat.default_context()
    rc = nat.lib().gprc_dev_knn_before(ctx.handle, _addr(X), d, n, first, count, _addr(sc), m, _addr(idx), _addr(dist), ld)
    return rc, idx, dist


def vecchia_prepare(h, m_cond):
    return nat.lib().gprc_lgpr_vecchia_prepare(h, m_cond)


def vecchia_neighbours(h, n, m_cond, ld=None):
    """the raw gprc_lgpr_vecchia_neighbours into a host array n x ld that starts as -7: (rc, idx)"""
    ld = m_cond if ld is None else ld
    idx = np.full((n, max(ld, 1)), -7, dtype=np.intc)
    return nat.lib().gprc_lgpr_vecchia_neighbours(h, idx.ctypes.data, ld), idx


def vecchia_call(h, theta, noise, n, grad=True, cond=True, flagged=True, cond_out=None):
    """the raw gprc_lgpr_vecchia_logp_grad: (rc, logp, grad, cond, flagged); cond_out: the caller's array or tensor instead of a host one"""
    _, pp, npar = nat.params_array(theta)
    g = np.full(npar + 1, -7.0) if grad else None
    c = cond_out if cond_out is not None else (np.full(n, -7.0) if cond else None)
    out, fl = C.c_double(-7.0), C.c_int64(-7)
    rc = nat.lib().gprc_lgpr_vecchia_logp_grad(h, pp, npar, float(noise), C.byref(out), _addr(g), _addr(c), C.byref(fl) if flagged else None)
    return rc, out.value, g, c, fl.value


def kernel_id(name):
    return grad_dict[name].kernel_id
