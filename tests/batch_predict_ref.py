"""What tests/test_batch_predict_cpu.py and tests/test_gpu_batch_predict.py share: the test-point sets of a data set, the float64 closed
form of the posterior mean and latent variance (computed once per grid entry of batch_ref and never changed), a float64 numpy model of
exactly the batched predict kernel's algorithm, and the raw C-ABI calls.  A plain module: importing it needs no GPU.

    K_y = K + noise I = L L^T,   alpha = K_y^-1 y,   K*[k, j] = k(x_k, x*_j)
    mean_j = sum_k K*[k, j] alpha_k,     var_j = k(x*_j, x*_j) - sum_i V[i, j]^2      (k(x, x) = 1 for the eight kernels)
closed form: V = L^-1 K* by substitution (pred_grad_ref, float64 or longdouble);  the kernel's algorithm, which `numpy_model` restates:
W = L^-1 formed explicitly, alpha = W^T (W y), V = W K* as a product.
"""
import ctypes as C

import numpy as np
from scipy.linalg import solve_triangular

import batch_ref as R
import pred_grad_ref as G
from gprc_amd import _native as nat
from gprc_amd.fit import grad_dict
from kernel_ref import pairwise

LD = np.longdouble
NS = 37          # test points per grid entry
TILE = 16        # test points per wave of the kernel (csrc/gprc_internal.h BATCH_PREDICT_TILE)
TURN = 8 * TILE  # test points per workgroup and turn: a workgroup with more of them loops


def star_points(X, ns=NS, seed=0):
    """d x ns test points of the data set X (d x n), three kinds in this order: ns - min(n, 5) - 3 points drawn uniformly inside the
    data's bounding box, the first min(n, 5) training points themselves, and three points 50 box-widths away from the box (beyond its
    upper corner, its lower corner, and along the first coordinate alone).  A box of no width (n = 1) counts as width 1."""
    X = np.asarray(X, dtype=float)
    d, n = X.shape
    lo, hi = X.min(1), X.max(1)
    width = np.where(hi > lo, hi - lo, 1.0)
    k = min(n, 5)
    rng = np.random.default_rng(50_000 + 1000 * d + n + seed)
    inside = lo[:, None] + (hi - lo)[:, None] * rng.uniform(0, 1, (d, ns - k - 3))
    far = np.stack([hi + 50 * width, lo - 50 * width, np.concatenate([[hi[0] + 50 * width[0]], lo[1:]])], axis=1)
    return np.asfortranarray(np.concatenate([inside, X[:, :k], far], axis=1))


def closed_form(name, theta, X, y, noise, Xs, dtype=np.float64):
    """(mean, var) at the columns of Xs by substitution, everything in dtype"""
    Xd = np.asarray(X, dtype=dtype)
    L, alpha = G.fit(name, theta, Xd, y, noise, dtype)
    return G.mean_var(name, theta, Xd, L, alpha, np.asarray(Xs, dtype=dtype), dtype)


def numpy_model(name, theta, X, y, noise, Xs):
    """(mean, var) by the batched predict kernel's algorithm in float64"""
    X, y = np.asarray(X, dtype=float), np.asarray(y, dtype=float)
    n = X.shape[1]
    K = pairwise(name, theta, X, X, np.float64)[0]
    L = np.linalg.cholesky(K + noise * np.eye(n))
    W = solve_triangular(L, np.eye(n), lower=True)
    alpha = W.T @ (W @ y)
    Ks = pairwise(name, theta, X, Xs, np.float64)[0]       # n x ns
    V = W @ Ks
    return Ks.T @ alpha, 1.0 - (V * V).sum(0)


_POINTS, _REFS = {}, {}


def grid_points(case, n):
    key = (case, n)
    if key not in _POINTS:
        _POINTS[key] = star_points(R.models(case, n)[1])
    return _POINTS[key]


def references(case, n):
    """per model of the grid entry of batch_ref: (mean, var) of the float64 closed form at grid_points(case, n), computed once"""
    key = (case, n)
    if key not in _REFS:
        name, X, y, thetas, noises = R.models(case, n)
        Xs = grid_points(case, n)
        _REFS[key] = [closed_form(name, th, X, y, nz, Xs) for th, nz in zip(thetas, noises)]
    return _REFS[key]


def var_err(got, ref):
    """per component, relative to the variance itself: max_j |got_j - ref_j| / |ref_j|"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and np.isfinite(np.asarray(got, dtype=float)).all()
    return float((np.abs(got - ref) / np.abs(ref)).max())


# ---- the raw calls --------------------------------------------------------------------------------------------------------------------
def _addr(a):
    return a if isinstance(a, int) or a is None else nat.ptr(a)


def call_fit(name, thetas, noises, X, d, n_max, y, x_stride=0, y_stride=0, n_each=None, ctx=None, model=True, logp=True, info=True):
    """the raw gprc_gpr_batch_fit: (rc, handle, logp, info); X, y: numpy arrays, torch tensors or addresses; nothing raises"""
    kid = name if isinstance(name, int) else grad_dict[name].kernel_id
    thetas = np.ascontiguousarray(np.atleast_2d(np.asarray(thetas, dtype=np.float64)))
    B, p = thetas.shape
    noises = np.ascontiguousarray(np.asarray(noises, dtype=np.float64))
    ne = None if n_each is None else np.ascontiguousarray(np.asarray(n_each, dtype=np.int64))
    lp = np.full(B, -7.0) if logp else None
    inf = np.full(B, -7, dtype=np.intc) if info else None
    h = C.c_void_p()
    ctx = ctx or nat.default_context()
    rc = nat.lib().gprc_gpr_batch_fit(ctx.handle, kid, B, thetas.ctypes.data, p, p, noises.ctypes.data, _addr(X), d, n_max, x_stride, _addr(y),
                                      y_stride, _addr(ne), C.byref(h) if model else None, _addr(lp), _addr(inf))
    return rc, h, lp, inf


def get_alpha(h, B, n_max):
    out = np.full((B, n_max), -7.0)
    nat.check(nat.lib().gprc_gpr_batch_get_alpha(h, out.ctypes.data))
    return out


def call_predict(h, B, Xs, ns_max, xs_stride=0, ns_each=None, mean=True, var=True, ld_out=None, fill=-7.0):
    """the raw gprc_gpr_batch_predict with host outputs: (rc, mean, var), B x ld_out arrays that start as `fill`; an output not asked
    for is passed as NULL and returned as None; Xs: a numpy array (point-major), a torch tensor or an address; nothing raises"""
    ld = ns_max if ld_out is None else ld_out
    ne = None if ns_each is None else np.ascontiguousarray(np.asarray(ns_each, dtype=np.int64))
    m = np.full((B, max(ld, 1)), fill) if mean else None
    v = np.full((B, max(ld, 1)), fill) if var else None
    rc = nat.lib().gprc_gpr_batch_predict(h, _addr(Xs), ns_max, xs_stride, _addr(ne), _addr(m), _addr(v), ld)
    return rc, m, v


def free(h):
    nat.lib().gprc_batch_model_free(h)


def flat(Xs):
    """a d x ns array as the library reads it: point-major, contiguous"""
    return np.ascontiguousarray(np.asarray(Xs, dtype=np.float64).ravel(order="F"))
