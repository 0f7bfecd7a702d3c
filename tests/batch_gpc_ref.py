"""What tests/test_batch_gpc_cpu.py, tests/test_gpu_batch_gpc.py and tests/test_gpu_local_gpc.py share: a float64 numpy model of exactly
the batched classifier kernel's algorithm (csrc/kernels_batch_gpc.hip), the tightly converged reference the device is judged against, the
data sets of the GPU tests (so that the references are judged here, on the very inputs the device sees) and the raw C-ABI calls.  A plain
module: importing it needs no GPU.

    loop from f = 0:  pi = sigmoid(f), W = pi (1 - pi), sw = sqrt(W), b = W f + (y + 1) / 2 - pi,  B = I + sw K sw = L L^T,
                      a = b - sw B^-1 (sw K b),  f = K a,  objective = -1/2 a.f - sum log(1 + exp(-y f));  stop: |objective - last| < EPS
    at the mode:      g = (y + 1) / 2 - pi,  Wt = L^-1 diag(sw),  logq = objective - sum log L_ii
    prediction:       fs_bar = K*^T g,   Vfs = k** - |Wt K*|^2   (k(x, x) = 1 for the eight kernels);   P(y* = +1) = the integral of
                      sigmoid(z) N(z; mean fs_bar, sd Vfs) -- the reference passes the VARIANCE as sd (R/GPCclass.R:117), kept

EPS = 1e-12 for every test here (gpu_calls.EPS = 1e-10 belongs to the evidence tests): at 1e-10 the latent mean of the loop's last iterate
is up to 3.3e-11 from the mode, a third of conftest.TOL; at 1e-12 it is within 4.8e-13.  Some models' last decrement lies within 1.2 x EPS,
so the device and numpy may stop one iteration apart: values are compared against the TIGHTLY CONVERGED reference (mode_search plus
three more Newton steps), iteration counts as |delta| <= 1.
"""
import ctypes as C

import numpy as np
from scipy.linalg import cholesky, solve_triangular

import gpc_grad_ref as GR
from gprc_amd import _native as nat
from gprc_amd.fit import grad_dict
from gpu_calls import gpc_problem
from kernel_ref import pairwise
from local_ref import knn_ref, metric_of, predict_points

EPS = 1e-12
EXTRA_STEPS = 3                            # Newton steps past mode_search's stop: the tightly converged reference
CASES = {"sqrexp": ("sqrexp", [0.8], 3), "gammaexp1.5": ("gammaexp", [0.9, 1.5], 3), "ratquad": ("rationalquadratic", [1.1, 1.7], 3),
         "ard3": ("sqrexp_ard", [0.8, 1.1, 1.9], 3), "matern52_ard8": ("matern52_ard", np.linspace(1.0, 3.0, 8), 8)}
SIZES = (1, 2, 15, 16, 17, 127, 128)       # the 16-row block edges of the factor body
LOCAL_N, LOCAL_MS, NS = 1000, (1, 17, 64, 128), 37
MAXITER, NONFINITE = -1, -2                # include/gprc_native.h GPRC_BATCH_GPC_MAXITER, GPRC_BATCH_GPC_NONFINITE


# ---- the algorithm ----------------------------------------------------------------------------------------------------------------------
def kmat(name, theta, A, B):
    return pairwise(name, theta, np.asarray(A, dtype=float), np.asarray(B, dtype=float), np.float64)[0]


def newton_step(K, y, f):
    """(f, a, objective) one IRLS step on from f, by substitution (gpc_grad_ref.mode_search's body)"""
    n = K.shape[0]
    P = GR.sigmoid(f)
    W = (1.0 - P) * P
    sw = np.sqrt(W)
    b = W * f + (y + 1.0) / 2.0 - P
    L = cholesky(np.eye(n) + (sw[:, None] * sw[None, :]) * K, lower=True)
    t = solve_triangular(L, sw * (K @ b), lower=True)
    t = solve_triangular(L, t, lower=True, trans="T")
    a = b - sw * t
    f = K @ a
    return f, a, -0.5 * float(a @ f) - float(np.log(1.0 + np.exp(-y * f)).sum())


def mode_state(K, y, f, objective):
    """what the fit keeps at the mode f: g, sw, L of B, logq"""
    n = K.shape[0]
    P = GR.sigmoid(f)
    sw = np.sqrt(P * (1.0 - P))
    L = cholesky(np.eye(n) + (sw[:, None] * sw[None, :]) * K, lower=True)
    return dict(f=f, g=(y + 1.0) / 2.0 - P, sw=sw, L=L, logq=objective - float(np.log(np.diag(L)).sum()))


def class_prob(fs, vf):
    """the integral by brute force: the trapezoid rule in t = (z - fs) / sd over [-12, 12] with 2401 nodes (the integrand is analytic in a
    strip of half-width pi / sd >= pi for sd <= 1, and k(x, x) = 1 bounds the variance by 1: the rule's error is far below 1e-16),
    sd = the variance"""
    fs, vf = np.atleast_1d(np.asarray(fs, dtype=float)), np.atleast_1d(np.asarray(vf, dtype=float))
    t = np.linspace(-12.0, 12.0, 2401)
    w = np.exp(-0.5 * t * t)
    w /= w.sum()                           # (the rule integrates the density itself to 1 within 1e-30: the rounding of the step goes)
    return (GR.sigmoid(fs[:, None] + vf[:, None] * t[None, :]) * w[None, :]).sum(1)


def predict_by_substitution(st, Ks):
    """(fs_bar, Vfs) as R/GPCclass.R:112-115: Ks = K(X, X*), n x ns"""
    v = solve_triangular(st["L"], st["sw"][:, None] * Ks, lower=True)
    return Ks.T @ st["g"], 1.0 - (v * v).sum(0)


def predict_through_wt(g, Wt, Ks):
    """(fs_bar, Vfs) as the batched predict kernel computes them from the stored g and Wt = L^-1 diag(sw)"""
    V = Wt @ Ks
    return Ks.T @ g, 1.0 - (V * V).sum(0)


def converged(name, theta, X, y, Xs):
    """the tightly converged reference of one model: mode_search at EPS (its iteration count is the one to compare), EXTRA_STEPS more
    Newton steps, then the state at that mode and the predictions at the columns of Xs by substitution"""
    X, y = np.asarray(X, dtype=float), np.asarray(y, dtype=float)
    K = kmat(name, theta, X, X)
    f, _, objective, iters, decrements = GR.mode_search(K, y, EPS)
    for _ in range(EXTRA_STEPS):
        f, _, objective = newton_step(K, y, f)
    st = mode_state(K, y, f, objective)
    fs, vf = predict_by_substitution(st, kmat(name, theta, X, Xs))
    st.update(iters=iters, decrements=decrements, fs=fs, vf=vf, prob=class_prob(fs, vf))
    return st


def numpy_model(name, theta, X, y, Xs, epsilon=EPS, max_iter=100):
    """the kernel's algorithm in float64: the loop at epsilon with the solves as products with the explicit inverse W_B = L^-1, the stop
    rule and the cap, the final factorisation, g and Wt, the prediction through Wt, logq and the class probability"""
    X, y = np.asarray(X, dtype=float), np.asarray(y, dtype=float)
    n = X.shape[1]
    K = kmat(name, theta, X, X)
    f, last, it, info = np.zeros(n), 0.0, 0, None
    while info is None:
        it += 1
        P = GR.sigmoid(f)
        W = (1.0 - P) * P
        sw = np.sqrt(W)
        b = W * f + (y + 1.0) / 2.0 - P
        WB = solve_triangular(cholesky(np.eye(n) + (sw[:, None] * sw[None, :]) * K, lower=True), np.eye(n), lower=True)
        a = b - sw * (WB.T @ (WB @ (sw * (K @ b))))
        f = K @ a
        objective = -0.5 * float(a @ f) - float(np.log(1.0 + np.exp(-y * f)).sum())
        if not np.isfinite(objective):
            info = NONFINITE
        elif it > 1 and abs(objective - last) < epsilon:
            info = 0
        elif it >= max_iter:
            info = MAXITER
        last = objective
    st = mode_state(K, y, f, objective)
    Wt = solve_triangular(st["L"], np.diag(st["sw"]), lower=True)
    fs, vf = predict_through_wt(st["g"], Wt, kmat(name, theta, X, Xs))
    st.update(Wt=Wt, iters=it, info=info, fs=fs, vf=vf, prob=class_prob(fs, vf))
    return st


# ---- the data sets of the GPU tests ---------------------------------------------------------------------------------------------------------
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def case_data(case, n=LOCAL_N):
    """(name, theta, X d x n, y, Xs d x 37) of a case: gpc_problem(n, d); 32 test points uniform in the data's box, then the first five
    training points themselves"""
    def make():
        name, theta, d = CASES[case]
        X, y = gpc_problem(n, d)
        X = np.asfortranarray(X)
        return name, np.asarray(theta, dtype=np.float64), X, np.ascontiguousarray(y), predict_points(X, NS)
    return _cached(("data", case, n), make)


def batch_reference(case, nb):
    """converged() of the first nb points of case_data(case), computed once"""
    def make():
        name, theta, X, y, Xs = case_data(case)
        return converged(name, theta, X[:, :nb], y[:nb], Xs)
    return _cached(("batch", case, nb), make)


def batch_model(case, nb):
    def make():
        name, theta, X, y, Xs = case_data(case)
        return numpy_model(name, theta, X[:, :nb], y[:nb], Xs)
    return _cached(("model", case, nb), make)


def local_neighbours(case, m, n=LOCAL_N):
    name, theta, X, _, Xs = case_data(case, n)
    return knn_ref(X, Xs, min(m, n), metric_of(name, theta))[0]


def local_reference(case, m, n=LOCAL_N, model=False):
    """per test point of case_data(case, n) the converged reference (model: the numpy model) of the classifier of its reference
    neighbours, in reference order: dict of fs, vf, prob, iters (arrays of 37) and single_class (how many neighbourhoods hold one label)"""
    def make():
        name, theta, X, y, Xs = case_data(case, n)
        out = dict(fs=np.empty(NS), vf=np.empty(NS), prob=np.empty(NS), iters=np.empty(NS, dtype=int), single_class=0)
        for j, nb in enumerate(local_neighbours(case, m, n)):
            st = (numpy_model if model else converged)(name, theta, X[:, nb], y[nb], Xs[:, j:j + 1])
            out["fs"][j], out["vf"][j], out["prob"][j], out["iters"][j] = st["fs"][0], st["vf"][0], st["prob"][0], st["iters"]
            out["single_class"] += int(np.all(y[nb] == y[nb][0]))
        return out
    return _cached(("local", case, m, n, model), make)


def var_err(got, ref):
    """per component, relative to the variance itself"""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape and np.isfinite(got).all()
    return float((np.abs(got - ref) / np.abs(ref)).max())


# ---- the raw calls --------------------------------------------------------------------------------------------------------------------
def _addr(a):
    return a if isinstance(a, int) or a is None else nat.ptr(a)


def flat(A):
    """a d x n array as the library reads it: point-major, contiguous"""
    return np.ascontiguousarray(np.asarray(A, dtype=np.float64).ravel(order="F"))


def call_fit(name, thetas, X, d, n_max, y, x_stride=0, y_stride=0, n_each=None, epsilon=EPS, max_iter=0, ctx=None, model=True, logq=True,
             iters=True, info=True, null_ctx=False):
    """the raw gprc_gpc_batch_fit: (rc, handle, logq, iters, info); X, y: numpy arrays, torch tensors or addresses; ctx: a Context (None:
    the default one; null_ctx: the NULL context, which needs no device); nothing raises"""
    kid = name if isinstance(name, int) else grad_dict[name].kernel_id
    thetas = np.ascontiguousarray(np.atleast_2d(np.asarray(thetas, dtype=np.float64)))
    B, p = thetas.shape
    ne = None if n_each is None else np.ascontiguousarray(np.asarray(n_each, dtype=np.int64))
    lq = np.full(B, -7.0) if logq else None
    its = np.full(B, -7, dtype=np.intc) if iters else None
    inf = np.full(B, -7, dtype=np.intc) if info else None
    h = C.c_void_p()
    ch = None if null_ctx else (ctx or nat.default_context()).handle
    rc = nat.lib().gprc_gpc_batch_fit(ch, kid, B, thetas.ctypes.data, p, p, _addr(X), d, n_max, x_stride, _addr(y), y_stride, _addr(ne), float(epsilon),
                                      int(max_iter), C.byref(h) if model else None, _addr(lq), _addr(its), _addr(inf))
    return rc, h, lq, its, inf


def get_f_hat(h, B, n_max):
    out = np.full((B, n_max), -7.0)
    nat.check(nat.lib().gprc_gpc_batch_get_f_hat(h, out.ctypes.data))
    return out


def call_latent(h, B, Xs, ns_max, xs_stride=0, ns_each=None, mean=True, var=True, ld_out=None, fill=-7.0):
    """the raw gprc_gpc_batch_predict_latent with host outputs: (rc, fs_bar, Vfs), B x ld_out arrays that start as `fill`"""
    ld = ns_max if ld_out is None else ld_out
    ne = None if ns_each is None else np.ascontiguousarray(np.asarray(ns_each, dtype=np.int64))
    m = np.full((B, max(ld, 1)), fill) if mean else None
    v = np.full((B, max(ld, 1)), fill) if var else None
    rc = nat.lib().gprc_gpc_batch_predict_latent(h, _addr(Xs), ns_max, xs_stride, _addr(ne), _addr(m), _addr(v), ld)
    return rc, m, v


def call_class(h, B, Xs, ns_max, xs_stride=0, ns_each=None, ld_out=None, fill=-7.0):
    """the raw gprc_gpc_batch_predict_class with a host output: (rc, prob)"""
    ld = ns_max if ld_out is None else ld_out
    ne = None if ns_each is None else np.ascontiguousarray(np.asarray(ns_each, dtype=np.int64))
    p = np.full((B, max(ld, 1)), fill)
    rc = nat.lib().gprc_gpc_batch_predict_class(h, _addr(Xs), ns_max, xs_stride, _addr(ne), p.ctypes.data, ld)
    return rc, p


def free(h):
    nat.lib().gprc_batch_model_free(h)


def lgpc_create(name, theta, X, y, m, epsilon=EPS, max_iter=0, ctx=None):
    """the raw gprc_lgpc_create: (rc, handle)"""
    kid = name if isinstance(name, int) else grad_dict[name].kernel_id
    _, pp, npar = nat.params_array(theta)
    X = np.asfortranarray(X)
    d, n = X.shape
    h = C.c_void_p()
    ctx = ctx or nat.default_context()
    rc = nat.lib().gprc_lgpc_create(ctx.handle, kid, pp, npar, X.ctypes.data, d, n, np.ascontiguousarray(y).ctypes.data, m, float(epsilon), int(max_iter),
                                    C.byref(h))
    return rc, h


def lgpc_predict(h, Xs, ns=None, fs=True, vf=True, prob=True, iters=True, info=True):
    """the raw gprc_lgpc_predict: (rc, fs_bar, Vfs, prob, iters, info); Xs: a d x ns numpy array, or (with ns) a tensor or an address;
    fs, vf, prob: True (a host array that starts as -7), False (NULL) or the caller's tensor"""
    if isinstance(Xs, np.ndarray):
        Xs = np.asfortranarray(Xs)
        ns = Xs.shape[1]
    outs = [np.full(ns, -7.0) if o is True else (None if o is False else o) for o in (fs, vf, prob)]
    its = np.full(ns, -7, dtype=np.intc) if iters else None
    inf = np.full(ns, -7, dtype=np.intc) if info else None
    rc = nat.lib().gprc_lgpc_predict(h, _addr(Xs), ns, _addr(outs[0]), _addr(outs[1]), _addr(outs[2]), _addr(its), _addr(inf))
    return (rc, *outs, its, inf)


def lgpc_free(h):
    nat.lib().gprc_lgpr_free(h)
