"""What tests/test_batch_predict_grad_cpu.py, tests/test_gpu_batch_predict_grad.py and tests/test_gpu_batch_loo.py share: the test points
of a grid entry of batch_ref, the references (pred_grad_ref.predict_grad and loo_ref.loo in float64, computed once per grid entry and
never changed), a float64 numpy model of exactly the two kernels' algorithm, the error measures, and the raw C-ABI calls.  A plain
module: importing it needs no GPU.

    K_y = K + noise I = L L^T,  W = L^-1 formed explicitly,  alpha = W^T (W y),  K*[k, j] = k(x_k, x*_j),  V = W K*,  U = W^T V
    d mean_j / d x*_c = -t_c sum_k alpha_k h_kj (x*_jc - x_kc),     d var_j / d x*_c = 2 t_c sum_k U_kj h_kj (x*_jc - x_kc)
    p_i = sum_k W_ki^2,  mean_i = y_i - alpha_i / p_i,  var_i = 1 / p_i,  logdens_i = 1/2 log p_i - alpha_i^2 / (2 p_i) - 1/2 log 2 pi
(h and t of every kernel: kernel_ref.pairwise.)
"""
import math

import numpy as np
from scipy.linalg import solve_triangular

import batch_predict_ref as P
import batch_ref as R
import loo_ref
import pred_grad_ref as G
from gprc_amd import _native as nat
from kernel_ref import pairwise

LD = np.longdouble
NS = P.NS


# ---- the test points ----------------------------------------------------------------------------------------------------------------------
_POINTS = {}


def grid_points(case, n):
    """batch_predict_ref.grid_points(case, n), except at n = 1: there its points inside the box are the one training point and the
    far points see nothing, so every gradient would be exactly 0.  At n = 1: 37 points drawn uniformly within +-2 of the training
    point in every coordinate, point 0 the training point itself."""
    if n != 1:
        return P.grid_points(case, n)
    if case not in _POINTS:
        X = R.models(case, 1)[1]
        rng = np.random.default_rng(60_000 + X.shape[0])
        Xs = X[:, :1] + rng.uniform(-2, 2, (X.shape[0], NS))
        Xs[:, 0] = X[:, 0]
        _POINTS[case] = np.asfortranarray(Xs)
    return _POINTS[case]


# ---- the references, computed once ------------------------------------------------------------------------------------------------------------
_GREFS, _LREFS = {}, {}


def grad_references(case, n):
    """per model of the grid entry: (mean, var, dmean[d, NS], dvar[d, NS]) of pred_grad_ref.predict_grad in float64 at grid_points"""
    key = (case, n)
    if key not in _GREFS:
        name, X, y, thetas, noises = R.models(case, n)
        Xs = grid_points(case, n)
        _GREFS[key] = [G.predict_grad(name, th, X, y, nz, Xs) for th, nz in zip(thetas, noises)]
    return _GREFS[key]


def loo_references(case, n):
    """per model of the grid entry: loo_ref.loo's dict in float64"""
    key = (case, n)
    if key not in _LREFS:
        name, X, y, thetas, noises = R.models(case, n)
        _LREFS[key] = [loo_ref.loo(name, th, X, y, nz) for th, nz in zip(thetas, noises)]
    return _LREFS[key]


# ---- the kernels' algorithm in float64 --------------------------------------------------------------------------------------------------------
def _fit(name, theta, X, y, noise):
    X, y = np.asarray(X, dtype=float), np.asarray(y, dtype=float)
    n = X.shape[1]
    K = pairwise(name, theta, X, X, np.float64)[0]
    L = np.linalg.cholesky(K + noise * np.eye(n))
    W = solve_triangular(L, np.eye(n), lower=True)
    return X, y, W, W.T @ (W @ y)


def numpy_model(name, theta, X, y, noise, Xs):
    """(mean, var, dmean[d, m], dvar[d, m]) by the batched gradient kernel's algorithm in float64"""
    X, y, W, alpha = _fit(name, theta, X, y, noise)
    Xs = np.asarray(Xs, dtype=float)
    ks, h, t = pairwise(name, theta, Xs, X, np.float64)     # m x n
    V = W @ ks.T                                            # n x m
    U = W.T @ V                                             # n x m: K_y^-1 k*
    diff = Xs[:, :, None] - X[:, None, :]                   # d x m x n
    dmean = -t[:, None] * (diff * (h * alpha[None, :])[None]).sum(2)
    dvar = 2.0 * t[:, None] * (diff * (h * U.T)[None]).sum(2)
    return ks @ alpha, 1.0 - (V * V).sum(0), dmean, dvar


def numpy_loo(name, theta, X, y, noise):
    """dict(mean, var, ell, loo) by the batched LOO kernel's algorithm in float64"""
    X, y, W, alpha = _fit(name, theta, X, y, noise)
    p = (W * W).sum(0)
    ell = 0.5 * np.log(p) - alpha * alpha / (2.0 * p) - 0.5 * math.log(2.0 * math.pi)
    return dict(mean=y - alpha / p, var=1.0 / p, ell=ell, loo=ell.sum())


# ---- the error measures ---------------------------------------------------------------------------------------------------------------------
def loo_errors(got, ref, y):
    """(mean relative to max |y| -- the LOO mean is exactly 0 at n = 1 and cannot be its own scale --, variance per component relative
    to itself, logdens normwise, the score relative); got, ref: dicts with mean, var, ell, loo"""
    scale = float(np.abs(np.asarray(y, dtype=float)).max())
    e_mean = float(np.abs(np.asarray(got["mean"]) - np.asarray(ref["mean"])).max()) / scale
    return dict(mean=e_mean, var=P.var_err(got["var"], ref["var"]), logdens=G.nerr(got["ell"], ref["ell"]),
                score=float(abs(got["loo"] - ref["loo"]) / abs(ref["loo"])))


def by_coordinate(row, d, ns):
    """one model's gradients as the library lays them out, [j][c] at d j + c, as a d x ns array (pred_grad_ref's orientation)"""
    return np.asarray(row)[:d * ns].reshape(ns, d).T


# ---- the raw calls --------------------------------------------------------------------------------------------------------------------------
def _addr(a):
    return a if isinstance(a, int) or a is None else nat.ptr(a)


def call_predict_grad(h, B, Xs, ns_max, d, xs_stride=0, ns_each=None, mean=True, var=True, dmean=True, dvar=True, ld_out=None, ld_grad=None, fill=-7.0):
    """the raw gprc_gpr_batch_predict_grad with host outputs: (rc, mean, var, dmean, dvar), B x ld_out and B x ld_grad arrays that start
    as `fill`; an output not asked for is passed as NULL and returned as None; Xs as batch_predict_ref.call_predict's; nothing raises"""
    ld = ns_max if ld_out is None else ld_out
    lg = d * ns_max if ld_grad is None else ld_grad
    ne = None if ns_each is None else np.ascontiguousarray(np.asarray(ns_each, dtype=np.int64))
    m = np.full((B, max(ld, 1)), fill) if mean else None
    v = np.full((B, max(ld, 1)), fill) if var else None
    dm = np.full((B, max(lg, 1)), fill) if dmean else None
    dv = np.full((B, max(lg, 1)), fill) if dvar else None
    rc = nat.lib().gprc_gpr_batch_predict_grad(h, _addr(Xs), ns_max, xs_stride, _addr(ne), _addr(m), _addr(v), ld, _addr(dm), _addr(dv), lg)
    return rc, m, v, dm, dv


def call_loo(h, B, n_max, mean=True, var=True, dens=True, score=True, ld_out=None, fill=-7.0):
    """the raw gprc_gpr_batch_loo with host outputs: (rc, mean, var, logdens, score); B x ld_out arrays and B scores that start as `fill`"""
    ld = n_max if ld_out is None else ld_out
    out = [np.full((B, max(ld, 1)), fill) if want else None for want in (mean, var, dens)]
    sc = np.full(B, fill) if score else None
    rc = nat.lib().gprc_gpr_batch_loo(h, _addr(out[0]), _addr(out[1]), _addr(out[2]), ld, _addr(sc))
    return rc, out[0], out[1], out[2], sc
