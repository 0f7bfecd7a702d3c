"""What tests/test_batch_cpu.py and tests/test_gpu_batch.py share: the grid of small models (cases of case_checks.LOGP_CASES at the edges of
the 16-wide sub-blocks and of the 128 block, six models each), their closed-form references computed once, a float64 numpy model of
exactly the batched kernel's algorithm, and the raw C-ABI call.  A plain module: importing it needs no GPU.

The algorithm of gprc_gpr_batch_logp_grad, which `numpy_model` restates: the explicit inverse W = L^-1 of the Cholesky factor,
alpha = W^T (W y), M = alpha alpha^T - W^T W, dlogp / dtheta = 1/2 sum_ij M_ij dK_ij / dtheta, dlogp / dnoise = 1/2 sum_i M_ii.
"""
import math

import numpy as np
from scipy.linalg import solve_triangular

import ard_grad_ref
from case_checks import LOGP_CASES, logp_case
from gprc_amd import _native as nat
from gprc_amd.fit import grad_dict
from kernel_ref import kernel, kernel_derivs

GRID_CASES = ["sqrexp", "gammaexp1.5", "gammaexp1", "ratquad", "ard3", "ard17", "ard33", "matern32", "matern52", "matern32_ard", "matern52_ard8",
              "matern52_ard17"]
GRID_SIZES = [1, 15, 16, 17, 127, 128]
SCALES = (0.5, 1.0, 2.0)
NOISES = (0.1, 0.01)
GRID = [(case, n) for case in GRID_CASES for n in GRID_SIZES]
GRID_IDS = ["%s-%d" % cn for cn in GRID]


def scaled_theta(name, theta, f):
    """the parameter vector with its length scales multiplied by f: every entry of an ARD kernel, the first of the others"""
    t = np.array(theta, dtype=float)
    if grad_dict[name].kernel_id in nat.ARD_KERNELS:
        return t * f
    t[0] *= f
    return t


_MODELS = {}


def models(case, n):
    """(name, X, y, thetas 6 x p, noises 6) of a grid entry: length scales x {0.5, 1, 2}, noise in {0.1, 0.01}"""
    key = (case, n)
    if key not in _MODELS:
        name, theta, X, y, _ = logp_case(case, n)
        thetas = np.array([scaled_theta(name, theta, f) for f in SCALES for _ in NOISES])
        noises = np.array([nz for _ in SCALES for nz in NOISES])
        _MODELS[key] = (name, np.asfortranarray(X), np.ascontiguousarray(y), thetas, noises)
    return _MODELS[key]


_REFS = {}


def references(case, n):
    """per model of the grid entry: (logp, grad, alpha) of the closed form (ard_grad_ref), computed once and never changed"""
    key = (case, n)
    if key not in _REFS:
        name, X, y, thetas, noises = models(case, n)
        out = []
        for th, nz in zip(thetas, noises):
            lp, g = ard_grad_ref.logp_grad(name, th, X, y, nz)
            out.append((lp, g, ard_grad_ref.gpr_fit(name, th, X, y, nz)["alpha"]))
        _REFS[key] = out
    return _REFS[key]


def numpy_model(name, theta, X, y, noise):
    """(logp, grad, alpha) by the batched kernel's algorithm in float64"""
    X, y = np.asarray(X, dtype=float), np.asarray(y, dtype=float)
    n = X.shape[1]
    K = kernel(name, theta, X)
    L = np.linalg.cholesky(K + noise * np.eye(n))
    W = solve_triangular(L, np.eye(n), lower=True)
    alpha = W.T @ (W @ y)
    logp = -0.5 * float(y @ alpha) - float(np.log(np.diag(L)).sum()) - 0.5 * n * math.log(2.0 * math.pi)
    M = np.outer(alpha, alpha) - W.T @ W
    grad = [0.5 * float(np.sum(M * dK)) for dK in kernel_derivs(name, theta, X, K)]
    grad.append(0.5 * float(np.trace(M)))
    return logp, np.array(grad), alpha


def block_also(case):
    """the parameter block is bounded on its own too (case_checks.LOGP_CASES' last column)"""
    return LOGP_CASES[case][4]


def _addr(a):
    return a if isinstance(a, int) or a is None else nat.ptr(a)


def call_batch(name, thetas, noises, X, d, n_max, y, x_stride=0, y_stride=0, n_each=None, want_grad=True, want_alpha=True, ctx=None,
               logp=True, info=True):
    """the raw gprc_gpr_batch_logp_grad: (rc, logp, grad, alpha, info); X, y: numpy arrays, torch tensors or addresses; an output
    not asked for is passed as NULL and returned as None; nothing raises"""
    kid = name if isinstance(name, int) else grad_dict[name].kernel_id
    thetas = np.ascontiguousarray(np.atleast_2d(np.asarray(thetas, dtype=np.float64)))
    B, p = thetas.shape
    noises = np.ascontiguousarray(np.asarray(noises, dtype=np.float64))
    ne = None if n_each is None else np.ascontiguousarray(np.asarray(n_each, dtype=np.int64))
    lp = np.full(B, -7.0) if logp else None
    g = np.full((B, p + 1), -7.0) if want_grad else None
    al = np.full((B, n_max), -7.0) if want_alpha else None
    inf = np.full(B, -7, dtype=np.intc) if info else None
    ctx = ctx or nat.default_context()
    rc = nat.lib().gprc_gpr_batch_logp_grad(ctx.handle, kid, B, thetas.ctypes.data, p, p, noises.ctypes.data, _addr(X), d, n_max, x_stride, _addr(y),
                                            y_stride, _addr(ne), _addr(lp), _addr(g), _addr(al), _addr(inf))
    return rc, lp, g, al, inf
