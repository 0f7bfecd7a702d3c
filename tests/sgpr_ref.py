"""numpy reference of the sparse GPR with inducing points (gprc_sgpr_*, SparseGPR) for tests/test_sgpr_cpu.py and
tests/test_gpu_sgpr.py, written from the formulas below (Titsias 2009, the collapsed bound in its whitened form) and nothing else.
No GPU, no torch.

    K_uu = k(Z,Z) + jitter I = L_u L_u^T          V = K(X,Z) L_u^-T   (n x m, row i = v_i^T)
    B    = I + V^T V / s2    = L_B L_B^T          b = V^T y,   c = L_B^-1 b / s2                       (s2 = noise, the variance)
    t    = sum_i ( k(x_i,x_i) - |v_i|^2 )
    elbo = -n/2 log(2 pi s2) - sum_j log (L_B)_jj - y^T y / (2 s2) + c^T c / 2 - t / (2 s2)
    predict at x*:   v* = L_u^-1 k(Z,x*),  w* = L_B^-1 v*,   mean = w*^T c,   var = k(x*,x*) - |v*|^2 + |w*|^2
    exact:  K_y = K(X,X) + s2 I = L L^T,  alpha = K_y^-1 y,  logp = -1/2 y^T alpha - sum_i log L_ii - n/2 log(2 pi)
            mean = k*^T alpha,  var = k(x*,x*) - |L^-1 k*|^2

Both in float64 (LAPACK) and in numpy.longdouble (pred_grad_ref's column Cholesky and substitutions).  K comes from kernel_ref.kernel on
the stacked points [Z | X | X*], in float64 in both dtypes (the comparison is of the algebra, as in loo_ref).  X is d x n, Z d x m, X*
d x n*, one point per column; parameter vectors in the C ABI's order.
"""
import math

import numpy as np

from kernel_ref import kernel
from pred_grad_ref import chol, solve_lower

LD = np.longdouble

# (kernel name, parameters, n, m, d): the cases of the CPU and the GPU tests; case i draws from numpy.random.default_rng(100 + i)
CASES = [
    ("sqrexp", [0.6], 1500, 300, 3),
    ("matern52_ard", [0.6, 0.85, 1.1], 1500, 300, 3),
    ("matern32", [0.8], 2000, 600, 2),
    ("linear", [1.3], 1000, 200, 3),
    ("rationalquadratic", [0.7, 1.5], 900, 130, 2),
]
NOISE, JITTER, N_STAR = 0.05, 1e-6, 257
TIGHT_CASES = [("sqrexp", [0.3]), ("matern52_ard", [0.6, 0.9])]     # Z = X, jitter = 0, n = 640, d = 2
TIGHT_N, TIGHT_D = 640, 2


def problem(index, n, m, d, n_star=N_STAR):
    """(X, y, Z, X*) of case `index`: X uniform in [-2, 2]^d, y = sin(sum_k x_k) + 0.1 N(0, 1), Z = m distinct columns of X"""
    rng = np.random.default_rng(100 + index)
    X = np.asfortranarray(rng.uniform(-2.0, 2.0, (d, n)))
    y = np.sin(X.sum(0)) + 0.1 * rng.standard_normal(n)
    Z = np.asfortranarray(X[:, np.sort(rng.choice(n, size=m, replace=False))])
    Xs = np.asfortranarray(rng.uniform(-2.0, 2.0, (d, n_star)))
    return X, y, Z, Xs


def blocks(name, theta, X, Z, Xs):
    """the float64 kernel blocks of the stacked points: dict(uu, fu, ff_diag, su, ss_diag, ff, sf)"""
    m, n = Z.shape[1], X.shape[1]
    K = kernel(name, theta, np.hstack([Z, X, Xs]))
    return dict(uu=K[:m, :m], fu=K[m:m + n, :m], ff=K[m:m + n, m:m + n], ff_diag=np.diag(K)[m:m + n].copy(),
                su=K[m + n:, :m], sf=K[m + n:, m:m + n], ss_diag=np.diag(K)[m + n:].copy())


def _col_sums(terms, dtype):
    """sum over axis 0 of the stacked `terms` (arrays of equal column count).  float64: every column by math.fsum, the exactly rounded
    sum of the float64 terms -- k(x,x) - |v|^2 cancels up to seven digits (case 3), and a plain 200-term reduction would put its own
    rounding, which depends on numpy's order of summation, on top of the algebra's; longdouble: numpy's sum"""
    A = np.vstack([np.atleast_2d(np.asarray(t, dtype=dtype)) for t in terms])
    if dtype != np.float64:
        return A.sum(0)
    return np.array([math.fsum(A[:, j]) for j in range(A.shape[1])])


def sgpr_from_blocks(Kb, y, noise, jitter, dtype=np.float64):
    """dict(elbo, t, c, mean, var) of the formulas in dtype from the kernel blocks"""
    uu, fu, su = (np.asarray(Kb[k], dtype=dtype) for k in ("uu", "fu", "su"))
    kff, kss = np.asarray(Kb["ff_diag"], dtype=dtype), np.asarray(Kb["ss_diag"], dtype=dtype)
    y = np.asarray(y, dtype=dtype)
    n, m = fu.shape
    s2, half, two = dtype(noise), dtype(1) / dtype(2), dtype(2)
    Lu = chol(uu + dtype(jitter) * np.eye(m, dtype=dtype))
    Vt = solve_lower(Lu, fu.T)                              # m x n: column i = v_i
    LB = chol(np.eye(m, dtype=dtype) + (Vt @ Vt.T) / s2)
    c = solve_lower(LB, (Vt @ y)[:, None])[:, 0] / s2
    per_point = _col_sums([kff, -(Vt * Vt)], dtype)          # k(x_i,x_i) - |v_i|^2
    t = _col_sums([per_point[:, None]], dtype)[0]
    pi = np.arccos(dtype(-1))
    elbo = -half * dtype(n) * np.log(two * pi * s2) - np.log(np.diag(LB)).sum() - (y @ y) / (two * s2) + half * (c @ c) - t / (two * s2)
    vs = solve_lower(Lu, su.T)                              # m x n*
    ws = solve_lower(LB, vs)
    return dict(elbo=elbo, t=t, c=c, mean=ws.T @ c, var=_col_sums([kss, -(vs * vs), ws * ws], dtype))


def exact_from_blocks(Kb, y, noise, dtype=np.float64):
    """dict(logp, mean, var) of the exact GPR in dtype from the kernel blocks"""
    ff, sf = np.asarray(Kb["ff"], dtype=dtype), np.asarray(Kb["sf"], dtype=dtype)
    kss = np.asarray(Kb["ss_diag"], dtype=dtype)
    y = np.asarray(y, dtype=dtype)
    n = ff.shape[0]
    half = dtype(1) / dtype(2)
    L = chol(ff + dtype(noise) * np.eye(n, dtype=dtype))
    alpha = solve_lower(L, solve_lower(L, y[:, None]), transpose=True)[:, 0]
    pi = np.arccos(dtype(-1))
    logp = -half * (y @ alpha) - np.log(np.diag(L)).sum() - half * dtype(n) * np.log(dtype(2) * pi)
    v = solve_lower(L, sf.T)
    return dict(logp=logp, mean=sf @ alpha, var=_col_sums([kss, -(v * v)], dtype))


def sgpr(name, theta, X, y, noise, Z, jitter, Xs, dtype=np.float64):
    return sgpr_from_blocks(blocks(name, theta, X, Z, Xs), y, noise, jitter, dtype)


def exact(name, theta, X, y, noise, Xs, dtype=np.float64):
    return exact_from_blocks(blocks(name, theta, X, X[:, :1], Xs), y, noise, dtype)
