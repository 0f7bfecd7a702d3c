"""numpy reference of leave-one-out cross-validation (gprc_gpr_loo, gprc_gpr_loo_grad) for tests/test_loo_cpu.py and
tests/test_gpu_loo.py, written from the formulas below (Rasmussen & Williams 5.4.2, eqs. 5.10 - 5.13) and nothing else.  No GPU, no torch.

    K_y = K + noise I = L L^T,   P = K_y^-1,   alpha = P y,   p_i = P_ii
    mu_i = y_i - alpha_i / p_i        var_i = 1 / p_i  (of the NOISY y_i)        ell_i = 1/2 log p_i - alpha_i^2 / (2 p_i) - 1/2 log 2 pi
    LOO = sum_i ell_i
    w_i = alpha_i / p_i,  c_i = (p_i + alpha_i^2) / p_i^2,  u = P w
    M = u alpha^T + alpha u^T - P diag(c) P        dLOO / dtheta = 1/2 sum_ij M_ij dK_ij / dtheta        dLOO / dnoise = 1/2 tr M

Three forms: the closed form in float64 (LAPACK), the same in longdouble (pred_grad_ref's column Cholesky and substitutions), and
`loo_brute`, which really removes point i and solves the (n - 1)-point problem.  K and dK / dtheta come from tests/kernel_ref.py (its eight
gradient kernels; `linear`, values only).  Parameter vectors are in the C ABI's order; X is d x n (one point per column).
"""
import math

import numpy as np

from kernel_ref import kernel, kernel_derivs
from pred_grad_ref import chol, solve_lower

LD = np.longdouble
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def _inverse(Ky):
    """(P, alpha-ready inverse) of a symmetric positive definite matrix in its dtype, through the Cholesky factor"""
    L = chol(Ky)
    Linv = solve_lower(L, np.eye(Ky.shape[0], dtype=Ky.dtype))
    return Linv.T @ Linv


def loo_from_K(K, y, noise, dtype=np.float64):
    """dict(mean, var, ell, loo, M) of the closed form in dtype, from the noise-free kernel matrix"""
    K = np.asarray(K, dtype=dtype)
    y = np.asarray(y, dtype=dtype)
    n = K.shape[0]
    P = _inverse(K + dtype(noise) * np.eye(n, dtype=dtype))
    alpha = P @ y
    p = np.diag(P).copy()
    half = dtype(1) / dtype(2)
    ell = half * np.log(p) - alpha * alpha / (dtype(2) * p) - half * np.log(dtype(2) * np.arccos(dtype(-1)))
    w = alpha / p
    c = (p + alpha * alpha) / (p * p)
    u = P @ w
    M = np.outer(u, alpha) + np.outer(alpha, u) - (P * c[None, :]) @ P
    return dict(mean=y - w, var=dtype(1) / p, ell=ell, loo=ell.sum(), M=M, alpha=alpha, p=p)


def loo(name, theta, X, y, noise, dtype=np.float64):
    """the closed form for kernel `name`; the kernel matrix itself is float64's in both dtypes (the comparison is of the algebra)"""
    return loo_from_K(kernel(name, theta, X), y, noise, dtype)


def loo_grad(name, theta, X, y, noise, dtype=np.float64):
    """(LOO, grad) in dtype: grad has len(theta) + 1 entries, dLOO / dnoise last"""
    X = np.asarray(X, dtype=float)
    K = kernel(name, theta, X)
    r = loo_from_K(K, y, noise, dtype)
    half = dtype(1) / dtype(2)
    grad = [half * (r["M"] * np.asarray(dK, dtype=dtype)).sum() for dK in kernel_derivs(name, theta, X, K)]
    grad.append(half * np.trace(r["M"]))
    return r["loo"], np.array(grad, dtype=dtype)


def loo_brute(name, theta, X, y, noise):
    """(mean, var, ell) by really leaving each point out: fit the other n - 1, predict the NOISY y_i (float64)"""
    X = np.asarray(X, dtype=float)
    y = np.asarray(y, dtype=float)
    n = X.shape[1]
    K = kernel(name, theta, X)
    mean, var, ell = np.empty(n), np.empty(n), np.empty(n)
    for i in range(n):
        keep = np.arange(n) != i
        L = np.linalg.cholesky(K[np.ix_(keep, keep)] + noise * np.eye(n - 1))
        ks = K[keep, i]
        v = solve_lower(L, ks[:, None])[:, 0]
        a = solve_lower(L, solve_lower(L, y[keep][:, None]), transpose=True)[:, 0]
        mean[i] = ks @ a
        var[i] = K[i, i] + noise - v @ v
        ell[i] = -0.5 * math.log(var[i]) - (y[i] - mean[i]) ** 2 / (2.0 * var[i]) - HALF_LOG_2PI
    return mean, var, ell


def loo_score_brute(name, theta, X, y, noise):
    return float(loo_brute(name, theta, X, y, noise)[2].sum())


def cond_Ky(name, theta, X, noise):
    K = kernel(name, theta, X)
    return float(np.linalg.cond(K + noise * np.eye(K.shape[0])))
