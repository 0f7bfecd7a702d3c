"""numpy float64 closed form of the log marginal likelihood and its exact gradient (explicit inverse): the reference of
tests/test_ard_grad_cpu.py, tests/test_gpu_ard_grad.py and the Matern model tests.

    logp       = -1/2 y.alpha - sum(log(diag(L))) - n/2 log(2 pi),        K_y = K + noise I = L L^T,  alpha = K_y^-1 y
    dlogp/dth  = 1/2 sum_ij (alpha_i alpha_j - (K_y^-1)_ij) dK_ij/dth  =  1/2 (alpha.dK.alpha - sum(K_y^-1 * dK))
    dlogp/dnoise = 1/2 (alpha.alpha - tr(K_y^-1))

K and dK / dtheta of every kernel come from tests/kernel_ref.py (the formula table is there).  Parameter vectors are in the C ABI's
order; X is d x n (one point per column).  Every factorisation is numpy's Cholesky of K_y as it stands: it raises LinAlgError when K_y
is not positive definite, no jitter is ever added.
"""
import math

import numpy as np
from scipy.linalg import solve_triangular

from kernel_ref import kernel, kernel_derivs


def logp(name, theta, X, y, noise):
    X, y = np.asarray(X, dtype=float), np.asarray(y, dtype=float)
    n = X.shape[1]
    L = np.linalg.cholesky(kernel(name, theta, X) + noise * np.eye(n))
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, y))
    return -0.5 * float(y @ alpha) - float(np.log(np.diag(L)).sum()) - 0.5 * n * math.log(2.0 * math.pi)


def logp_grad(name, theta, X, y, noise):
    """(logp, grad): grad has len(theta) + 1 entries, d logp / d noise last"""
    X = np.asarray(X, dtype=float)
    y = np.asarray(y, dtype=float)
    n = X.shape[1]
    K = kernel(name, theta, X)
    Ky = K + noise * np.eye(n)
    L = np.linalg.cholesky(Ky)
    Kinv = np.linalg.inv(Ky)
    Kinv = 0.5 * (Kinv + Kinv.T)
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, y))
    value = -0.5 * float(y @ alpha) - float(np.log(np.diag(L)).sum()) - 0.5 * n * math.log(2.0 * math.pi)
    grad = [0.5 * (float(alpha @ dK @ alpha) - float(np.sum(Kinv * dK))) for dK in kernel_derivs(name, theta, X, K)]
    grad.append(0.5 * (float(alpha @ alpha) - float(np.trace(Kinv))))
    return value, np.array(grad)


def gpr_fit(name, theta, X, y, noise):
    """float64 model: dict(L, alpha, logp), alpha through the other pair of triangular solves"""
    X, y = np.asarray(X, dtype=float), np.asarray(y, dtype=float)
    n = X.shape[1]
    L = np.linalg.cholesky(kernel(name, theta, X) + noise * np.eye(n))
    alpha = solve_triangular(L, solve_triangular(L, y, lower=True), lower=True, trans="T")
    value = -0.5 * float(y @ alpha) - float(np.log(np.diag(L)).sum()) - 0.5 * n * math.log(2.0 * math.pi)
    return dict(L=L, alpha=alpha, logp=value)
