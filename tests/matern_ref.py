"""numpy reference of the Matern 3/2 and 5/2 kernels, isotropic and ARD, for tests/test_matern_cpu.py and tests/test_gpu_matern.py:
values, the three gradients the library forms from them, written from the formulas below and nothing else.  No GPU, no torch.

With s = sum_k (x_k - y_k)^2, r = sqrt(s), and for ARD rho^2 = sum_k ((x_k - y_k) / l_k)^2:

    matern32      (l)          a = sqrt(3) r / l     K = (1 + a) exp(-a)               g = 3 exp(-a)
    matern52      (l)          a = sqrt(5) r / l     K = (1 + a + a^2 / 3) exp(-a)     g = 5/3 (1 + a) exp(-a)
    matern32_ard  (l_1..l_d)   a = sqrt(3) rho       as matern32
    matern52_ard  (l_1..l_d)   a = sqrt(5) rho       as matern52

    dK / dl   = g s / l^3                      (isotropic)
    dK / dl_k = g (x_k - y_k)^2 / l_k^3        (ARD)
    dk(x*, x) / dx*_c = -g (x*_c - x_c) t_c,   t_c = 1 / l^2 (isotropic), 1 / l_c^2 (ARD)

No derivative holds a 1 / r: at r = 0 the differences are 0 and g is finite, so a coinciding pair contributes an exact 0.

The structure around the kernel is the sibling references': pred_grad_ref's chol / solve_lower (float64 or longdouble), ard_grad_ref's
closed form of the log marginal likelihood's gradient, gpc_grad_ref's mode search.  Those modules' own kernel functions do not know the
Matern names, so the few lines around them are restated here on top of this module's kernels.  Parameter vectors are in the C ABI's
order; X is d x n (one point per column).
"""
import math

import numpy as np
from scipy.linalg import cholesky, solve_triangular

import gpc_grad_ref
from pred_grad_ref import chol, solve_lower

LD = np.longdouble
NAMES = ("matern32", "matern52", "matern32_ard", "matern52_ard")
KERNEL_ID = {"matern32": 7, "matern52": 8, "matern32_ard": 9, "matern52_ard": 10}   # include/gprc_native.h

# (kernel name, parameters in the ABI's order, d): the cases of the prediction-gradient tests, CPU and GPU
CASES = [
    ("matern32", [0.9], 3),
    ("matern52", [1.1], 3),
    ("matern52", [1.5], 8),
    ("matern32_ard", [0.5, 1.5, 3.0], 3),
    ("matern52_ard", [0.6, 1.4, 2.5], 3),
]
SIZES = [(300, 0.1), (600, 0.01)]      # (n, noise)


def is_ard(name):
    return name.endswith("_ard")


def value_and_g(name, rho2, dtype):
    """(K, g) from rho2 = s / l^2 (ARD: the scaled squared distance), in dtype"""
    nu2 = dtype(3) if name.startswith("matern32") else dtype(5)
    a = np.sqrt(nu2 * rho2)
    e = np.exp(-a)
    one = dtype(1)
    if name.startswith("matern32"):
        return (one + a) * e, dtype(3) * e
    if name.startswith("matern52"):
        return (one + a + a * a / dtype(3)) * e, dtype(5) / dtype(3) * (one + a) * e
    raise KeyError(name)


def kernel_and_h(name, par, A, B, dtype):
    """(k, g, t): k[i, j] = k(A[:, i], B[:, j]), g as above, t the d per-coordinate factors; everything in dtype
    (pred_grad_ref.kernel_and_h's shape)"""
    A, B = np.asarray(A, dtype=dtype), np.asarray(B, dtype=dtype)
    d = A.shape[0]
    l = np.asarray(par, dtype=dtype)
    if not is_ard(name):
        assert l.size == 1
        l = np.full(d, l[0], dtype=dtype)
    assert l.size == d
    diff = A[:, :, None] - B[:, None, :]                  # d x m x n
    rho2 = ((diff / l[:, None, None]) ** 2).sum(0)
    k, g = value_and_g(name, rho2, dtype)
    return k, g, dtype(1) / (l * l)


# ---- prediction gradients (pred_grad_ref.fit / mean_var / predict_grad on this module's kernels) ---------------------------------
def fit(name, par, X, y, noise, dtype=np.float64):
    """(L, alpha) of K + noise I in dtype"""
    X = np.asarray(X, dtype=dtype)
    K = kernel_and_h(name, par, X, X, dtype)[0] + dtype(noise) * np.eye(X.shape[1], dtype=dtype)
    L = chol(K)
    yv = np.asarray(y, dtype=dtype).reshape(-1, 1)
    alpha = solve_lower(L, solve_lower(L, yv), transpose=True)[:, 0]
    return L, alpha


def mean_var(name, par, X, L, alpha, Xs, dtype=np.float64):
    """(mean, var) at the test points alone (what the central differences difference)"""
    ks = kernel_and_h(name, par, Xs, X, dtype)[0]        # m x n
    v = solve_lower(L, ks.T)                               # n x m
    return ks @ alpha, np.ones(ks.shape[0], dtype=dtype) - (v * v).sum(0)


def predict_cov(name, par, X, L, alpha, Xs, dtype=np.float64):
    """(mean, full posterior covariance) at the test points"""
    ks = kernel_and_h(name, par, Xs, X, dtype)[0]
    v = solve_lower(L, ks.T)
    return ks @ alpha, kernel_and_h(name, par, Xs, Xs, dtype)[0] - v.T @ v


def predict_grad(name, par, X, y, noise, Xs, dtype=np.float64, factor=None):
    """(mean[m], var[m], dmean[d, m], dvar[d, m]) in dtype; factor: (L, alpha) of fit() to reuse"""
    X, Xs = np.asarray(X, dtype=dtype), np.asarray(Xs, dtype=dtype)
    L, alpha = factor if factor is not None else fit(name, par, X, y, noise, dtype)
    ks, g, t = kernel_and_h(name, par, Xs, X, dtype)      # m x n
    v = solve_lower(L, ks.T)                               # n x m
    w = solve_lower(L, v, transpose=True)                  # n x m: K_y^-1 k*
    mean = ks @ alpha
    var = np.ones(ks.shape[0], dtype=dtype) - (v * v).sum(0)
    diff = Xs[:, :, None] - X[:, None, :]                  # d x m x n
    dk = -g[None, :, :] * diff * t[:, None, None]          # dk(x*_i, x_j) / d x*_ic
    dmean = (dk * alpha[None, None, :]).sum(2)
    dvar = -dtype(2) * (dk * w.T[None, :, :]).sum(2)
    return mean, var, dmean, dvar


# ---- log marginal likelihood (ard_grad_ref's shape) ------------------------------------------------------------------------------
def sqdist_per_dim(X):
    """generator of the n x n matrices (x_ik - x_jk)^2, k = 0 .. d-1"""
    for k in range(X.shape[0]):
        yield np.subtract.outer(X[k], X[k]) ** 2


def _scales(name, theta, d):
    theta = np.atleast_1d(np.asarray(theta, dtype=float))
    if is_ard(name):
        assert theta.size == d
        return theta
    assert theta.size == 1
    return np.full(d, theta[0])


def kernel(name, theta, X):
    X = np.asarray(X, dtype=float)
    rho2 = sum(sk / (l * l) for sk, l in zip(sqdist_per_dim(X), _scales(name, theta, X.shape[0])))
    return value_and_g(name, rho2, np.float64)[0]


def kernel_derivs(name, theta, X, K=None):
    """generator of dK / dtheta_i in parameter order (K is not needed: the derivative goes through g, not through K)"""
    X = np.asarray(X, dtype=float)
    ell = _scales(name, theta, X.shape[0])
    rho2 = sum(sk / (l * l) for sk, l in zip(sqdist_per_dim(X), ell))
    g = value_and_g(name, rho2, np.float64)[1]
    if is_ard(name):
        for sk, l in zip(sqdist_per_dim(X), ell):
            yield g * sk / l ** 3
    else:
        yield g * sum(sqdist_per_dim(X)) / ell[0] ** 3


def logp(name, theta, X, y, noise):
    X, y = np.asarray(X, dtype=float), np.asarray(y, dtype=float)
    n = X.shape[1]
    L = np.linalg.cholesky(kernel(name, theta, X) + noise * np.eye(n))
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, y))
    return -0.5 * float(y @ alpha) - float(np.log(np.diag(L)).sum()) - 0.5 * n * math.log(2.0 * math.pi)


def logp_grad(name, theta, X, y, noise):
    """(logp, grad): grad has len(theta) + 1 entries, d logp / d noise last.  Raises numpy's LinAlgError when K_y is not PD."""
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
    """float64 model: dict(L, alpha, logp); numpy's Cholesky raises when K_y is not positive definite (no jitter is ever added)"""
    X, y = np.asarray(X, dtype=float), np.asarray(y, dtype=float)
    n = X.shape[1]
    L = np.linalg.cholesky(kernel(name, theta, X) + noise * np.eye(n))
    alpha = solve_triangular(L, solve_triangular(L, y, lower=True), lower=True, trans="T")
    value = -0.5 * float(y @ alpha) - float(np.log(np.diag(L)).sum()) - 0.5 * n * math.log(2.0 * math.pi)
    return dict(L=L, alpha=alpha, logp=value)


# ---- Laplace evidence of the classifier (gpc_grad_ref.laplace_state / logq_grad on this module's kernels) ------------------------
def logq_grad(name, theta, X, y, epsilon=1e-10):
    """(logq, grad, iterations, decrements) in the book's per-parameter form; the mode search is gpc_grad_ref's"""
    X = np.asarray(X, dtype=float)
    y = np.asarray(y, dtype=float)
    K = kernel(name, theta, X)
    f, a, objective, iters, decrements = gpc_grad_ref.mode_search(K, y, epsilon)
    n = K.shape[0]
    P = gpc_grad_ref.sigmoid(f)
    W = P * (1.0 - P)
    sw = np.sqrt(W)
    L = cholesky(np.eye(n) + (sw[:, None] * sw[None, :]) * K, lower=True)
    logq = objective - float(np.log(np.diag(L)).sum())
    Linv_sw = solve_triangular(L, np.diag(sw), lower=True)            # L^-1 diag(sw)
    R = Linv_sw.T @ Linv_sw                                            # sw B^-1 sw
    C = solve_triangular(L, sw[:, None] * K, lower=True)
    s2 = 0.5 * (np.diag(K) - (C * C).sum(0)) * (W * (2.0 * P - 1.0))
    g = (y + 1.0) / 2.0 - P
    grad = []
    for dK in kernel_derivs(name, theta, X, K):
        s1 = 0.5 * float(a @ dK @ a) - 0.5 * float(np.sum(R * dK))
        b = dK @ g
        s3 = b - K @ (R @ b)
        grad.append(s1 + float(s2 @ s3))
    return logq, np.array(grad), iters, decrements


def case_id(case):
    name, par, d = case
    return "%s-%s-d%d" % (name, "_".join("%g" % p for p in par), d)
