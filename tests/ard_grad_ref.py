"""numpy float64 closed form of the log marginal likelihood and its exact gradient (explicit inverse): the reference of
tests/test_ard_grad_cpu.py and tests/test_gpu_ard_grad.py.

    logp       = -1/2 y.alpha - sum(log(diag(L))) - n/2 log(2 pi),        K_y = K + noise I = L L^T,  alpha = K_y^-1 y
    dlogp/dth  = 1/2 sum_ij (alpha_i alpha_j - (K_y^-1)_ij) dK_ij/dth  =  1/2 (alpha.dK.alpha - sum(K_y^-1 * dK))
    dlogp/dnoise = 1/2 (alpha.alpha - tr(K_y^-1))

with s = |x - y|^2, r = sqrt(s):
    sqrexp (l)               K = exp(-s / (2 l^2))                  dK/dl = K s / l^3
    sqrexp_ard (l_1..l_d)    K = exp(-1/2 sum_k ((x_k-y_k)/l_k)^2)  dK/dl_k = K (x_k - y_k)^2 / l_k^3
    gammaexp (l, gamma)      K = exp(-u), u = (r / l)^gamma         dK/dl = K gamma u / l;  dK/dgamma = -K u log(r / l), 0 at r = 0
    rationalquadratic (l, alpha)  K = q^-alpha, q = 1 + s/(2 alpha l^2)   dK/dl = K s / (l^3 q);  dK/dalpha = K (-log q + (q - 1) / q)
Parameter vectors are in the C ABI's order; X is d x n (one point per column).  Written from the formulas above.
"""
import math

import numpy as np


def sqdist_per_dim(X):
    """generator of the n x n matrices (x_ik - x_jk)^2, k = 0 .. d-1"""
    for k in range(X.shape[0]):
        yield np.subtract.outer(X[k], X[k]) ** 2


def kernel(name, theta, X):
    theta = np.atleast_1d(np.asarray(theta, dtype=float))
    if name == "sqrexp_ard":
        s = sum(sk / (l * l) for sk, l in zip(sqdist_per_dim(X), theta))
        return np.exp(-0.5 * s)
    s = sum(sqdist_per_dim(X))
    if name == "sqrexp":
        return np.exp(-s / (2.0 * theta[0] ** 2))
    if name == "gammaexp":
        return np.exp(-(np.sqrt(s) / theta[0]) ** theta[1])
    if name == "rationalquadratic":
        return (1.0 + s / (2.0 * theta[1] * theta[0] ** 2)) ** (-theta[1])
    raise KeyError(name)


def kernel_derivs(name, theta, X, K):
    """generator of dK / dtheta_i in parameter order (one n x n matrix alive at a time)"""
    theta = np.atleast_1d(np.asarray(theta, dtype=float))
    if name == "sqrexp_ard":
        for sk, l in zip(sqdist_per_dim(X), theta):
            yield K * sk / l ** 3
        return
    s = sum(sqdist_per_dim(X))
    if name == "sqrexp":
        yield K * s / theta[0] ** 3
    elif name == "gammaexp":
        l, g = theta
        r = np.sqrt(s)
        u = (r / l) ** g
        yield K * g * u / l
        with np.errstate(divide="ignore", invalid="ignore"):
            t = u * np.log(r / l)
        t[r == 0.0] = 0.0
        yield -K * t
    elif name == "rationalquadratic":
        l, al = theta
        q = 1.0 + s / (2.0 * al * l * l)
        yield K * s / (l ** 3 * q)
        yield K * (-np.log(q) + (q - 1.0) / q)
    else:
        raise KeyError(name)


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
    logp = -0.5 * float(y @ alpha) - float(np.log(np.diag(L)).sum()) - 0.5 * n * math.log(2.0 * math.pi)
    grad = [0.5 * (float(alpha @ dK @ alpha) - float(np.sum(Kinv * dK))) for dK in kernel_derivs(name, theta, X, K)]
    grad.append(0.5 * (float(alpha @ alpha) - float(np.trace(Kinv))))
    return logp, np.array(grad)
