"""numpy float64 reference of the Laplace log evidence of GP classification and its exact gradient (Rasmussen & Williams,
Algorithm 5.1, logistic likelihood, y in {-1, +1}): the reference of tests/test_gpc_grad_cpu.py and tests/test_gpu_gpc_grad.py.

At the mode f of the Newton iteration, with pi = sigmoid(f), W = pi (1 - pi), sw = sqrt(W), g = (y + 1) / 2 - pi, a = K^-1 f:

    B = I + sw K sw = L L^T
    log q = -1/2 a.f + sum log sigmoid(y f) - sum log diag(L)
    R  = sw B^-1 sw                                     (= (K + W^-1)^-1)
    C  = L^-1 (sw K)
    s2 = +1/2 (diag(K) - colSums(C^2)) d3,  d3 = W (2 pi - 1)        (d log q / d f_i; the book prints -1/2 beside grad^3 log p,
                                                                       which is wrong: dW_ii / df_i = -d3_i because W = -grad grad log p)
    per parameter:  s1 = 1/2 a.dK.a - 1/2 sum(R * dK);  b = dK g;  s3 = b - K R b;  d log q / d theta = s1 + s2.s3

This is the book's per-parameter form on purpose: it shares no algebra with the rank-two form the device contracts
(`gradient_rank_two` below restates that one, for the CPU test that pins the two against each other).
The mode search is the device's: from f = 0, stop when |delta objective| < epsilon (absolute), so iteration counts compare.
Kernels and their derivatives come from tests/kernel_ref.py.  Parameter vectors are in the C ABI's order; X is d x n.
"""
import numpy as np
from scipy.linalg import cholesky, solve_triangular

from kernel_ref import kernel, kernel_derivs


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def mode_search(K, y, epsilon, max_iter=1000):
    """(f, a, objective, iterations, decrements): the Newton / IRLS loop; decrements[k] = |objective_{k+2} - objective_{k+1}|"""
    n = K.shape[0]
    f = np.zeros(n)
    last = 0.0
    decrements = []
    for it in range(1, max_iter + 1):
        P = sigmoid(f)
        W = (1.0 - P) * P
        sw = np.sqrt(W)
        b = W * f + (y + 1.0) / 2.0 - P
        L = cholesky(np.eye(n) + (sw[:, None] * sw[None, :]) * K, lower=True)
        t = solve_triangular(L, sw * (K @ b), lower=True)
        t = solve_triangular(L, t, lower=True, trans="T")
        a = b - sw * t
        f = K @ a
        objective = -0.5 * float(a @ f) - float(np.log(1.0 + np.exp(-y * f)).sum())
        if it > 1:
            decrements.append(abs(objective - last))
            if decrements[-1] < epsilon:
                return f, a, objective, it, decrements
        last = objective
    raise ArithmeticError("mode search: iteration cap reached")


def laplace_state(name, theta, X, y, epsilon):
    X = np.asarray(X, dtype=float)
    y = np.asarray(y, dtype=float)
    K = kernel(name, theta, X)
    f, a, objective, iters, decrements = mode_search(K, y, epsilon)
    n = K.shape[0]
    P = sigmoid(f)
    W = P * (1.0 - P)
    sw = np.sqrt(W)
    L = cholesky(np.eye(n) + (sw[:, None] * sw[None, :]) * K, lower=True)
    logq = objective - float(np.log(np.diag(L)).sum())
    Linv_sw = solve_triangular(L, np.diag(sw), lower=True)            # L^-1 diag(sw)
    R = Linv_sw.T @ Linv_sw                                            # sw B^-1 sw
    C = solve_triangular(L, sw[:, None] * K, lower=True)
    s2 = 0.5 * (np.diag(K) - (C * C).sum(0)) * (W * (2.0 * P - 1.0))
    g = (y + 1.0) / 2.0 - P
    return dict(K=K, f=f, a=a, g=g, sw=sw, W=W, L=L, R=R, s2=s2, logq=logq, iters=iters, decrements=decrements)


def logq_grad(name, theta, X, y, epsilon=1e-10):
    """(logq, grad, iterations, decrements) in the book's per-parameter form"""
    st = laplace_state(name, theta, X, y, epsilon)
    K, a, g, R, s2 = st["K"], st["a"], st["g"], st["R"], st["s2"]
    grad = []
    for dK in kernel_derivs(name, theta, np.asarray(X, dtype=float), K):
        s1 = 0.5 * float(a @ dK @ a) - 0.5 * float(np.sum(R * dK))
        b = dK @ g
        s3 = b - K @ (R @ b)
        grad.append(s1 + float(s2 @ s3))
    return st["logq"], np.array(grad), st["iters"], st["decrements"]


def gradient_rank_two(name, theta, X, st):
    """the same gradient as ONE contraction sum_ij M_ij dK_ij with M = 1/2 (a a^T - R) + 1/2 (u g^T + g u^T), u = s2 - R K s2:
    what the device kernel sums (st: laplace_state's result)"""
    K, a, g, R, s2 = st["K"], st["a"], st["g"], st["R"], st["s2"]
    u = s2 - R @ (K @ s2)
    M = 0.5 * (np.outer(a, a) - R) + 0.5 * (np.outer(u, g) + np.outer(g, u))
    return np.array([float(np.sum(M * dK)) for dK in kernel_derivs(name, theta, np.asarray(X, dtype=float), K)])


def logq(name, theta, X, y, epsilon=1e-10):
    K = kernel(name, theta, np.asarray(X, dtype=float))
    y = np.asarray(y, dtype=float)
    f, a, objective, _, _ = mode_search(K, y, epsilon)
    P = sigmoid(f)
    sw = np.sqrt(P * (1.0 - P))
    L = cholesky(np.eye(K.shape[0]) + (sw[:, None] * sw[None, :]) * K, lower=True)
    return objective - float(np.log(np.diag(L)).sum())
