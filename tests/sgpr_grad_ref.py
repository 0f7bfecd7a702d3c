"""numpy reference of the gradient of the sparse GPR's collapsed bound (gprc_sgpr_elbo_grad, fit.elbo_grad) for
tests/test_sgpr_grad_cpu.py and tests/test_gpu_sgpr_grad.py, written from the formulas below and nothing else.  No GPU, no torch.

Notation of tests/sgpr_ref.py (s2 = noise, the variance), and
    q = L_B^-T c,   mu = L_u^-T q,   r = y - V q
    G_fu (n x m) = [ V (I - B^-1) L_u^-1 + r mu^T ] / s2
    G_uu (m x m) = 1/2 L_u^-T (2 I - B^-1 - B) L_u^-1 - 1/2 mu mu^T                                  (symmetric)
    d elbo / d theta = sum_ij G_fu,ij dk(x_i,z_j)/d theta + sum_jk G_uu,jk dk(z_j,z_k)/d theta       (the jitter is a constant)
    d elbo / d z_jc  = sum_i G_fu,ij dk(x_i,z_j)/d z_jc + 2 sum_k G_uu,jk dk(z_k,z_j)/d z_jc,        dk(x,z)/d z_c = h (x_c - z_c) t_c
    d elbo / d s2    = -n/(2 s2) + (m - tr B^-1)/(2 s2) + y^T y/(2 s2^2) - c^T c/(2 s2) - q^T q/(2 s2) + t/(2 s2^2)

dK / dtheta comes from kernel_ref.kernel_derivs on the stacked points [Z | X], h and t from kernel_ref.pairwise, K from sgpr_ref.blocks,
all in float64 in both dtypes (the comparison is of the algebra, as in sgpr_ref); the algebra runs in float64 (LAPACK) or in
numpy.longdouble (pred_grad_ref's column Cholesky and substitutions).  X is d x n, Z d x m, one point per column; parameter vectors in
the C ABI's order; the gradient is [d / d theta_1 .. d / d theta_p, d / d s2], dZ is d x m.
"""
import numpy as np

from kernel_ref import kernel, kernel_derivs, pairwise
from pred_grad_ref import chol, solve_lower
import sgpr_ref as R

LD = np.longdouble
NOISE, JITTER = 0.05, 1e-6

# (kernel name, parameters, n, m, d): n and m off every tile size; case i draws from sgpr_ref.problem(20 + i, ...)
CASES = [
    ("sqrexp", [0.6], 700, 200, 3),                          # baseline
    ("matern52_ard", [0.6, 0.85, 1.1], 700, 200, 3),         # ARD Matern
    ("matern32", [0.1], 900, 600, 2),                        # m_pad = 1024: two panels, cross-panel tiles
    ("rationalquadratic", [0.2, 1.5], 500, 130, 2),          # m barely over one 128-block
    ("gammaexp", [0.8, 1.5], 500, 130, 2),                   # s = 0 pairs (Z is a subset of X)
    ("sqrexp_ard", list(np.linspace(2.0, 3.0, 20)), 600, 150, 20),   # d > 16: second staging pass; d > 8
    ("matern32_ard", list(np.linspace(0.9, 1.6, 9)), 400, 100, 9),   # ARD with d just over 8
    ("matern52", [0.9], 400, 100, 3),                        # isotropic Matern 5/2
]
# The length scales of cases 2 and 3 are as short as the float64 formulas need to stand within 1e-12 of longdouble on dZ (measured:
# matern32 {0.8} 5.4e-11, {0.35} 8.9e-12, {0.25} 2.1e-12, {0.1} 2.0e-13; rationalquadratic {0.7} 1.9e-11, {0.3} 1.9e-12, {0.2} 1.8e-13):
# dZ is the difference of two parts thirteen times its size there, and G_fu, G_uu carry the conditioning of K_uu and B.
CASE_IDS = ["%d-%s" % (i, c[0]) for i, c in enumerate(CASES)]


def problem(index):
    """(X, y, Z) of case `index` (sgpr_ref.problem's inputs: Z is m distinct columns of X)"""
    _, _, n, m, d = CASES[index]
    X, y, Z, _ = R.problem(20 + index, n, m, d, n_star=1)
    return X, y, Z


def derivative_blocks(name, theta, X, Z):
    """float64: (list of (dK_uu, dK_fu) per parameter, (h_fu, diff_fu, h_uu, diff_uu, t)); diff_fu[c, i, j] = x_ic - z_jc, diff_uu[c, k, j] =
    z_kc - z_jc"""
    m = Z.shape[1]
    S = np.hstack([Z, X])
    dKs = [(dK[:m, :m].copy(), dK[m:, :m].copy()) for dK in kernel_derivs(name, theta, S, kernel(name, theta, S))]
    _, h_fu, t = pairwise(name, theta, X, Z, np.float64)
    _, h_uu, _ = pairwise(name, theta, Z, Z, np.float64)
    return dKs, (h_fu, X[:, :, None] - Z[:, None, :], h_uu, Z[:, :, None] - Z[:, None, :], t)


def elbo_grad(name, theta, X, y, noise, Z, jitter, dtype=np.float64, with_terms=False):
    """dict(elbo, grad, dZ) in dtype; with_terms: also G_fu, G_uu (what the contraction kernel is given)"""
    X, Z = np.asarray(X, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    n, m = X.shape[1], Z.shape[1]
    Kb = R.blocks(name, theta, X, Z, X[:, :1])
    dKs, (h_fu, diff_fu, h_uu, diff_uu, t) = derivative_blocks(name, theta, X, Z)
    uu, fu = np.asarray(Kb["uu"], dtype=dtype), np.asarray(Kb["fu"], dtype=dtype)
    kff = np.asarray(Kb["ff_diag"], dtype=dtype)
    y = np.asarray(y, dtype=dtype)
    s2, half, two, one = dtype(noise), dtype(1) / dtype(2), dtype(2), dtype(1)
    eye = np.eye(m, dtype=dtype)
    Lu = chol(uu + dtype(jitter) * eye)
    Vt = solve_lower(Lu, fu.T)                                   # m x n
    B = eye + (Vt @ Vt.T) / s2
    LB = chol(B)
    c = solve_lower(LB, (Vt @ y)[:, None])[:, 0] / s2
    q = solve_lower(LB, c[:, None], transpose=True)[:, 0]
    mu = solve_lower(Lu, q[:, None], transpose=True)[:, 0]
    r = y - Vt.T @ q
    EB = solve_lower(LB, eye)                                    # L_B^-1
    Binv = EB.T @ EB
    Eu = solve_lower(Lu, eye)                                    # L_u^-1
    G_fu = (Vt.T @ ((eye - Binv) @ Eu) + np.outer(r, mu)) / s2
    G_uu = half * (Eu.T @ (two * eye - Binv - B) @ Eu) - half * np.outer(mu, mu)
    G_uu = half * (G_uu + G_uu.T)
    tr = (kff - (Vt * Vt).sum(0)).sum()
    pi = np.arccos(dtype(-1))
    elbo = -half * dtype(n) * np.log(two * pi * s2) - np.log(np.diag(LB)).sum() - (y @ y) / (two * s2) + half * (c @ c) - tr / (two * s2)
    grad = [(G_fu * np.asarray(dfu, dtype=dtype)).sum() + (G_uu * np.asarray(duu, dtype=dtype)).sum() for duu, dfu in dKs]
    grad.append(-dtype(n) / (two * s2) + (dtype(m) - np.trace(Binv)) / (two * s2) + (y @ y) / (two * s2 * s2) - (c @ c) / (two * s2)
                - (q @ q) / (two * s2) + tr / (two * s2 * s2))
    wf = G_fu * np.asarray(h_fu, dtype=dtype)                     # n x m
    wu = G_uu.T * np.asarray(h_uu, dtype=dtype)                   # [k, j] = G_uu[j, k] h(z_k, z_j)
    dZ = ((wf[None, :, :] * np.asarray(diff_fu, dtype=dtype)).sum(1) + two * (wu[None, :, :] * np.asarray(diff_uu, dtype=dtype)).sum(1))
    dZ = dZ * np.asarray(t, dtype=dtype)[:, None]
    out = dict(elbo=elbo, grad=np.array(grad, dtype=dtype), dZ=dZ)
    if with_terms:
        out.update(G_fu=G_fu, G_uu=G_uu)
    return out


def elbo_ld(name, theta, X, y, noise, Z, jitter):
    """the bound alone in longdouble through sgpr_ref (what the central differences difference)"""
    return R.sgpr(name, theta, X, y, noise, Z, jitter, X[:, :1], dtype=LD)["elbo"]


def cross_terms(name, theta, G, A, Z):
    """float64, for the contraction kernel alone on an arbitrary G (rows x cols): (list per parameter of the rows x cols terms
    G_ij dk(a_i, z_j) / d theta_p, the d x rows x cols terms G_ij dk(a_i, z_j) / d z_jc)"""
    rows = A.shape[1]
    S = np.hstack([A, Z])
    th = [G * dK[:rows, rows:] for dK in kernel_derivs(name, theta, S, kernel(name, theta, S))]
    _, h, t = pairwise(name, theta, A, Z, np.float64)
    z = (G * h)[None, :, :] * (A[:, :, None] - Z[:, None, :]) * t[:, None, None]
    return th, z
