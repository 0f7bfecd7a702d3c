"""Reference of the posterior sample paths (gprc_gpr_paths_*, GPR.sample_paths) for the tests (tests/test_paths_cpu.py,
tests/test_gpu_paths.py): pathwise conditioning written from the formulas and nothing else.  No GPU, no torch.

    Phi[i, k] = cos 2 pi(nu_k . x_i + u_k)        nu: d x D in cycles, u: D in turns, c = sqrt(2 / D)
    K_y = K + noise I = L L^T
    U = K_y^-1 (y 1^T - c Phi(X) W - sqrt(noise) E)                                  n x S
    F = c Phi(X*) W + K(X*, X) U                                                     n* x S: the paths at the test points

Everything in `dtype` -- numpy.float64 (LAPACK) or numpy.longdouble, the twin (pred_grad_ref's column Cholesky and substitutions;
2 pi from 4 atan 1 in that type).  Kernels are tests/kernel_ref.py's.  Points are columns, as the library takes them.

The finite-feature covariance, the exact covariance of a path at the test points GIVEN the features (over W and E, standard normal):
    A = K(X*, X) K_y^-1,   G = c (Phi(X*) - A Phi(X)),   C_D = G G^T + noise A A^T
and its mean is A y, the exact posterior mean, whatever the features.  C_D tends to the posterior covariance K** - A K(X, X*) as D grows.
"""
import numpy as np

from kernel_ref import pairwise
from pred_grad_ref import chol, solve_lower

LD = np.longdouble
NOISE = 0.1

# (kernel, parameters in the ABI's order, d, n, n*, D, S): the eight kernels; n_pad 512 and 1024 (a two-panel forward and reversed solve);
# n* 1, 130 (two row tiles), 300; D 1, 6, 260 (over four column tiles); S off 16, over one 64 block, over the 128-row solve block;
# d = 20: two staging passes, ARD with unequal scales
CASES = [
    ("sqrexp", [0.7], 3, 300, 130, 260, 5),
    ("gammaexp", [1.2, 1.5], 3, 300, 1, 6, 1),
    ("rationalquadratic", [0.9, 1.7], 1, 300, 300, 1, 70),
    ("sqrexp_ard", [0.5, 1.5, 3.0], 3, 700, 130, 260, 130),
    ("matern32", [0.9], 3, 300, 130, 260, 5),
    ("matern52", [6.0], 20, 300, 130, 260, 70),
    ("matern32_ard", list(np.linspace(3.0, 9.0, 20)), 20, 300, 300, 6, 5),
    ("matern52_ard", [0.6, 1.4, 2.5], 3, 700, 300, 260, 70),
]


def case_id(index):
    name, _, d, n, ns, D, S = CASES[index]
    return "%d-%s-d%d-n%d-ns%d-D%d-S%d" % (index, name, d, n, ns, D, S)


def problem(index):
    """(X d x n, y, Xs d x n*, nu d x D, phase, W D x S, E n x S) of case `index`: the inputs the GPU tests and the CPU tests share.  The
    frequencies are normal with the scale of the kernel's first length (the arithmetic is judged, not the spectral density)."""
    name, par, d, n, ns, D, S = CASES[index]
    rng = np.random.default_rng(4200 + index)
    X = rng.uniform(-2, 2, (d, n))
    y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
    Xs = rng.uniform(-2, 2, (d, ns))
    nu = rng.standard_normal((d, D)) / (2.0 * np.pi * par[0])
    phase = rng.random(D)
    W = rng.standard_normal((D, S))
    E = rng.standard_normal((n, S))
    return tuple(np.asfortranarray(v) for v in (X, y, Xs, nu, phase, W, E))


def two_pi(dtype):
    return dtype(8) * np.arctan(dtype(1))


def features(nu, phase, X, dtype=np.float64):
    """Phi (points x D) in dtype"""
    nu, phase, X = (np.asarray(v, dtype=dtype) for v in (nu, phase, X))
    return np.cos(two_pi(dtype) * (X.T @ nu + phase[None, :]))


def paths(name, par, X, y, noise, nu, phase, W, E, Xs, dtype=np.float64):
    """(F n* x S, U n x S) in dtype"""
    X, y, Xs, W, E = (np.asarray(v, dtype=dtype) for v in (X, y, Xs, W, E))
    n, D = X.shape[1], W.shape[0]
    c = np.sqrt(dtype(2) / dtype(D))
    L = chol(pairwise(name, par, X, X, dtype)[0] + dtype(noise) * np.eye(n, dtype=dtype))
    R = y[:, None] - c * (features(nu, phase, X, dtype) @ W) - np.sqrt(dtype(noise)) * E
    U = solve_lower(L, solve_lower(L, R), transpose=True)
    F = c * (features(nu, phase, Xs, dtype) @ W) + pairwise(name, par, Xs, X, dtype)[0] @ U
    return F, U


def feature_covariance(name, par, X, y, noise, nu, phase, Xs, dtype=np.float64):
    """(mean, C_D, exact posterior covariance) at the test points, the features given"""
    X, y, Xs = (np.asarray(v, dtype=dtype) for v in (X, y, Xs))
    n, D = X.shape[1], np.asarray(nu).shape[1]
    c = np.sqrt(dtype(2) / dtype(D))
    L = chol(pairwise(name, par, X, X, dtype)[0] + dtype(noise) * np.eye(n, dtype=dtype))
    ks = pairwise(name, par, Xs, X, dtype)[0]                                  # n* x n
    A = solve_lower(L, solve_lower(L, ks.T), transpose=True).T                 # K* K_y^-1
    G = c * (features(nu, phase, Xs, dtype) - A @ features(nu, phase, X, dtype))
    v = solve_lower(L, ks.T)
    return A @ y, G @ G.T + dtype(noise) * (A @ A.T), pairwise(name, par, Xs, Xs, dtype)[0] - v.T @ v


# ---- the two products alone ---------------------------------------------------------------------------------------------------------
U64 = 2.0 ** -53


def gamma(k):
    return k * U64 / (1.0 - k * U64)


def feature_product(nu, phase, A, B, dtype=np.float64):
    """(out rows x S, bound): out = Phi(A) B and the componentwise bound of the float64 product (test_gpu_paths.py states its derivation):
    gamma_{D+1} (|Phi| |B|) + 2 pi gamma_{d+1} sum_j (sum_c |nu_cj a_ic| + |u_j|) |B_js|"""
    d, D = np.asarray(nu).shape
    Phi = features(nu, phase, A, dtype)
    out = Phi @ np.asarray(B, dtype=dtype)
    mag = np.abs(np.asarray(A, dtype=float)).T @ np.abs(np.asarray(nu, dtype=float)) + np.abs(np.asarray(phase, dtype=float))[None, :]
    absB = np.abs(np.asarray(B, dtype=float))
    bound = gamma(D + 1) * (np.abs(Phi).astype(float) @ absB) + 2.0 * np.pi * gamma(d + 1) * (mag @ absB)
    return out, bound


def kernel_product(name, par, A, Bpts, B, dtype=np.float64):
    """(out rows x S, bound): out = K(A, Bpts) B and gamma_{cols+1} (|K| |B|)"""
    K = pairwise(name, par, A, Bpts, dtype)[0]
    out = K @ np.asarray(B, dtype=dtype)
    return out, gamma(np.asarray(Bpts).shape[1] + 1) * (np.abs(K).astype(float) @ np.abs(np.asarray(B, dtype=float)))


# (what, kernel, parameters, rows, cols, d, S): rows over one 128-row tile; cols off 4, and 2117 = 34 column tiles in 17 stripes of two,
# the last tile ragged; d = 20: two staging passes
PRODUCTS = [
    ("features", None, None, 130, 2117, 3, 70),
    ("features", None, None, 129, 67, 20, 5),
    ("kernel", "matern52_ard", [0.6, 1.4, 2.5], 130, 2117, 3, 70),
    ("kernel", "sqrexp", [5.0], 129, 67, 20, 5),
    ("kernel", "gammaexp", [1.2, 1.5], 131, 301, 2, 17),
    ("kernel", "rationalquadratic", [0.9, 1.7], 257, 130, 1, 1),
]


def product_problem(index):
    """(A d x rows, column points or frequencies d x cols, phase, B cols x S) of PRODUCTS[index]"""
    _, name, par, rows, cols, d, S = PRODUCTS[index]
    rng = np.random.default_rng(9100 + index)
    A = rng.uniform(-2, 2, (d, rows))
    P = rng.uniform(-2, 2, (d, cols)) if name else rng.standard_normal((d, cols)) / (2.0 * np.pi)
    return np.asfortranarray(A), np.asfortranarray(P), rng.random(cols), np.asfortranarray(rng.standard_normal((cols, S)))


def product_reference(index, dtype=np.float64):
    what, name, par, *_ = PRODUCTS[index]
    A, P, phase, B = product_problem(index)
    return feature_product(P, phase, A, B, dtype) if what == "features" else kernel_product(name, par, A, P, B, dtype)


# ---- the fixed-seed statistics problem ------------------------------------------------------------------------------------------------
STAT = dict(name="sqrexp", par=[0.5], d=1, n=40, noise=0.05, D=2048, S=4096, n_star=8)


def stat_problem(seed=0):
    """(X 1 x 40, y, Xs 1 x 8) of the statistics tests"""
    rng = np.random.default_rng(77 + seed)
    X = np.sort(rng.uniform(-2, 2, (1, STAT["n"])), axis=1)
    y = np.sin(3.0 * X[0]) + np.sqrt(STAT["noise"]) * rng.normal(size=STAT["n"])
    Xs = np.linspace(-2.3, 2.3, STAT["n_star"]).reshape(1, -1)
    return np.asfortranarray(X), y, np.asfortranarray(Xs)


def stat_draws(seed, D=None, S=None):
    """(nu, phase, W, E) of the statistics problem: sqrexp's frequencies z / l in cycles, drawn here as sampling.spectral_frequencies
    documents its order (one standard_normal((D, d)) call), then phase, W and E as GPR.sample_paths draws them"""
    D, S = D or STAT["D"], S or STAT["S"]
    rng = np.random.default_rng(1234 + seed)
    nu = np.asfortranarray((rng.standard_normal((D, STAT["d"])) / STAT["par"][0]).T / (2.0 * np.pi))
    phase = rng.random(D)
    W = np.asfortranarray(rng.standard_normal((S, D)).T)
    E = np.asfortranarray(rng.standard_normal((S, STAT["n"])).T)
    return nu, phase, W, E


def stat_z_scores(F, mean, C):
    """(worst |z| of the sample mean, worst |z| of the sample covariance) of the paths F (n* x S) against mean and C:
    standard errors sqrt(C_ii / S) and sqrt((C_ii C_jj + C_ij^2) / S)"""
    S = F.shape[1]
    dg = np.diag(C)
    zm = np.abs(F.mean(1) - mean) / np.sqrt(dg / S)
    zc = np.abs(np.cov(F) - C) / np.sqrt((np.outer(dg, dg) + C * C) / S)
    return float(zm.max()), float(zc.max())
