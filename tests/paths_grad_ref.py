"""Reference of the sample paths' gradients (gprc_gpr_paths_eval_grad, gprc_dev_feature_gemm_grad, gprc_dev_kernel_gemm_grad,
SamplePaths.paths_grad) for the tests (tests/test_paths_grad_cpu.py, tests/test_gpu_paths_grad.py), written from the formula and nothing
else.  No GPU, no torch.  With c = sqrt(2 / D), t_k = nu_k . x + u_k and (k, h, t) as kernel_ref.pairwise returns them:

    d f_s / d x_c = -2 pi c sum_k nu_ck sin(2 pi t_k) W[k, s]  -  t_c sum_j h(x, x_j) (x_c - x_jc) U[j, s]

Everything in `dtype` (numpy.float64, or numpy.longdouble: the twin).  The problems are paths_ref's own, with one test point replaced by
a training point (gammaexp has h = 0 there, the Matern kernels a finite h and a zero difference); the product problems are paths_ref's
unchanged.  Gradients are n* x S x d arrays, [i, s, c], as the library returns them.

The two maximisation problems of the tests (maximize_paths on the numpy evaluator here, SamplePaths.maximize on the device) are stated
here too, with their draws.
"""
import numpy as np

import paths_ref as R
from kernel_ref import pairwise
from paths_ref import gamma, two_pi

LD = np.longdouble
TRAIN_POINT = 17          # the training point that replaces the last test point


def problem(index):
    """paths_ref.problem(index) with the last test point replaced by training point TRAIN_POINT"""
    X, y, Xs, nu, phase, W, E = R.problem(index)
    Xs = np.array(Xs, order="F")
    Xs[:, -1] = X[:, TRAIN_POINT]
    return X, y, Xs, nu, phase, W, E


def feature_grad(nu, phase, A, B, dtype=np.float64):
    """d / da_ic of Phi(A) B: rows x S x d in dtype"""
    nu, phase, A, B = (np.asarray(v, dtype=dtype) for v in (nu, phase, A, B))
    sin = np.sin(two_pi(dtype) * (A.T @ nu + phase[None, :]))
    return np.stack([-two_pi(dtype) * ((sin * nu[c][None, :]) @ B) for c in range(nu.shape[0])], axis=2)


def kernel_grad(name, par, A, Bpts, B, dtype=np.float64):
    """d / da_ic of K(A, Bpts) B: rows x S x d in dtype"""
    A, Bpts, B = (np.asarray(v, dtype=dtype) for v in (A, Bpts, B))
    _, h, t = pairwise(name, par, A, Bpts, dtype)
    return np.stack([-t[c] * ((h * (A[c][:, None] - Bpts[c][None, :])) @ B) for c in range(A.shape[0])], axis=2)


def values(name, par, X, nu, phase, W, U, Xs, dtype=np.float64):
    """the paths at Xs from given weights U (paths_ref.paths' last line): n* x S in dtype"""
    W, U = np.asarray(W, dtype=dtype), np.asarray(U, dtype=dtype)
    c = np.sqrt(dtype(2) / dtype(W.shape[0]))
    return c * (R.features(nu, phase, Xs, dtype) @ W) + pairwise(name, par, Xs, X, dtype)[0] @ U


def grad(name, par, X, nu, phase, W, U, Xs, dtype=np.float64):
    """the paths' gradients at Xs from given weights U: n* x S x d in dtype"""
    c = np.sqrt(dtype(2) / dtype(np.asarray(W).shape[0]))
    return c * feature_grad(nu, phase, Xs, W, dtype) + kernel_grad(name, par, Xs, X, U, dtype)


def paths_grad(name, par, X, y, noise, nu, phase, W, E, Xs, dtype=np.float64):
    """(F n* x S, dF n* x S x d, U n x S) in dtype"""
    F, U = R.paths(name, par, X, y, noise, nu, phase, W, E, Xs, dtype)
    return F, grad(name, par, X, nu, phase, W, U, Xs, dtype), U


def central_differences(name, par, X, nu, phase, W, U, Xs, h, dtype=LD):
    """(f(x + h e_c) - f(x - h e_c)) / (2 h) of `values`, n* x S x d in dtype"""
    Xs = np.asarray(Xs, dtype=dtype)
    out = []
    for c in range(Xs.shape[0]):
        step = np.zeros_like(Xs)
        step[c] = dtype(h)
        out.append((values(name, par, X, nu, phase, W, U, Xs + step, dtype) - values(name, par, X, nu, phase, W, U, Xs - step, dtype)) / (dtype(2) * dtype(h)))
    return np.stack(out, axis=2)


# ---- the two products alone and their componentwise bounds (derivation: tests/test_gpu_paths_grad.py) --------------------------------------
def feature_grad_product(nu, phase, A, B, dtype=np.float64):
    """(out rows x S x d, bound): gamma_{D+3} 2 pi (|nu_c o sin| |B|) + gamma_{d+1} 4 pi^2 sum_j (sum_c' |nu_c'j a_ic'| + |u_j|) |nu_cj| |B_js|"""
    d, D = np.asarray(nu).shape
    out = feature_grad(nu, phase, A, B, dtype)
    nu64, A64, ph64, absB = (np.abs(np.asarray(v, dtype=float)) for v in (nu, A, phase, B))
    sin = np.abs(np.sin(two_pi(dtype) * (np.asarray(A, dtype=dtype).T @ np.asarray(nu, dtype=dtype) + np.asarray(phase, dtype=dtype)[None, :]))).astype(float)
    mag = A64.T @ nu64 + ph64[None, :]
    bound = np.stack([gamma(D + 3) * 2.0 * np.pi * ((sin * nu64[c][None, :]) @ absB) + gamma(d + 1) * 4.0 * np.pi ** 2 * ((mag * nu64[c][None, :]) @ absB)
                      for c in range(d)], axis=2)
    return out, bound


def kernel_grad_product(name, par, A, Bpts, B, dtype=np.float64):
    """(out rows x S x d, bound): gamma_{cols+d+4} (|G_c| |B|), G_c[i, j] = t_c h_ij (a_ic - b_jc)"""
    A_, P_ = np.asarray(A, dtype=dtype), np.asarray(Bpts, dtype=dtype)
    d, cols = P_.shape
    out = kernel_grad(name, par, A, Bpts, B, dtype)
    _, h, t = pairwise(name, par, A_, P_, dtype)
    absB = np.abs(np.asarray(B, dtype=float))
    bound = np.stack([gamma(cols + d + 4) * (np.abs(t[c] * h * (A_[c][:, None] - P_[c][None, :])).astype(float) @ absB) for c in range(d)], axis=2)
    return out, bound


def product_grad_reference(index, dtype=np.float64):
    what, name, par, *_ = R.PRODUCTS[index]
    A, P, phase, B = R.product_problem(index)
    return feature_grad_product(P, phase, A, B, dtype) if what == "features" else kernel_grad_product(name, par, A, P, B, dtype)


# ---- the maximisation problems -----------------------------------------------------------------------------------------------------------
# (kernel, parameters, d, n, S, starts, D, noise, box, grid points per axis)
MAXIMA = [
    dict(name="sqrexp", par=[0.5], d=1, n=40, S=8, starts=16, D=512, noise=0.05, box=(-2.0, 2.0), grid=20001),
    dict(name="matern52_ard", par=[0.6, 1.4], d=2, n=300, S=8, starts=32, D=512, noise=0.05, box=(-2.0, 2.0), grid=401),
]
MAXIMA_SEEDS = (0, 1, 2)


def maxima_problem(which, seed):
    """(X d x n, y, nu, phase, W, E) of maximisation problem `which`: the frequencies from the kernel's spectral density in cycles (sqrexp:
    z / l; matern52_ard: z / l_c times sqrt(5 / chi^2_5)), drawn in the order sampling.spectral_frequencies documents, then phase, W, E
    as GPR.sample_paths draws them"""
    m = MAXIMA[which]
    d, n, D, S = m["d"], m["n"], m["D"], m["S"]
    rng = np.random.default_rng(500 + 10 * which + seed)
    X = rng.uniform(m["box"][0], m["box"][1], (d, n))
    y = np.sin(3.0 * X[0]) * np.cos(X[d - 1]) + np.sqrt(m["noise"]) * rng.normal(size=n)
    omega = rng.standard_normal((D, d)) / np.asarray(m["par"])[None, :]
    if m["name"].startswith("matern52"):
        omega = omega * np.sqrt(5.0 / rng.chisquare(5.0, D))[:, None]
    nu = np.asfortranarray(omega.T / (2.0 * np.pi))
    phase = rng.random(D)
    W = np.asfortranarray(rng.standard_normal((S, D)).T)
    E = np.asfortranarray(rng.standard_normal((S, n)).T)
    return np.asfortranarray(X), y, nu, phase, W, E


def maxima_grid(which):
    """the grid of problem `which` as d x points"""
    m = MAXIMA[which]
    ax = np.linspace(m["box"][0], m["box"][1], m["grid"])
    if m["d"] == 1:
        return np.asfortranarray(ax[None, :])
    g0, g1 = np.meshgrid(ax, ax, indexing="ij")
    return np.asfortranarray(np.vstack([g0.ravel(), g1.ravel()]))


def check_maxima(res, grid_max, fmax, lower, upper):
    """the four conditions on a PathMaxima but the bits: (worst shortfall of a best value below its grid maximum, in units of fmax; worst
    projected-gradient norm of the best points; all inside the box)"""
    S = res.f_best.size
    Q = res.f.size
    best_pg = []
    for s in range(S):
        cand = np.arange(Q)[np.arange(Q) % S == s]
        hit = cand[np.all(res.x[:, cand] == res.x_best[:, s:s + 1], axis=0) & (res.f[cand] == res.f_best[s])]
        assert hit.size >= 1
        best_pg.append(res.pg[hit[0]])
    short = float(((grid_max - res.f_best) / fmax).max())
    inside = bool(((res.x >= lower[:, None]) & (res.x <= upper[:, None])).all() and ((res.x_best >= lower[:, None]) & (res.x_best <= upper[:, None])).all())
    return short, float(max(best_pg)), inside
