"""The reference of the posterior sample paths (tests/paths_ref.py) judged on the CPU, and the frequency samplers.  No GPU.

1. The float64 reference against its longdouble twin on the very inputs of tests/test_gpu_paths.py: it must stand well inside the
   project's TOL = 1e-10, which the GPU tests then hold the library to against IT: gated at TOL / 100.  Measured here
   (normwise, paths | U): at noise 0.1 every case <= 7.1e-14 | 5.9e-14; case 0 again at noise 1e-3: 1.9e-13 | 3.5e-13.
2. The bounds of the two products (test_gpu_paths.py derives them): the float64 numpy product itself lies inside them against the twin
   (at most 0.014 of the bound).
3. sampling.spectral_frequencies: the mean of cos 2 pi nu . r over N = 200 000 frequencies against k(r), within 5 standard errors
   (the standard error from the sample itself), every kernel with a sampler, four displacements each: worst z 1.8.
4. The statistics of the reference with fixed seeds (d = 1, n = 40, sqrexp l = 0.5, noise 0.05, D = 2048, S = 4096, eight test
   points): sample mean within 5 standard errors sqrt(C_D,ii / S) of the exact posterior mean, sample covariance within 5 standard
   errors sqrt((C_ii C_jj + C_ij^2) / S) of the finite-feature covariance C_D.  Worst z-scores over three seeds: mean 2.7, covariance 2.7.
5. The gap max |C_D - exact posterior covariance| is a property of the method (random Fourier features), not of the code: printed
   (0.010, 0.031, 0.010 for the three seeds at D = 2048; 0.058 at D = 256 and 0.0026 at D = 16 384), recorded in DESIGN.md section 7,
   and gated only to be smaller at D = 16 384 than at D = 256 for the same seed.
"""
import numpy as np
import pytest

import paths_ref as R
from conftest import TOL
from gprc_amd.sampling import spectral_frequencies
from gpu_calls import kfun
from kernel_ref import pairwise
from pred_grad_ref import nerr

LD = np.longdouble


@pytest.mark.parametrize("index", range(len(R.CASES)), ids=[R.case_id(i) for i in range(len(R.CASES))])
def test_float64_reference_against_its_longdouble_twin(index):
    name, par, *_ = R.CASES[index]
    X, y, Xs, nu, phase, W, E = R.problem(index)
    for noise in (R.NOISE, 1e-3) if index == 0 else (R.NOISE,):
        F, U = R.paths(name, par, X, y, noise, nu, phase, W, E, Xs)
        Fl, Ul = R.paths(name, par, X, y, noise, nu, phase, W, E, Xs, LD)
        ef, eu = nerr(F.astype(LD), Fl), nerr(U.astype(LD), Ul)
        print("paths_ref %s noise %g: paths %.2e U %.2e" % (R.case_id(index), noise, ef, eu))
        assert max(ef, eu) <= 0.01 * TOL


@pytest.mark.parametrize("index", range(len(R.PRODUCTS)), ids=["%d-%s" % (i, p[1] or p[0]) for i, p in enumerate(R.PRODUCTS)])
def test_float64_products_lie_inside_their_bounds(index):
    out, bound = R.product_reference(index)
    twin, _ = R.product_reference(index, LD)
    ratio = float((np.abs(out.astype(LD) - twin) / bound).max())
    print("product %d %s: worst |float64 - longdouble| / bound %.3f" % (index, R.PRODUCTS[index][:2], ratio))
    assert ratio <= 1.0


SAMPLER_CASES = [("sqrexp", [0.7], 2), ("sqrexp_ard", [0.5, 1.5, 3.0], 3), ("matern32", [0.9], 2), ("matern52", [1.1], 3),
                 ("matern32_ard", [0.5, 1.5], 2), ("matern52_ard", [0.6, 1.4, 2.5], 3), ("rationalquadratic", [0.9, 1.7], 2)]
N_FREQ = 200000


@pytest.mark.parametrize("case", SAMPLER_CASES, ids=[c[0] for c in SAMPLER_CASES])
def test_frequency_samplers_reproduce_the_kernel(case):
    name, par, d = case
    nu = spectral_frequencies(kfun(name, par), d, N_FREQ, np.random.default_rng(5))
    assert nu.shape == (d, N_FREQ) and nu.flags.f_contiguous
    rng = np.random.default_rng(6)
    worst = 0.0
    for scale in (0.1, 0.5, 1.0, 2.0):
        r = rng.standard_normal((d, 1)) * scale
        c = np.cos(2.0 * np.pi * (nu.T @ r)[:, 0])
        k = float(pairwise(name, par, r, np.zeros((d, 1)), np.float64)[0][0, 0])
        z = abs(c.mean() - k) / (c.std(ddof=1) / np.sqrt(N_FREQ))
        worst = max(worst, z)
        assert z <= 5.0, (name, scale, c.mean(), k, z)
    print("sampler %s: worst z %.2f over four displacements, N = %d" % (name, worst, N_FREQ))
    again = spectral_frequencies(kfun(name, par), d, 16, np.random.default_rng(5))
    assert np.array_equal(again, spectral_frequencies(kfun(name, par), d, 16, np.random.default_rng(5)))   # a seed reproduces


def test_kernels_without_a_sampler_raise():
    from gprc_amd import cov_func, linear
    with pytest.raises(ValueError):
        spectral_frequencies(kfun("gammaexp", [1.2, 1.5]), 2, 8, np.random.default_rng(0))
    with pytest.raises(ValueError):
        spectral_frequencies(cov_func(linear, sigma=1.3), 2, 8, np.random.default_rng(0))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_statistics_of_the_reference(seed):
    s = R.STAT
    X, y, Xs = R.stat_problem()
    nu, phase, W, E = R.stat_draws(seed)
    F, _ = R.paths(s["name"], s["par"], X, y, s["noise"], nu, phase, W, E, Xs)
    mean, CD, exact = R.feature_covariance(s["name"], s["par"], X, y, s["noise"], nu, phase, Xs)
    zm, zc = R.stat_z_scores(F, mean, CD)
    print("statistics seed %d: worst z of the mean %.2f, of the covariance %.2f; RFF gap max |C_D - exact| %.4f (max |exact| %.3f)"
          % (seed, zm, zc, np.abs(CD - exact).max(), np.abs(exact).max()))
    assert zm <= 5.0 and zc <= 5.0


def test_feature_gap_shrinks_with_the_number_of_features():
    s = R.STAT
    X, y, Xs = R.stat_problem()
    gaps = {}
    for D in (256, 16384):
        nu, phase, _, _ = R.stat_draws(0, D=D, S=1)
        _, CD, exact = R.feature_covariance(s["name"], s["par"], X, y, s["noise"], nu, phase, Xs)
        gaps[D] = float(np.abs(CD - exact).max())
    print("RFF gap max |C_D - exact posterior covariance|: %s" % gaps)
    assert gaps[16384] < gaps[256]
