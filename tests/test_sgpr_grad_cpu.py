"""The numpy reference of the sparse bound's gradient (tests/sgpr_grad_ref.py) judged without a GPU, on the very cases
tests/test_gpu_sgpr_grad.py runs; the host side of fit.optimize_sparse; the two new symbols of the C ABI.

Bounds: the float64 reference against its longdouble twin 1e-12 (relative on every kernel parameter's entry and on the noise's, normwise
on dZ) -- a hundredth of the 1e-10 the GPU tests allow the library against the float64 reference; the longdouble gradient against
longdouble central differences of sgpr_ref's bound 1e-8 (kernel parameters, noise, three entries of Z, with Z moved off X: gammaexp is
not smooth where an inducing point sits on a training point); at Z = X, jitter 0 (sgpr_ref.TIGHT_CASES) the kernel parameters' and the
noise's entries are those of ard_grad_ref.logp_grad (1e-12) and the bound does not depend on Z: max |dZ| <= 1e-10 max |grad|.

Figures of this file: float64 against longdouble, worst of theta / noise / elbo per case <= 7e-15 and dZ 2.7e-13, 5.4e-14, 2.0e-13, 1.8e-13,
7.8e-15, 1.8e-15, 2.0e-15, 1.5e-14; central differences (one Richardson step, h = 1e-4 relative) <= 2.1e-12 on theta and noise (rationalquadratic's
alpha 9.9e-11), <= 6e-11 on the three entries of Z (rationalquadratic; the others <= 2e-11); Z = X in float64: grad 3.4e-14 / 2.5e-14, elbo 7.0e-14 / 6.5e-15, max |dZ| /
max |grad| 6.4e-12 / 2.6e-15 (sqrexp {0.3} / matern52_ard).
"""
import ctypes
import os

import numpy as np
import pytest

import ard_grad_ref as A
import sgpr_grad_ref as G
import sgpr_ref as R
from gprc_amd import _native as nat
from gprc_amd.fit import optimize_sparse

LD = np.longdouble
REF_TOL, FD_TOL = 1e-12, 1e-8


def rel(a, b):
    return float(abs(a - b) / abs(b))


@pytest.mark.parametrize("index", range(len(G.CASES)), ids=G.CASE_IDS)
def test_float64_reference_against_longdouble(index):
    name, theta, n, m, d = G.CASES[index]
    X, y, Z = G.problem(index)
    r64 = G.elbo_grad(name, theta, X, y, G.NOISE, Z, G.JITTER)
    rld = G.elbo_grad(name, theta, X, y, G.NOISE, Z, G.JITTER, LD)
    errs = {"theta": max(rel(r64["grad"][k], rld["grad"][k]) for k in range(len(theta))), "noise": rel(r64["grad"][-1], rld["grad"][-1]),
            "dZ": float(np.abs(r64["dZ"] - rld["dZ"]).max() / np.abs(rld["dZ"]).max()), "elbo": rel(r64["elbo"], rld["elbo"])}
    print("sgpr gradient reference case %d (%s): %s" % (index, name, {k: "%.2e" % v for k, v in errs.items()}))
    assert max(errs.values()) <= REF_TOL, errs


FD_CASES = [("sqrexp", [0.6], 3), ("matern52_ard", [0.6, 0.85, 1.1], 3), ("matern32", [0.8], 2), ("rationalquadratic", [0.7, 1.5], 2),
            ("gammaexp", [0.8, 1.5], 2), ("sqrexp_ard", [1.0, 1.25, 1.5, 1.1], 4), ("matern32_ard", [0.9, 1.2, 1.6], 3), ("matern52", [0.9], 3)]


@pytest.mark.parametrize("case", FD_CASES, ids=[c[0] for c in FD_CASES])
def test_longdouble_gradient_against_central_differences(case):
    name, theta, d = case
    n, m = 300, 40
    X, y, Z, _ = R.problem(60 + d, n, m, d, n_star=1)
    Z = np.asfortranarray(Z + 0.05 * np.random.default_rng(2).standard_normal(Z.shape))   # off X
    g = G.elbo_grad(name, theta, X, y, G.NOISE, Z, G.JITTER, LD)
    bound = lambda th, s2, Zc: G.elbo_ld(name, th, X, y, s2, Zc, G.JITTER)   # noqa: E731

    def diff(f, h):
        """central difference with one Richardson step: O(h^4)"""
        d1 = (f(h) - f(-h)) / (2 * LD(h))
        d2 = (f(2 * h) - f(-2 * h)) / (4 * LD(h))
        return (4 * d1 - d2) / 3

    errs = {}
    for p in range(len(theta)):
        def f(h, p=p):
            th = list(theta)
            th[p] += h
            return bound(th, G.NOISE, Z)
        errs["theta%d" % p] = rel(g["grad"][p], diff(f, 1e-4 * theta[p]))
    errs["noise"] = rel(g["grad"][-1], diff(lambda h: bound(theta, G.NOISE + h, Z), 1e-4 * G.NOISE))
    scale = float(np.abs(g["dZ"]).max())
    for c, j in ((0, 0), (1, 17), (d - 1, m - 1)):
        def f(h, c=c, j=j):
            Zc = Z.copy()
            Zc[c, j] += h
            return bound(theta, G.NOISE, Zc)
        errs["Z%d,%d" % (c, j)] = float(abs(g["dZ"][c, j] - diff(f, 1e-4)) / scale)
    print("central differences %s: %s" % (name, {k: "%.2e" % v for k, v in errs.items()}))
    assert max(errs.values()) <= FD_TOL, errs


@pytest.mark.parametrize("index,case", list(enumerate(R.TIGHT_CASES)), ids=[c[0] for c in R.TIGHT_CASES])
def test_inducing_points_equal_to_the_data_give_the_exact_gradient(index, case):
    name, theta = case
    X, y, _, _ = R.problem(len(R.CASES) + index, R.TIGHT_N, 1, R.TIGHT_D)
    lp, gl = A.logp_grad(name, theta, X, y, R.NOISE)
    r = G.elbo_grad(name, theta, X, y, R.NOISE, X, 0.0)
    errs = (max(rel(float(r["grad"][k]), gl[k]) for k in range(len(gl))), rel(float(r["elbo"]), lp), float(np.abs(r["dZ"]).max() / np.abs(r["grad"]).max()))
    print("Z = X %s (float64): grad %.2e elbo %.2e max |dZ| / max |grad| %.2e" % (name, *errs))
    assert errs[0] <= REF_TOL and errs[1] <= REF_TOL and errs[2] <= 1e-10, errs


def test_optimize_sparse_with_a_numpy_objective():
    name, theta0, d, n, m = "sqrexp", [1.4], 2, 120, 12
    X, y, Z0, _ = R.problem(70, n, m, d, n_star=1)
    calls = []

    def vg(theta, noise, Z):
        calls.append((tuple(theta), noise, Z.shape, Z.flags.f_contiguous))
        try:
            r = G.elbo_grad(name, list(theta), X, y, noise, Z, G.JITTER)
        except np.linalg.LinAlgError:                      # a long step of the line search: what the native call reports as info > 0
            raise nat.NotPositiveDefinite(1)
        return float(r["elbo"]), np.asarray(r["grad"], dtype=float), np.asarray(r["dZ"], dtype=float)

    start = vg(np.array(theta0), 0.3, Z0)[0]
    r = optimize_sparse(X, y, 0.3, name, Z0, theta0, value_and_grad=vg, maxit=8)
    assert set(r) == {"par", "noise", "Z", "value", "counts", "convergence", "func"}
    assert r["value"] > start and r["noise"] > 0 and len(r["par"]) == 1 and r["par"][0] > 0
    assert r["Z"].shape == (d, m) and r["Z"].flags.f_contiguous and not np.array_equal(r["Z"], Z0)
    assert all(c[2] == (d, m) and c[3] for c in calls)
    assert abs(vg(np.array(r["par"]), r["noise"], r["Z"])[0] - r["value"]) <= 1e-9 * abs(r["value"])   # the dict describes one point
    assert r["func"].native_params(d)[0] == r["par"][0]
    # the noise and the inducing points stay where they are when asked to; a failing evaluation is the sentinel, not an error
    fixed = optimize_sparse(X, y, 0.3, name, Z0, theta0, optimize_noise=False, optimize_Z=False, value_and_grad=vg, maxit=4)
    assert fixed["noise"] == 0.3 and np.array_equal(fixed["Z"], Z0) and fixed["value"] > start

    def failing(theta, noise, Z):
        if theta[0] > 1.45:
            raise nat.NotPositiveDefinite(3)
        return vg(theta, noise, Z)

    guarded = optimize_sparse(X, y, 0.3, name, Z0, theta0, value_and_grad=failing, maxit=4)
    assert guarded["par"][0] <= 1.45 and guarded["value"] >= start
    with pytest.raises(ValueError):
        optimize_sparse(X, y, 0.3, name, Z0, [-1.0], value_and_grad=vg)
    with pytest.raises(ValueError):
        optimize_sparse(X, y, 0.0, name, Z0, theta0, value_and_grad=vg)


def test_the_two_new_symbols_are_bound_and_exported():
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name, nargs in (("gprc_sgpr_elbo_grad", 15), ("gprc_dev_cross_grad", 14)):
        assert name in nat.PROTOTYPES and len(nat.PROTOTYPES[name][1]) == nargs, name
        assert hasattr(lib, name), name
    import gprc_amd
    from gprc_amd.fit import elbo_grad
    assert gprc_amd.elbo_grad is elbo_grad and gprc_amd.optimize_sparse is optimize_sparse
    assert {"elbo_grad", "optimize_sparse"} <= set(gprc_amd.__all__)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(nat.LIB_PATH))), "include", "gprc_native.h")) as f:
        header = f.read()
    assert "gprc_sgpr_elbo_grad(" in header and "gprc_dev_cross_grad(" in header
