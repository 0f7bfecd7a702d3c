"""Exact gradient and ARD, the parts that need no GPU: the header / binding surface, the argument checks of
cov_func(sqrexp_ard, ...), the numpy closed form of the gradient (tests/ard_grad_ref.py) pinned by the CPU oracle, and
fit.optimize driving vmmin on that numpy objective against scipy's L-BFGS-B."""
import os
import re

import numpy as np
import pytest

import ard_grad_ref as ref
from conftest import ROOT, nerr
from gprc_amd import _native as nat
from gprc_amd import CovFunc, GPR_sqrexp_ard, cov_func, sqrexp_ard
from gprc_amd.fit import optimize
from oracle import oracle as orc


def test_header_and_binding_carry_the_new_surface():
    header = open(os.path.join(ROOT, "include", "gprc_native.h")).read()
    assert re.search(r"GPRC_SQREXP_ARD\s*=\s*6\b", header)
    assert nat.SQREXP_ARD == 6
    assert re.search(r"GPRC_API\s+int\s+gprc_gpr_logp_grad\s*\(", header)
    assert "gprc_gpr_logp_grad" in nat.PROTOTYPES
    assert hasattr(nat.lib(), "gprc_gpr_logp_grad")
    assert nat.lib().gprc_abi_version() == 1          # the change is additive
    assert len(nat.PROTOTYPES["gprc_gpr_logp_grad"][1]) == 11
    assert len(nat.PROF_KINDS) == nat.lib().gprc_prof_kinds() and {"inverse_gemm", "grad_contract"} <= set(nat.PROF_KINDS)


def test_cov_func_sqrexp_ard_checks_its_length_scales():
    k = cov_func(sqrexp_ard, l=[0.5, 1.0, 2.0])
    assert isinstance(k, CovFunc) and callable(k)
    assert k.gprc_kernel[0] == nat.SQREXP_ARD and np.array_equal(k.gprc_kernel[1], [0.5, 1.0, 2.0])
    assert np.array_equal(k.native_params(3), [0.5, 1.0, 2.0])
    with pytest.raises(ValueError, match="length\\(l\\) == nrow\\(X\\)"):
        k.native_params(2)                                          # wrong length for the inputs
    for bad in ([1.0, 0.0, 1.0], [1.0, -2.0, 1.0], [1.0, float("nan"), 1.0], [1.0, float("inf"), 1.0]):
        with pytest.raises(ValueError, match="l > 0"):
            cov_func(sqrexp_ard, l=bad)
    with pytest.raises(TypeError):
        cov_func(sqrexp_ard, sigma=[1.0])                           # argument matching as for the other generics
    assert cov_func(sqrexp_ard, [3.0]).native_params(1)[0] == 3.0   # positional, scalar-length vector
    with pytest.raises(ValueError, match="length\\(l\\) == nrow\\(X\\)"):
        GPR_sqrexp_ard(np.zeros((3, 5)), np.zeros(5), 0.1, l=[1.0, 1.0])   # raised on the host, before any native call


def ard_problem():
    rng = np.random.default_rng(11)
    n, d = 60, 3
    X = rng.uniform(-2, 2, (d, n))
    y = np.sin(2 * X[0]) + 0.5 * X[1] ** 2 + 0.1 * rng.normal(size=n)   # the third coordinate is irrelevant
    return X, y


def test_numpy_closed_form_against_differences_of_the_oracle():
    """The tests' reference is itself pinned: its gradient against central differences (h = 1e-5 theta) of the oracle's logp on
    the scaled inputs, 1e-6 normwise; its value against the oracle's."""
    X, y = ard_problem()
    for ell, noise in ((np.array([1.0, 1.0, 1.0]), 0.1), (np.array([0.8, 1.7, 3.0]), 0.05)):
        def logp(ell_, noise_):
            f = orc.gpr_fit(orc.SQREXP, [1.0], X / ell_[:, None], y, noise_)
            assert f["attempts"] == 1
            return f["logp"]
        val, grad = ref.logp_grad("sqrexp_ard", ell, X, y, noise)
        assert abs(val - logp(ell, noise)) <= 1e-12 * abs(val)
        fd = np.empty(4)
        for k in range(3):
            h = 1e-5 * ell[k]
            e = np.zeros(3)
            e[k] = h
            fd[k] = (logp(ell + e, noise) - logp(ell - e, noise)) / (2 * h)
        h = 1e-5 * noise
        fd[3] = (logp(ell, noise + h) - logp(ell, noise - h)) / (2 * h)
        err = nerr(grad, fd)
        print("closed form vs oracle differences:", err)
        assert err <= 1e-6


def test_closed_forms_of_the_isotropic_kernels_against_differences_of_the_oracle():
    X, y = ard_problem()
    for name, theta in (("sqrexp", [1.3]), ("gammaexp", [0.9, 1.5]), ("gammaexp", [1.2, 1.0]), ("rationalquadratic", [1.1, 1.7])):
        theta, noise = np.array(theta), 0.1
        logp = lambda th, nz: orc.gpr_fit(orc.KERNEL_IDS[name], list(th), X, y, nz)["logp"]   # noqa: E731
        val, grad = ref.logp_grad(name, theta, X, y, noise)
        assert abs(val - logp(theta, noise)) <= 1e-12 * abs(val)
        fd = np.empty(theta.size + 1)
        for k in range(theta.size):
            e = np.zeros(theta.size)
            e[k] = 1e-5 * theta[k]
            fd[k] = (logp(theta + e, noise) - logp(theta - e, noise)) / (2 * e[k])
        h = 1e-5 * noise
        fd[-1] = (logp(theta, noise + h) - logp(theta, noise - h)) / (2 * h)
        assert nerr(grad, fd) <= 1e-6, name


def test_optimize_reaches_the_optimum_of_l_bfgs_b_on_the_numpy_objective():
    """fit.optimize (vmmin over log theta, log noise) on the numpy closed form against scipy's L-BFGS-B on the same objective:
    the same maximum to 1e-3 max(1, |value|) -- the objective is flat along the irrelevant length scale, so the two stop at
    different points of one plateau -- and the irrelevant coordinate gets the largest length scale."""
    from scipy.optimize import minimize
    X, y = ard_problem()
    vg = lambda theta, noise: ref.logp_grad("sqrexp_ard", theta, X, y, noise)   # noqa: E731
    r = optimize(X, y, 0.1, "sqrexp_ard", start=np.ones(3), optimize_noise=True, maxit=200, value_and_grad=vg)
    assert r["convergence"] == 0
    assert len(r["par"]) == 3 and int(np.argmax(r["par"])) == 2
    assert r["func"].gprc_kernel[0] == nat.SQREXP_ARD and np.array_equal(r["func"].gprc_kernel[1], r["par"])
    assert 0 < r["noise"] < 0.1

    def neg(z):
        t = np.exp(z)
        val, g = vg(t[:3], t[3])
        return -val, -g * t
    s = minimize(neg, np.log([1.0, 1.0, 1.0, 0.1]), jac=True, method="L-BFGS-B")
    print("vmmin", r["value"], r["par"], r["noise"], r["counts"], "L-BFGS-B", -s.fun)
    assert abs(r["value"] - (-s.fun)) <= 1e-3 * max(1.0, abs(s.fun))
    assert r["value"] > ref.logp_grad("sqrexp_ard", np.ones(3), X, y, 0.1)[0]
    # the noise stays fixed when asked, and for noise = 0
    r2 = optimize(X, y, 0.1, "sqrexp_ard", optimize_noise=False, maxit=200, value_and_grad=vg)
    assert r2["noise"] == 0.1 and r2["value"] <= r["value"] + 1e-9


def test_optimize_treats_a_failing_evaluation_as_the_sentinel():
    """A NotPositiveDefinite (or overflow) inside the line search is a rejected step, not an error."""
    calls = []

    def vg(theta, noise):   # a concave bowl in log theta with a forbidden region
        calls.append(theta.copy())
        z = np.log(theta)
        if z[0] > 1.0:
            raise nat.NotPositiveDefinite(1)
        return -float(((z - 0.9) ** 2).sum()), np.append(-2.0 * (z - 0.9) / theta, 0.0)
    r = optimize(np.zeros((2, 4)), np.zeros(4), 0.0, "gammaexp", start=[1.0, 1.0], value_and_grad=vg)
    assert r["convergence"] == 0 and np.allclose(np.log(r["par"]), 0.9, atol=1e-4) and r["noise"] == 0.0
    assert any(np.log(t[0]) > 1.0 for t in calls)
