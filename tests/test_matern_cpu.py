"""The Matern kernels, the parts that need no GPU and that only they need: the exact zero of a coinciding pair, the identities between
the isotropic and the ARD forms, the references of the two evidence gradients on the Matern formulas of tests/kernel_ref.py, and the host
surface (ids, header, generics, argument checks, classes, fit.optimize on a numpy objective).  The prediction gradients of the Matern
cases are judged by the checks of tests/case_checks.py (the gates of tests/test_pred_grad_cpu.py; cond(K_y) <= 1.1e4 is asserted for these cases).

Gates (the project's own, tests/test_ard_grad_cpu.py):
  * log marginal likelihood: closed-form gradient against central differences (relative step 1e-5) of the reference's own value:
    1e-6 (measured <= 6.3e-10 on the Matern cases, <= 3.1e-10 on the six older ones);
  * identities: an ARD kernel with equal length scales is the isotropic kernel (<= 1e-15), the diagonal is exactly 1.
That Matern 3/2 >= Matern 5/2 pointwise is not asserted: it is not a theorem."""
import os
import re

import numpy as np
import pytest

import ard_grad_ref as LP
from case_checks import check_float64_reference_against_longdouble, check_gradients_against_central_differences
import gpc_grad_ref
import kernel_ref as K
import pred_grad_ref as G
from conftest import ROOT, nerr
from gpu_calls import grad_problem
from gprc_amd import _native as nat
from gprc_amd import (CovFunc, GPR, GPR_matern32, GPR_matern32_ard, GPR_matern52, GPR_matern52_ard, cov_func, matern32, matern32_ard,
                      matern52, matern52_ard)
from gprc_amd.fit import cov_dict, grad_dict, optimize

LD = np.longdouble
GENERIC = {"matern32": matern32, "matern52": matern52, "matern32_ard": matern32_ard, "matern52_ard": matern52_ard}


# the prediction gradients: the checks of every kernel (tests/case_checks.py) on the Matern cases, under the names they have always had
MATERN_CASES = [c for c in K.CASES if c[0] in K.MATERN_NAMES]


@pytest.mark.parametrize("size", K.SIZES, ids=lambda s: "n%d-noise%g" % s)
@pytest.mark.parametrize("case", MATERN_CASES, ids=K.case_id)
def test_float64_reference_against_longdouble(case, size):
    check_float64_reference_against_longdouble(case, size)


@pytest.mark.parametrize("size", K.SIZES, ids=lambda s: "n%d-noise%g" % s)
@pytest.mark.parametrize("case", MATERN_CASES, ids=K.case_id)
def test_gradients_against_central_differences(case, size):
    check_gradients_against_central_differences(case, size)


def test_a_coinciding_pair_contributes_an_exact_zero():
    """x*_0 = x_5: g is finite and positive there and the difference is 0 -- no convention is needed"""
    for case in MATERN_CASES:
        X, _, Xs = G.make_case(case, 50)
        k, g, t = K.pairwise(case[0], case[1], Xs, X, np.float64)
        assert k[0, 5] == 1.0 and np.isfinite(g).all() and (g > 0).all()
        assert g[0, 5] == (3.0 if case[0].startswith("matern32") else 5.0 / 3.0)
        assert not (Xs[:, 0] - X[:, 5]).any()


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_logp_gradient_against_differences_of_the_reference_value(case):
    name, theta, d = case
    theta, noise = np.array(theta, dtype=float), 0.1
    X, y, _ = grad_problem(300, d)                                   # the inputs of tests/test_gpu_ard_grad.py
    val, grad = LP.logp_grad(name, theta, X, y, noise)
    assert val == LP.logp(name, theta, X, y, noise)
    assert abs(val - LP.gpr_fit(name, theta, X, y, noise)["logp"]) <= 1e-12 * abs(val)     # the other pair of triangular solves
    fd = np.empty(theta.size + 1)
    for k in range(theta.size):
        e = np.zeros(theta.size)
        e[k] = 1e-5 * theta[k]
        fd[k] = (LP.logp(name, theta + e, X, y, noise) - LP.logp(name, theta - e, X, y, noise)) / (2 * e[k])
    h = 1e-5 * noise
    fd[-1] = (LP.logp(name, theta, X, y, noise + h) - LP.logp(name, theta, X, y, noise - h)) / (2 * h)
    err = nerr(grad, fd)
    print(K.case_id(case), "closed form vs differences of logp: %.2e" % err)
    assert err <= 1e-6


def test_logq_gradient_against_differences_of_the_reference_value():
    """the Laplace evidence's reference likewise, once per order (n = 120: the mode search runs 2 theta.size + 1 times)"""
    rng = np.random.default_rng(17)
    X = rng.uniform(-1, 1, (3, 120))
    y = np.sign(X[0] - 0.5 * X[2] + 0.3 * rng.normal(size=120))
    y[y == 0] = 1.0
    for name, theta in (("matern32_ard", [0.8, 1.1, 1.9]), ("matern52", [0.9])):
        theta = np.array(theta)
        _, grad, iters, _ = gpc_grad_ref.logq_grad(name, theta, X, y, 1e-13)
        assert iters < 50
        fd = np.empty(theta.size)
        for k in range(theta.size):
            e = np.zeros(theta.size)
            e[k] = 1e-5 * theta[k]
            fd[k] = (gpc_grad_ref.logq_grad(name, theta + e, X, y, 1e-13)[0] - gpc_grad_ref.logq_grad(name, theta - e, X, y, 1e-13)[0]) / (2 * e[k])
        err = nerr(grad, fd)
        print(name, "logq closed form vs differences: %.2e" % err)
        assert err <= 1e-6


@pytest.mark.parametrize("order", ["matern32", "matern52"])
def test_identities(order):
    rng = np.random.default_rng(3)
    for d in (1, 3, 8):
        A, B = rng.uniform(-2, 2, (d, 40)), rng.uniform(-2, 2, (d, 30))
        for dtype in (np.float64, LD):
            iso = K.pairwise(order, [1.3], A, B, dtype)
            ard = K.pairwise(order + "_ard", [1.3] * d, A, B, dtype)
            for a, b in zip(iso, ard):
                assert np.abs(a - b).max() <= 1e-15
            assert np.all(np.diag(K.pairwise(order, [1.3], A, A, dtype)[0]) == 1.0)
        assert np.abs(K.kernel(order, [1.3], A) - K.kernel(order + "_ard", [1.3] * d, A)).max() <= 1e-15
        assert np.all(np.diag(K.kernel(order + "_ard", rng.uniform(0.5, 2, d), A)) == 1.0)
        # the two forms of the reference agree: kernel() (per-coordinate outer differences) and pairwise() (broadcast)
        assert np.abs(K.kernel(order, [0.7], A) - K.pairwise(order, [0.7], A, A, np.float64)[0]).max() <= 1e-15


# ---- host surface ---------------------------------------------------------------------------------------------------------------
def test_ids_in_the_binding_and_in_the_header():
    header = open(os.path.join(ROOT, "include", "gprc_native.h")).read()
    for name in K.NAMES:
        enum, kid = "RATQUAD" if name == "rationalquadratic" else name.upper(), K.KERNEL_ID[name]
        assert getattr(nat, enum) == kid
        m = re.search(r"GPRC_%s\s*=\s*(\d+)\b" % enum, header)
        assert m and int(m.group(1)) == kid
        assert grad_dict[name].kernel_id == kid
    assert set(grad_dict) == set(K.NAMES) and all(GENERIC[name] is grad_dict[name] for name in K.MATERN_NAMES)
    assert nat.SQREXP_ARD == 6 and re.search(r"GPRC_SQREXP_ARD\s*=\s*6\b", header)
    assert (nat.CONSTANT, nat.LINEAR, nat.POLYNOMIAL, nat.SQREXP, nat.GAMMAEXP, nat.RATQUAD) == (0, 1, 2, 3, 4, 5)
    assert nat.lib().gprc_abi_version() == 1          # the change is additive: no new symbol (tests/test_abi_cpu.py compares the list)


def test_fit_dictionaries():
    assert set(cov_dict) == {"sqrexp", "gammaexp", "constant", "linear", "polynomial", "rationalquadratic"}   # fit() selects among these
    assert set(K.MATERN_NAMES) <= set(grad_dict) and "sqrexp_ard" in grad_dict
    for name in K.MATERN_NAMES:
        assert grad_dict[name] is GENERIC[name] and grad_dict[name].arg_names == ("l",)


def test_cov_func_checks_the_length_scales():
    for gen in (matern32, matern52):
        k = cov_func(gen, l=0.7)
        assert isinstance(k, CovFunc) and k.gprc_kernel[0] == gen.kernel_id and np.array_equal(k.gprc_kernel[1], [0.7])
        assert np.array_equal(k.native_params(5), [0.7])
        assert cov_func(gen, 2.0).native_params(1)[0] == 2.0             # positional
        for bad in ([1.0, 2.0], [], 0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="l > 0"):
                cov_func(gen, l=bad)
        with pytest.raises(TypeError):
            cov_func(gen, sigma=1.0)
    for gen in (matern32_ard, matern52_ard):
        k = cov_func(gen, l=[0.5, 1.0, 2.0])
        assert k.gprc_kernel[0] == gen.kernel_id and np.array_equal(k.native_params(3), [0.5, 1.0, 2.0])
        with pytest.raises(ValueError, match="length\\(l\\) == nrow\\(X\\)"):
            k.native_params(2)                                          # wrong length for the inputs
        for bad in ([1.0, 0.0, 1.0], [1.0, -2.0, 1.0], [1.0, float("nan"), 1.0], [1.0, float("inf"), 1.0]):
            with pytest.raises(ValueError, match="l > 0"):
                cov_func(gen, l=bad)
        with pytest.raises(TypeError):
            cov_func(gen, sigma=[1.0])
    with pytest.raises(TypeError, match="matern52_ard"):
        cov_func(lambda x, y: 0.0)                                      # the list of kernels in the refusal names the new ones


def test_gpr_classes_exist_and_check_on_the_host():
    assert (GPR.matern32, GPR.matern52, GPR.matern32_ard, GPR.matern52_ard) == (GPR_matern32, GPR_matern52, GPR_matern32_ard, GPR_matern52_ard)
    for cls in (GPR_matern32, GPR_matern52, GPR_matern32_ard, GPR_matern52_ard):
        assert issubclass(cls, GPR)
    X, y = np.zeros((3, 5)), np.zeros(5)
    for cls in (GPR_matern32_ard, GPR_matern52_ard):                    # raised on the host, before any native call
        with pytest.raises(ValueError, match="length\\(l\\) == nrow\\(X\\)"):
            cls(X, y, 0.1, l=[1.0, 1.0])
    for cls in (GPR_matern32, GPR_matern52):
        with pytest.raises(ValueError, match="length\\(l\\) == 1"):
            cls(X, y, 0.1, l=[1.0, 1.0, 1.0])
        with pytest.raises(ValueError, match="l > 0"):
            cls(X, y, 0.1, l=-1.0)


@pytest.mark.parametrize("name", K.MATERN_NAMES)
def test_optimize_moves_uphill_on_the_numpy_objective(name):
    """fit.optimize drives vmmin on the reference's value and gradient: default start (1 or ones(d)), a higher value at the end,
    the result's `func` is the tagged kernel"""
    rng = np.random.default_rng(11)
    n, d = 200, 3
    X = rng.uniform(-2, 2, (d, n))
    y = np.sin(2 * X[0]) + 0.5 * X[1] ** 2 + 0.1 * rng.normal(size=n)   # the third coordinate is irrelevant

    def vg(theta, noise):       # the native objective's contract: a matrix that is not positive definite is NotPositiveDefinite
        try:
            return LP.logp_grad(name, theta, X, y, noise)
        except np.linalg.LinAlgError:
            raise nat.NotPositiveDefinite(1)
    npar = d if K.is_ard(name) else 1
    start_value = vg(np.ones(npar), 0.1)[0]
    r = optimize(X, y, 0.1, name, optimize_noise=True, maxit=200, value_and_grad=vg)
    print(name, "start", start_value, "end", r["value"], r["par"], r["noise"], r["counts"])
    assert r["convergence"] == 0 and len(r["par"]) == npar
    assert r["value"] > start_value
    assert r["func"].gprc_kernel[0] == K.KERNEL_ID[name] and np.array_equal(r["func"].gprc_kernel[1], r["par"])
    if K.is_ard(name):
        assert int(np.argmax(r["par"])) == 2
