"""GPC evidence gradient, the parts that need no GPU: the numpy reference (tests/gpc_grad_ref.py, the book's per-parameter form)
pinned by central differences of its own log q; the rank-two form the device kernel contracts pinned against it; fit.optimize_gpc
driving vmmin on the numpy objective; the binding surface."""
import os
import re

import numpy as np
import pytest

import gpc_grad_ref as ref
from conftest import ROOT, nerr
from gprc_amd import _native as nat
from gprc_amd.fit import optimize_gpc
from gpu_calls import gpc_problem

CASES = [("sqrexp", [0.8], 300, 2), ("gammaexp", [0.9, 1.5], 300, 2), ("gammaexp", [1.2, 1.0], 600, 3),
         ("rationalquadratic", [1.1, 1.7], 600, 3), ("sqrexp_ard", [0.8, 1.9], 300, 2), ("sqrexp_ard", [0.8, 1.1, 1.9], 600, 3)]


@pytest.mark.parametrize("name,theta,n,d", CASES)
def test_reference_gradient_against_differences_of_its_own_log_q(name, theta, n, d):
    """normwise <= 1e-6 with a relative step of 1e-5 (measured: <= 9e-10).  With the book's printed sign of s2 the error is 3-15 %."""
    X, y = gpc_problem(n, d)
    theta = np.array(theta)
    _, grad, iters, _ = ref.logq_grad(name, theta, X, y)
    assert iters < 50
    fd = np.empty(theta.size)
    for k in range(theta.size):
        e = np.zeros(theta.size)
        e[k] = 1e-5 * theta[k]
        fd[k] = (ref.logq(name, theta + e, X, y) - ref.logq(name, theta - e, X, y)) / (2 * e[k])
    err = nerr(grad, fd)
    print(f"reference vs central differences {name} n={n} d={d}: {err:.3e}")
    assert err <= 1e-6


@pytest.mark.parametrize("name,theta,n,d", CASES)
def test_rank_two_form_equals_the_per_parameter_form(name, theta, n, d):
    """sum_ij M_ij dK_ij, M = 1/2 (a a^T - R) + 1/2 (u g^T + g u^T), is the algebra the device kernel implements: <= 1e-12
    against the book's s1 + s2.s3 (measured: <= 2e-15)."""
    X, y = gpc_problem(n, d)
    _, grad, _, _ = ref.logq_grad(name, theta, X, y)
    st = ref.laplace_state(name, theta, X, y, 1e-10)
    err = nerr(ref.gradient_rank_two(name, theta, X, st), grad)
    print(f"rank-two form vs per-parameter form {name} n={n} d={d}: {err:.3e}")
    assert err <= 1e-12


def test_optimize_gpc_on_the_numpy_objective():
    """n = 200, d = 3, y = sign(x_0 - 0.5 x_2 + 0.3 eps): coordinate 1 is irrelevant and gets the largest length scale."""
    rng = np.random.default_rng(21)
    n, d = 200, 3
    X = rng.uniform(-1, 1, (d, n))
    y = np.sign(X[0] - 0.5 * X[2] + 0.3 * rng.normal(size=n))
    y[y == 0] = 1.0

    def vg(theta):
        val, g, _, _ = ref.logq_grad("sqrexp_ard", theta, X, y)
        return val, g
    start_value = vg(np.ones(3))[0]
    r = optimize_gpc(X, y, "sqrexp_ard", start=np.ones(3), value_and_grad=vg)
    print("optimize_gpc on the numpy reference:", start_value, "->", r["value"], r["par"], r["counts"], r["convergence"])
    assert r["convergence"] == 0
    assert r["value"] >= start_value
    assert int(np.argmax(r["par"])) == 1
    assert set(r) == {"par", "value", "counts", "convergence", "func"}
    assert r["func"].gprc_kernel[0] == nat.SQREXP_ARD and np.array_equal(r["func"].gprc_kernel[1], r["par"])


def test_optimize_gpc_treats_a_failing_evaluation_as_the_sentinel():
    calls = []

    def vg(theta):   # a concave bowl in log theta with a forbidden region
        calls.append(theta.copy())
        z = np.log(theta)
        if z[0] > 1.0:
            raise ArithmeticError("the mode search did not converge")
        return -float(((z - 0.9) ** 2).sum()), -2.0 * (z - 0.9) / theta
    r = optimize_gpc(np.zeros((2, 4)), np.ones(4), "gammaexp", start=[1.0, 1.0], value_and_grad=vg)
    assert r["convergence"] == 0 and np.allclose(np.log(r["par"]), 0.9, atol=1e-4)
    assert any(np.log(t[0]) > 1.0 for t in calls)


def test_header_and_binding_carry_the_new_surface():
    header = open(os.path.join(ROOT, "include", "gprc_native.h")).read()
    assert re.search(r"GPRC_API\s+int\s+gprc_gpc_logq_grad\s*\(", header)
    assert "gprc_gpc_logq_grad" in nat.PROTOTYPES
    assert len(nat.PROTOTYPES["gprc_gpc_logq_grad"][1]) == 13
    assert hasattr(nat.lib(), "gprc_gpc_logq_grad")
    assert nat.lib().gprc_abi_version() == 1          # the change is additive
    assert len(nat.PROF_KINDS) == nat.lib().gprc_prof_kinds() and nat.PROF_KINDS[-1] == "gpc_grad_contract"
