"""Leave-one-out cross-validation on the CPU: the closed form of tests/loo_ref.py (the reference of tests/test_gpu_loo.py) against a
brute force that really leaves each point out, float64 against longdouble, the closed-form gradient against central differences of the
brute-force score, and the host surface (header, binding, fit.optimize's objective keyword).  No device is needed.

Measured on these cases: closed form against brute force <= 1.3e-14 normwise (gate 1e-11, the three orders of margin of the Matern CPU
tests); float64 against longdouble <= 1.1e-14 at cond(K_y) <= 533 (gate 1e-12); gradient against central differences <= 6.5e-11 (gate
1e-8, h = 1e-6, the project's other difference checks)."""
import os
import re

import numpy as np
import pytest

import loo_ref as R
from conftest import ROOT, nerr
from gprc_amd import _native as nat
from gprc_amd.fit import optimize

CASES = {"sqrexp": [0.9], "gammaexp": [1.1, 1.5], "rationalquadratic": [0.9, 1.7]}
NOISE = 0.1


def params(name, d):
    return CASES[name] if name in CASES else list(np.linspace(0.8, 1.6, d))   # matern52_ard


def make(n, d, seed=7):
    rng = np.random.default_rng(seed + 1000 * n + d)
    X = np.asfortranarray(rng.uniform(-2.0, 2.0, (d, n)))
    y = np.sin(X.sum(0)) + 0.3 * np.cos(2.0 * X[0]) + 0.1 * rng.standard_normal(n)
    return X, y


@pytest.mark.parametrize("n,d", [(37, 3), (150, 2)])
@pytest.mark.parametrize("name", ["sqrexp", "gammaexp", "rationalquadratic", "matern52_ard"])
def test_closed_form_is_the_brute_force(name, n, d):
    X, y = make(n, d)
    th = params(name, d)
    r = R.loo(name, th, X, y, NOISE)
    for what, got, ref in zip(("mean", "var", "ell"), (r["mean"], r["var"], r["ell"]), R.loo_brute(name, th, X, y, NOISE)):
        e = nerr(got, ref)
        print("%s n %d d %d %s %.2e" % (name, n, d, what, e))
        assert e <= 1e-11, (what, e)


@pytest.mark.parametrize("name", ["sqrexp", "gammaexp", "rationalquadratic", "matern52_ard"])
def test_float64_is_the_longdouble_form(name):
    n, d = 150, 2
    X, y = make(n, d)
    th = params(name, d)
    print("%s cond(K_y) %.3g" % (name, R.cond_Ky(name, th, X, NOISE)))
    a, b = R.loo(name, th, X, y, NOISE), R.loo(name, th, X, y, NOISE, R.LD)
    ga, gb = R.loo_grad(name, th, X, y, NOISE)[1], R.loo_grad(name, th, X, y, NOISE, R.LD)[1]
    for what, got, ref in (("mean", a["mean"], b["mean"]), ("var", a["var"], b["var"]), ("ell", a["ell"], b["ell"]), ("grad", ga, gb)):
        e = nerr(got, np.asarray(ref, dtype=float))
        print("%s %s %.2e" % (name, what, e))
        assert e <= 1e-12, (what, e)


@pytest.mark.parametrize("name", ["sqrexp", "gammaexp", "rationalquadratic", "matern52_ard"])
def test_gradient_is_the_difference_of_the_brute_force_score(name):
    n, d, h = 37, 3, 1e-6
    X, y = make(n, d)
    th = np.array(params(name, d), dtype=float)
    grad = R.loo_grad(name, th, X, y, NOISE)[1]
    fd = []
    for k in range(th.size + 1):
        def at(step):
            t, nz = th.copy(), NOISE
            if k < th.size:
                t[k] += step
            else:
                nz += step
            return R.loo_score_brute(name, t, X, y, nz)
        fd.append((at(h) - at(-h)) / (2.0 * h))
    e = nerr(grad, np.array(fd))
    print("%s gradient against central differences %.2e" % (name, e))
    assert e <= 1e-8, e


def test_header_and_binding_declare_both_entry_points():
    header = open(os.path.join(ROOT, "include", "gprc_native.h")).read()
    assert re.search(r"GPRC_API\s+int\s+gprc_gpr_loo\s*\(", header)
    assert re.search(r"GPRC_API\s+int\s+gprc_gpr_loo_grad\s*\(", header)
    assert "gprc_gpr_loo" in nat.PROTOTYPES and "gprc_gpr_loo_grad" in nat.PROTOTYPES
    assert hasattr(nat.lib(), "gprc_gpr_loo") and hasattr(nat.lib(), "gprc_gpr_loo_grad")
    assert len(nat.PROTOTYPES["gprc_gpr_loo"][1]) == 5
    assert len(nat.PROTOTYPES["gprc_gpr_loo_grad"][1]) == len(nat.PROTOTYPES["gprc_gpr_logp_grad"][1]) == 11


def test_optimize_with_the_loo_objective_on_the_reference():
    """the vmmin-over-log driver with objective="loo" and the numpy reference as the hook: the LOO score ends higher than it began"""
    X, y = make(60, 2)
    calls = []

    def vg(theta, noise):
        val, g = R.loo_grad("matern52_ard", theta, X, y, noise)
        calls.append(float(val))
        return float(val), np.asarray(g, dtype=float)

    r = optimize(X, y, NOISE, "matern52_ard", objective="loo", value_and_grad=vg, maxit=15)
    start = float(R.loo_grad("matern52_ard", [1.0, 1.0], X, y, NOISE)[0])
    print("LOO %.6f -> %.6f in %d evaluations" % (start, r["value"], len(calls)))
    assert calls[0] == start and r["value"] > start
    assert r["value"] == pytest.approx(float(R.loo_grad("matern52_ard", r["par"], X, y, r["noise"])[0]), rel=1e-12)


def test_optimize_refuses_an_unknown_objective():
    X, y = make(10, 2)
    with pytest.raises(ValueError):
        optimize(X, y, NOISE, "sqrexp", objective="bogus", value_and_grad=lambda t, nz: (0.0, np.zeros(2)))
    with pytest.raises(ValueError):
        optimize(X, y, NOISE, "sqrexp", objective="bogus")
