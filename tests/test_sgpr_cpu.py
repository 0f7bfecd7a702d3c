"""The numpy reference of the sparse GPR (tests/sgpr_ref.py) judged without a GPU, on the very cases tests/test_gpu_sgpr.py runs, and the
six new symbols of the C ABI.

Bounds: the float64 reference against its longdouble twin 1e-11 (normwise on mean and var, relative on elbo and t) -- a tenth of the
1e-10 the GPU tests allow the library against the float64 reference; the collapsed bound never exceeds the exact log marginal
likelihood; at Z = X, jitter = 0 the bound IS the log marginal likelihood and the predictions are the exact GPR's (1e-11).
Case 3 (linear: K_uu has rank 3 plus jitter) compares elbo, mean and var only: its trace term cancels to about 0, so a relative bound on
it has no meaning.

The identity at Z = X is a statement about the FORMULAS, so it is evaluated in longdouble: in float64 the whitening with jitter 0 goes
through a K_uu of condition 3e14 (sqrexp {0.3}, 640 uniform points in [-2, 2]^2: 1.7e13 .. 6e14 over the draws), and the triangular solve
V = K_fu L_u^-T alone then carries 2.5e-11 into the mean whatever the formulas are; the float64 figure is printed beside it.  (On the
device the same identity is tested in float64 against the library's own exact GPR at 1e-10: tests/test_gpu_sgpr.py.)
The float64 reference takes its final sums (k - |v|^2 + |w|^2, the trace term) by math.fsum: k(x*,x*) - |v*|^2 cancels seven digits in
case 3, and with numpy's plain 200-term reductions on top the variance there stood at 1.34e-11 against longdouble.

Figures of this file (float64 against longdouble, worst of elbo / mean / var / t per case): 1.6e-13, 1.9e-14, 1.1e-13, 6.3e-12 (case 3:
the variance; what is left is the float64 solve with L_u, 5.8e-12 alone), 2.1e-12.  Z = X against the exact formulas in longdouble:
<= 7e-16 on elbo, mean and var, |t| <= 1e-15; in float64 (printed, not judged): sqrexp 1.9e-11 (the mean), matern52_ard 1.0e-13.
"""
import ctypes
import functools

import numpy as np
import pytest

import sgpr_ref as R
from conftest import nerr
from gprc_amd import _native as nat

REF_TOL = 1e-11
CASE_IDS = ["%d-%s" % (i, c[0]) for i, c in enumerate(R.CASES)]


@functools.lru_cache(maxsize=None)
def case_data(index):
    """the kernel blocks and the float64 results of case `index`, computed once and shared; never written to"""
    name, theta, n, m, d = R.CASES[index]
    X, y, Z, Xs = R.problem(index, n, m, d)
    Kb = R.blocks(name, theta, X, Z, Xs)
    return Kb, y, R.sgpr_from_blocks(Kb, y, R.NOISE, R.JITTER), R.exact_from_blocks(Kb, y, R.NOISE)


@pytest.mark.parametrize("index", range(len(R.CASES)), ids=CASE_IDS)
def test_float64_reference_against_longdouble(index):
    Kb, y, r64, _ = case_data(index)
    rld = R.sgpr_from_blocks(Kb, y, R.NOISE, R.JITTER, R.LD)
    errs = dict(elbo=float(abs(r64["elbo"] - rld["elbo"]) / abs(rld["elbo"])), mean=nerr(r64["mean"], rld["mean"].astype(float)),
                var=nerr(r64["var"], rld["var"].astype(float)))
    if index != 3:
        errs["t"] = float(abs(r64["t"] - rld["t"]) / abs(rld["t"]))
    print("sgpr reference case %d: %s" % (index, {k: "%.2e" % v for k, v in errs.items()}))
    assert max(errs.values()) <= REF_TOL, errs


@pytest.mark.parametrize("index", range(len(R.CASES)), ids=CASE_IDS)
def test_the_bound_is_below_the_log_marginal_likelihood(index):
    _, _, r64, ex = case_data(index)
    print("case %d: elbo %.6f logp %.6f gap %.3g, t %.3g" % (index, r64["elbo"], ex["logp"], ex["logp"] - r64["elbo"], r64["t"]))
    assert r64["elbo"] <= ex["logp"]


@pytest.mark.parametrize("index,case", list(enumerate(R.TIGHT_CASES)), ids=[c[0] for c in R.TIGHT_CASES])
def test_inducing_points_equal_to_the_data_reproduce_the_exact_model(index, case):
    name, theta = case
    X, y, _, Xs = R.problem(len(R.CASES) + index, R.TIGHT_N, 1, R.TIGHT_D)
    Kb = R.blocks(name, theta, X, X, Xs)

    def errors(dtype):
        s, ex = R.sgpr_from_blocks(Kb, y, R.NOISE, 0.0, dtype), R.exact_from_blocks(Kb, y, R.NOISE, dtype)
        rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())      # normwise, in dtype
        return (float(abs(s["elbo"] - ex["logp"]) / abs(ex["logp"])), rel(s["mean"], ex["mean"]), rel(s["var"], ex["var"])), float(s["t"])

    e64, t64 = errors(np.float64)
    eld, tld = errors(R.LD)
    print("Z = X %s: longdouble elbo %.2e mean %.2e var %.2e, t %.2e; float64 elbo %.2e mean %.2e var %.2e, t %.2e" % (name, *eld, tld, *e64, t64))
    assert max(eld) <= REF_TOL, eld
    assert abs(tld) <= 1e-9 and abs(t64) <= 1e-9


def test_the_six_new_symbols_are_bound_and_exported():
    names = ("gprc_sgpr_fit", "gprc_sgpr_elbo", "gprc_sgpr_predict", "gprc_sgpr_get_elbo", "gprc_dev_gram_rows", "gprc_dev_col_reduce")
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in names:
        assert name in nat.PROTOTYPES, name
        assert hasattr(lib, name), name
    from gprc_amd import SparseGPR, select_inducing
    from gprc_amd.fit import elbo
    assert callable(SparseGPR) and callable(select_inducing) and callable(elbo)
