"""The reference of the prediction-gradient tests judges itself (no GPU): tests/pred_grad_ref.py on the kernels of tests/kernel_ref.py, in
float64 against the same formulas in numpy.longdouble and against central differences of the longdouble mean and variance; and the
identity the backward solve rests on, V L^-1 = ((V J) M^-T) J with M = J L^T J lower triangular, on the packed layout.

Gates: float64 against longdouble 1e-11 normwise on each of the four outputs (measured <= 1.6e-13 on these cases), central differences
(h = 1e-6) 1e-8 (measured <= 3.4e-11 for the smooth kernels and the Matern ones, 5.4e-9 for gammaexp with gamma = 1, whose third
derivative grows towards every training point).  gammaexp with gamma <= 1 is not differentiable at a training point: the test point that
equals one is left out of the difference check there (the analytic value follows the h = 0 convention); no Matern derivative holds a
1 / r, so theirs stays in.  Every Matern case has cond(K_y) <= 1.1e4 (asserted): 1e-11 in float64 is not a statement about an
ill-conditioned solve.  (The older cases reach 1.2e4 -- rationalquadratic at n = 600, noise 0.01 -- and carry no such assertion.)"""
import os
import re

import numpy as np
import pytest

from case_checks import check_float64_reference_against_longdouble, check_gradients_against_central_differences
from conftest import ROOT
import kernel_ref as K
import packed_ref as R
import pred_grad_ref as G

LD = np.longdouble
# every case but the Matern ones, which keep the names they have always had in tests/test_matern_cpu.py
OTHER_CASES = [c for c in K.CASES if c[0] not in K.MATERN_NAMES]


@pytest.mark.parametrize("size", K.SIZES, ids=lambda s: "n%d-noise%g" % s)
@pytest.mark.parametrize("case", OTHER_CASES, ids=K.case_id)
def test_float64_reference_against_longdouble(case, size):
    check_float64_reference_against_longdouble(case, size)


@pytest.mark.parametrize("size", K.SIZES, ids=lambda s: "n%d-noise%g" % s)
@pytest.mark.parametrize("case", OTHER_CASES, ids=K.case_id)
def test_gradients_against_central_differences(case, size):
    check_gradients_against_central_differences(case, size)


def test_gammaexp_convention_at_a_training_point():
    """h = 0 at r = 0: the pair (x*_0, x_5) contributes nothing, for gamma > 1 (the limit) and gamma <= 1 (the convention)"""
    for case in K.CASES:
        if case[0] != "gammaexp":
            continue
        X, _, Xs = G.make_case(case, 50)
        _, h, _ = K.pairwise(case[0], case[1], Xs, X, np.float64)
        assert h[0, 5] == 0.0 and np.isfinite(h).all() and (np.delete(h[0], 5) > 0).all()


@pytest.mark.parametrize("n", [512, 700, 1100])
def test_reversal_identity_on_the_packed_layout(n):
    rng = np.random.default_rng(n)
    L = np.tril(rng.normal(size=(n, n))) / np.sqrt(n)
    L[np.diag_indices(n)] = rng.uniform(0.5, 1.5, n)
    g = R.geometry(n)
    n_pad = g.n_pad
    packed = R.pack(L + np.triu(rng.normal(size=(n, n)), 1), n)     # stale values above the diagonal of the diagonal blocks
    Lp = R.unpack_lower(packed, n_pad)
    assert np.array_equal(Lp, R.pad_identity(L, n_pad))
    winv = rng.normal(size=g.winv_size)
    packed_rev, winv_rev = G.reverse_packed(packed, winv, n_pad)
    M = Lp[::-1, ::-1].T                                            # J L^T J
    assert not np.triu(M, 1).any()                                  # lower triangular
    assert np.array_equal(R.unpack_lower(packed_rev, n_pad), M)
    for p in range(g.P):                                            # the diagonal blocks carry zeros above the diagonal
        assert not np.triu(R.panel_view(packed_rev, g, p)[:g.NB], 1).any()
    pad = n_pad - n                                                 # the identity padding now leads
    assert np.array_equal(M[:pad, :pad], np.eye(pad)) and not M[pad:, :pad].any()
    B = n_pad // 128
    for b in (0, B - 1):
        assert np.array_equal(R.winv_block(winv_rev, b), R.winv_block(winv, B - 1 - b)[::-1, ::-1].T)
    # V L^-1 = ((V J) M^-T) J in longdouble: rows of V as right-hand sides, X L = V  <=>  L^T X^T = V^T
    V = rng.normal(size=(3, n_pad))
    Ll, Ml = np.asarray(Lp, dtype=LD), np.asarray(M, dtype=LD)
    direct = G.solve_lower(Ll, np.asarray(V.T, dtype=LD), transpose=True).T
    Y = G.solve_lower(Ml, np.asarray(V[:, ::-1].T, dtype=LD)).T   # Y M^T = V J
    assert G.nerr(Y[:, ::-1], direct) <= 1e-13


def test_header_binding_and_profiler_carry_the_new_surface():
    from gprc_amd import _native as nat
    header = open(os.path.join(ROOT, "include", "gprc_native.h")).read()
    assert re.search(r"GPRC_API\s+int\s+gprc_gpr_predict_grad\s*\(", header) and re.search(r"GPRC_API\s+int\s+gprc_dev_reverse_factor\s*\(", header)
    assert len(nat.PROTOTYPES["gprc_gpr_predict_grad"][1]) == 7 and len(nat.PROTOTYPES["gprc_dev_reverse_factor"][1]) == 6
    assert hasattr(nat.lib(), "gprc_gpr_predict_grad") and hasattr(nat.lib(), "gprc_dev_reverse_factor")
    assert nat.lib().gprc_abi_version() == 1          # the change is additive
    assert len(nat.PROF_KINDS) == nat.lib().gprc_prof_kinds() == 20 and sorted(nat.PROF_KIND_ID.values()) == list(range(20))
    assert sorted(nat.PROF_KIND_ID) == sorted(nat.PROF_KINDS)
    assert (nat.PROF_KIND_ID["gpc_grad_contract"], nat.PROF_KIND_ID["reverse_factor"], nat.PROF_KIND_ID["pred_grad_contract"]) == (17, 18, 19)
    assert [nat.PROF_KIND_ID[k] for k in nat.PROF_KINDS[:17]] == list(range(17))          # the earlier kinds keep their numbers
