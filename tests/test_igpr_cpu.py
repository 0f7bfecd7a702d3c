"""The iterative exact GPR without a GPU: the float64 numpy model of the device's algorithm (tests/igpr_ref.py) stays inside every bound
and condition tests/test_gpu_igpr.py holds the device to, on the very same inputs (the eight paths_ref.CASES, noise 0.1, tolerance 1e-10,
ranks 0 and 32), and the C ABI and the Python layer expose the feature.

Figures of the model on these inputs: every column converges; iterations 24 .. 158 at rank 0 and 1 .. 65 at rank 32; true residual
<= 1.0e-10; alpha within 4.6e-10 of the longdouble solution; variance error <= 0.0024 of its bound; rank 33 at r = 64 for case 2
(rationalquadratic, d = 1).
"""
import ctypes
import os
import re

import numpy as np
import pytest

import igpr_ref as I
import paths_ref as R
from conftest import ROOT
from gprc_amd import _native as nat

CASE_IDS = [R.case_id(i) for i in range(len(R.CASES))]
NEW_SYMBOLS = ("gprc_igpr_fit", "gprc_igpr_solve", "gprc_igpr_predict", "gprc_igpr_get_alpha", "gprc_igpr_stats", "gprc_dev_pivoted_cholesky")


@pytest.mark.parametrize("index", range(len(R.CASES)), ids=CASE_IDS)
def test_model_pivoted_cholesky_inside_its_bounds(index):
    ref = I.reference(index)
    L, piv, rank, _ = I.pivoted_cholesky(ref["K"], 32)
    fig = I.check_pivoted_cholesky(ref, 32, L, piv, rank)
    assert rank == 32
    print("pivoted Cholesky model %s: interpolation %.2e (bound %.2e), greedy %.2e (slack %.2e)" % (CASE_IDS[index], fig["interpolation"], fig["bound"],
                                                                                                   fig["greedy"], fig["slack"]))


def test_model_pivoted_cholesky_stops_early_on_a_one_dimensional_problem():
    ref = I.reference(2)                                            # rationalquadratic, d = 1
    L, piv, rank, _ = I.pivoted_cholesky(ref["K"], 64)
    fig = I.check_pivoted_cholesky(ref, 64, L, piv, rank)
    print("pivoted Cholesky model, case 2 at r = 64: rank %d, largest remaining diagonal %.2e" % (rank, fig["remaining"]))
    assert 1 <= rank < 64


@pytest.mark.parametrize("index", range(len(R.CASES)), ids=CASE_IDS)
def test_model_solve_predict_and_weights_inside_their_bounds(index):
    ref = I.reference(index)
    n, B = ref["n"], I.solve_rhs(ref)
    iters = {}
    for rank in I.RANKS:
        Q = I.model_preconditioner(ref, rank)
        X, it, rec, true, done = I.pcg(ref["K"], I.NOISE, B, I.CG_TOL, Q=Q)
        assert done and (rec <= I.CG_TOL).all()
        fig = I.check_solve(ref, B, X, true)
        iters[rank] = it
        print("solve model %s rank %d: iterations %d .. %d, true residual %.2e, error %.2e (%.4f of its bound), report ratio %.3f" % (
            CASE_IDS[index], rank, it.min(), it.max(), fig["true"], fig["err"], fig["err_bound_ratio"], fig["report_ratio"]))
    assert (iters[32] < iters[0]).all()                              # fewer iterations with the preconditioner, column by column
    # a zero column: zeros, no iteration, and its neighbours unchanged bit for bit
    Bz = B.copy()
    Bz[:, -1] = 0.0
    Xz, itz, _, _, _ = I.pcg(ref["K"], I.NOISE, Bz, I.CG_TOL, Q=Q)
    assert not Xz[:, -1].any() and itz[-1] == 0 and np.array_equal(Xz[:, :-1], X[:, :-1])
    # fit and predict from the rank-32 solve of y
    alpha = X[:, 0]
    ks = I.pairwise(ref["name"], ref["par"], ref["Xs"], ref["X"], np.float64)[0]
    W, _, _, _, done = I.pcg(ref["K"], I.NOISE, ks.T, I.CG_TOL, Q=Q)
    assert done
    fig = I.check_predict(ref, alpha, ks @ alpha, 1.0 - (ks.T * W).sum(0))
    print("predict model %s: mean %.4f of its bound, variance %.4f of its bound" % (CASE_IDS[index], fig["mean_ratio"], fig["var_ratio"]))
    # the sample paths' weights
    c = np.sqrt(2.0 / ref["W"].shape[0])
    rhs = ref["y"][:, None] - c * (R.features(ref["nu"], ref["phase"], ref["X"]) @ ref["W"]) - np.sqrt(I.NOISE) * ref["E"]
    Uw, _, _, _, done = I.pcg(ref["K"], I.NOISE, rhs, I.CG_TOL, Q=Q)
    assert done
    fig = I.check_weights(ref, Uw)
    print("weights model %s: %.2e (bound %.2e)" % (CASE_IDS[index], fig["err"], fig["bound"]))


@pytest.mark.parametrize("index", [2, 3, 5, 7], ids=[CASE_IDS[i] for i in (2, 3, 5, 7)])
def test_model_solves_a_block_of_seventy_columns(index):
    ref = I.reference(index)
    B = np.asfortranarray(ref["E"][:, :70])
    for rank in I.RANKS:
        X, it, rec, true, done = I.pcg(ref["K"], I.NOISE, B, I.CG_TOL, Q=I.model_preconditioner(ref, rank))
        assert done
        I.check_solve(ref, B, X, true)


def test_condition_numbers_are_the_documented_ones():
    kappas = [I.reference(i)["kappa"] for i in range(len(R.CASES))]
    print("kappa(K_y): " + ", ".join("%.0f" % k for k in kappas))
    assert round(min(kappas)) == 202 and round(max(kappas)) == 1570


def test_abi_declares_binds_and_exports_the_iterative_calls():
    header = open(os.path.join(ROOT, "include", "gprc_native.h")).read()
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"GPRC_API\s+int\s+" + name + r"\s*\(", header), name
        assert name in nat.PROTOTYPES, name
        assert hasattr(lib, name), name
    assert lib.gprc_prof_kinds() == 20


def test_python_layer_exports_iterative_gpr():
    import gprc_amd
    from gprc_amd import IterativeGPR
    assert "IterativeGPR" in gprc_amd.__all__
    for attr in ("predict", "solve", "alpha", "stats", "sample_paths", "thompson_batch", "close", "__enter__", "__exit__"):
        assert hasattr(IterativeGPR, attr), attr
