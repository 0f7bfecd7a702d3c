"""Batched prediction gradients and batched LOO on the host: the numpy models of the two kernels' algorithm
(batch_predict_grad_ref.numpy_model, numpy_loo: W = L^-1 formed explicitly, u = W^T (W k*), p_i = sum_k W_ki^2) against the
extended-precision references, on the inputs the GPU tests use, inside the bound they use; BatchGPR.predict_grad and BatchGPR.loo on a
hook that replaces the native calls; and the two symbols in the header and the bindings.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import batch_predict_grad_ref as Q
import batch_ref as R
import loo_ref
from conftest import TOL
from gprc_amd import BatchGPR
from gprc_amd import _native as nat
from test_batch_predict_cpu import _StubCtx, _StubLib

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "include", "gprc_native.h")


# ---- 1. the numpy models stay inside the bound the GPU tests use ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GRID_CASES)
def test_models_of_the_gradient_and_loo_kernels_are_within_tol_of_extended_precision(case):
    """The whole grid of batch_ref (6 sizes x 6 models a case), all <= conftest.TOL = 1e-10: dmean and dvar normwise per model over
    the d x 37 block; the LOO mean relative to max |y|, the LOO variance per component relative to itself, logdens normwise, the score
    relative.  Measured on the CPU over the grid: the printed worst values are ~1e-13, three orders inside the bound."""
    worst = dict(dmean=0.0, dvar=0.0, mean=0.0, var=0.0, logdens=0.0, score=0.0)
    smallest = np.inf
    for n in R.GRID_SIZES:
        name, X, y, thetas, noises = R.models(case, n)
        Xs = Q.grid_points(case, n)
        assert Xs.shape == (X.shape[0], Q.NS)
        for th, nz in zip(thetas, noises):
            _, _, want_dm, want_dv = Q.G.predict_grad(name, th, X, y, nz, Xs, Q.LD)
            _, _, dm, dv = Q.numpy_model(name, th, X, y, nz, Xs)
            worst["dmean"] = max(worst["dmean"], Q.G.nerr(np.asarray(dm, dtype=Q.LD), want_dm))
            worst["dvar"] = max(worst["dvar"], Q.G.nerr(np.asarray(dv, dtype=Q.LD), want_dv))
            smallest = min(smallest, float(np.abs(want_dm).max()), float(np.abs(want_dv).max()))
            got = {k: np.asarray(v, dtype=Q.LD) for k, v in Q.numpy_loo(name, th, X, y, nz).items()}
            for k, e in Q.loo_errors(got, loo_ref.loo(name, th, X, y, nz, Q.LD), y).items():
                worst[k] = max(worst[k], e)
    print(case, {k: "%.2e" % v for k, v in worst.items()}, "smallest largest |gradient| %.2e" % smallest)
    assert smallest > 1e-6                                   # no model's gradients are all zero: the normwise error has a scale
    assert all(v <= TOL for v in worst.values()), worst


def test_the_float64_references_are_fit_references_for_the_gpu_tests():
    """what the GPU tests compare with (pred_grad_ref and loo_ref in float64) against extended precision, on one entry of every size"""
    for case, n in (("sqrexp", 1), ("matern52_ard8", 17), ("ard33", 128), ("gammaexp1", 127)):
        name, X, y, thetas, noises = R.models(case, n)
        Xs = Q.grid_points(case, n)
        for ref, lref, th, nz in zip(Q.grad_references(case, n), Q.loo_references(case, n), thetas, noises):
            _, _, want_dm, want_dv = Q.G.predict_grad(name, th, X, y, nz, Xs, Q.LD)
            assert Q.G.nerr(np.asarray(ref[2], dtype=Q.LD), want_dm) <= 0.1 * TOL
            assert Q.G.nerr(np.asarray(ref[3], dtype=Q.LD), want_dv) <= 0.1 * TOL
            got = {k: np.asarray(lref[k], dtype=Q.LD) for k in ("mean", "var", "ell", "loo")}
            assert max(Q.loo_errors(got, loo_ref.loo(name, th, X, y, nz, Q.LD), y).values()) <= 0.1 * TOL


def test_the_test_points_at_one_training_point():
    X = R.models("ard3", 1)[1]
    Xs = Q.grid_points("ard3", 1)
    assert Xs.shape == (3, 37) and np.array_equal(Xs[:, 0], X[:, 0]) and (np.abs(Xs - X) <= 2).all() and (Xs[:, 1:] != X).all()
    assert Q.grid_points("ard3", 17) is Q.P.grid_points("ard3", 17)


# ---- 2. BatchGPR.predict_grad and BatchGPR.loo on a stand-in library ----------------------------------------------------------------------
class _GradStub(_StubLib):
    def __init__(self):
        super().__init__()
        self.grads, self.loos = [], []

    def gprc_gpr_batch_predict_grad(self, model, Xs, ns_max, xs_stride, ns_each, mean, var, ld_out, dmean, dvar, ld_grad):
        B, d = self.B, self.d
        counts = None if not ns_each else self._arr(ns_each, B, C.c_int64)
        self.grads.append(dict(model=model.value, Xs=self._arr(Xs, (B - 1) * xs_stride + d * ns_max), ns_max=ns_max, xs_stride=xs_stride, ns_each=counts,
                               var=bool(var), dvar=bool(dvar), ld_out=ld_out, ld_grad=ld_grad))
        for b in range(B):                       # what the library does: a model's count of entries, nothing behind it
            nb = ns_max if counts is None else int(counts[b])
            np.ctypeslib.as_array((C.c_double * nb).from_address(mean + 8 * b * ld_out))[:] = 100 * b + np.arange(nb)
            g = 1000 * b + 10 * np.repeat(np.arange(nb), d) + np.tile(np.arange(d), nb)          # [j][c]: 1000 b + 10 j + c
            np.ctypeslib.as_array((C.c_double * (d * nb)).from_address(dmean + 8 * b * ld_grad))[:] = g
            if var:
                np.ctypeslib.as_array((C.c_double * nb).from_address(var + 8 * b * ld_out))[:] = -(100 * b + np.arange(nb))
            if dvar:
                np.ctypeslib.as_array((C.c_double * (d * nb)).from_address(dvar + 8 * b * ld_grad))[:] = -g
        return 0

    def gprc_gpr_batch_loo(self, model, mean, var, dens, ld_out, score):
        self.loos.append(dict(model=model.value, arrays=(bool(mean), bool(var), bool(dens)), ld_out=ld_out, score=bool(score)))
        for b, nb in enumerate(self.sizes):
            for k, p in enumerate((mean, var, dens)):
                if p:
                    np.ctypeslib.as_array((C.c_double * nb).from_address(p + 8 * b * ld_out))[:] = 10 * k + b + 0.01 * np.arange(nb)
            if score:
                np.ctypeslib.as_array((C.c_double * 1).from_address(score + 8 * b))[:] = -b
        return 0


def test_batchgpr_predict_grad_and_loo_pad_orient_and_cut(monkeypatch):
    stub = _GradStub()
    monkeypatch.setattr(nat, "lib", lambda: stub)
    rng = np.random.default_rng(6)
    d, sizes, stars = 3, [5, 1, 9, 4], [2, 7, 1, 3]
    stub.sizes = sizes
    g = BatchGPR([rng.normal(size=(d, n)) for n in sizes], [rng.normal(size=n) for n in sizes], 0.1, "sqrexp_ard", rng.uniform(0.5, 2.0, (4, d)),
                 ctx=_StubCtx())
    # unequal test sets: one stride per model, the counts; four lists back, the gradients d x n*_b
    Ts = [rng.normal(size=(d, m)) for m in stars]
    mean, var, dmean, dvar = g.predict_grad(Ts)
    q = stub.grads[0]
    assert (q["model"], q["ns_max"], q["xs_stride"], q["ld_out"], q["ld_grad"], q["var"], q["dvar"]) == (4242, 7, d * 7, 7, d * 7, True, True)
    assert np.array_equal(q["ns_each"], stars)
    for b, m in enumerate(stars):
        assert np.array_equal(q["Xs"][b * d * 7:b * d * 7 + d * m].reshape(m, d).T, Ts[b])
        assert np.array_equal(mean[b], 100 * b + np.arange(m)) and np.array_equal(var[b], -(100 * b + np.arange(m)))
        want = 1000 * b + 10 * np.arange(m)[None, :] + np.arange(d)[:, None]              # [c, j]
        assert dmean[b].shape == (d, m) and np.array_equal(dmean[b], want) and np.array_equal(dvar[b], -want)
    # one shared set: no stride, no counts, arrays back; var=False passes NULL for var and dvar
    mean, var, dmean, dvar = g.predict_grad(Ts[1], var=False)
    q = stub.grads[1]
    assert (q["ns_max"], q["xs_stride"], q["ld_out"], q["ld_grad"], q["var"], q["dvar"]) == (7, 0, 7, d * 7, False, False) and q["ns_each"] is None
    assert np.array_equal(q["Xs"].reshape(7, d).T, Ts[1]) and var is None and dvar is None
    assert mean.shape == (4, 7) and dmean.shape == (4, d, 7)
    assert np.array_equal(dmean[2], 2000 + 10 * np.arange(7)[None, :] + np.arange(d)[:, None])
    mean, var, dmean, dvar = g.predict_grad(Ts[1])
    assert var.shape == (4, 7) and dvar.shape == (4, d, 7) and np.array_equal(dvar, -dmean)
    with pytest.raises(ValueError):
        g.predict_grad(Ts[:3])                                             # one set per model
    with pytest.raises(ValueError):
        g.predict_grad([rng.normal(size=(d + 1, 2))] * 4)                  # the models' d
    # LOO: B x n_max, NaN behind a model's points; the score is a call of its own with the arrays NULL
    lm, lv, ld = g.loo()
    assert stub.loos[0] == dict(model=4242, arrays=(True, True, True), ld_out=9, score=False)
    for k, a in enumerate((lm, lv, ld)):
        assert a.shape == (4, 9)
        for b, nb in enumerate(sizes):
            assert np.array_equal(a[b, :nb], 10 * k + b + 0.01 * np.arange(nb)) and np.isnan(a[b, nb:]).all()
    assert np.array_equal(g.loo_score, -np.arange(4.0))
    assert stub.loos[1] == dict(model=4242, arrays=(False, False, False), ld_out=9, score=True)
    g.close()
    with pytest.raises(nat.GprcError):
        g.predict_grad(Ts)
    with pytest.raises(nat.GprcError):
        g.loo()


# ---- 3. the two symbols: declared in the header, bound by the package ----------------------------------------------------------------------
@pytest.mark.parametrize("symbol,nargs", [("gprc_gpr_batch_predict_grad", 11), ("gprc_gpr_batch_loo", 6)])
def test_the_header_declares_and_the_package_binds_the_new_calls(symbol, nargs):
    text = open(HEADER).read()
    m = re.search(r"GPRC_API\s+int\s+%s\s*\(([^;]*)\)\s*;" % symbol, text)
    assert m, symbol + " is not declared in include/gprc_native.h"
    assert len(m.group(1).split(",")) == nargs
    assert symbol in nat.PROTOTYPES
    restype, argtypes = nat.PROTOTYPES[symbol]
    assert restype is C.c_int and len(argtypes) == nargs
