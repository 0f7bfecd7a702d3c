"""Batched predict on the host: the numpy model of the kernel's algorithm (batch_predict_ref.numpy_model: W = L^-1 formed explicitly,
V = W K* as a product) against an extended-precision reference, on the inputs the GPU tests use, inside the bound they use; and
BatchGPR's padding of unequal data sets and unequal test sets, on a hook that replaces the native calls.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import batch_predict_ref as P
import batch_ref as R
from conftest import TOL
from gprc_amd import BatchGPR
from gprc_amd import _native as nat
from gprc_amd.fit import grad_dict


# ---- 1. the numpy model of the batched predict stays inside the bound the GPU tests use -------------------------------------------------
@pytest.mark.parametrize("case", R.GRID_CASES)
def test_model_of_the_batched_predict_is_within_tol_of_extended_precision(case):
    """Mean normwise, variance per component RELATIVE TO THE VARIANCE ITSELF, both <= conftest.TOL = 1e-10.  Measured on the CPU over
    the whole grid below (37 test points an entry): the printed worst values are ~1e-13 for the mean and ~1e-12 for the variance, which
    leaves the device two orders of magnitude."""
    worst = dict(mean=0.0, var=0.0)
    smallest = np.inf
    for n in (1, 17, 128):
        name, X, y, thetas, noises = R.models(case, n)
        Xs = P.grid_points(case, n)
        assert Xs.shape == (X.shape[0], P.NS)
        for th, nz in zip(thetas, noises):
            want_m, want_v = P.closed_form(name, th, X, y, nz, Xs, P.LD)
            m, v = P.numpy_model(name, th, X, y, nz, Xs)
            worst["mean"] = max(worst["mean"], P.G.nerr(np.asarray(m, dtype=P.LD), want_m))
            worst["var"] = max(worst["var"], P.var_err(np.asarray(v, dtype=P.LD), want_v))
            smallest = min(smallest, float(want_v.min()))
    print(case, {k: "%.2e" % v for k, v in worst.items()}, "smallest variance %.2e" % smallest)
    assert smallest > 0
    assert all(v <= TOL for v in worst.values()), worst


def test_the_float64_closed_form_is_a_fit_reference_for_the_gpu_tests():
    """the reference the GPU tests compare with (float64 substitution) against extended precision, on one entry of every size"""
    for case, n in (("sqrexp", 1), ("matern52_ard8", 17), ("ard33", 128), ("gammaexp1", 128)):
        name, X, y, thetas, noises = R.models(case, n)
        Xs = P.grid_points(case, n)
        for (m, v), th, nz in zip(P.references(case, n), thetas, noises):
            want_m, want_v = P.closed_form(name, th, X, y, nz, Xs, P.LD)
            assert P.G.nerr(np.asarray(m, dtype=P.LD), want_m) <= 0.1 * TOL
            assert P.var_err(np.asarray(v, dtype=P.LD), want_v) <= 0.1 * TOL


def test_the_three_kinds_of_test_points():
    name, X, y, _, _ = R.models("ard3", 17)
    Xs = P.star_points(X)
    lo, hi = X.min(1), X.max(1)
    assert Xs.shape == (3, 37)
    assert ((Xs[:, :29] >= lo[:, None]) & (Xs[:, :29] <= hi[:, None])).all()
    assert np.array_equal(Xs[:, 29:34], X[:, :5])
    assert (np.abs(Xs[0, 34:] - X[0].mean()) >= 50 * (hi[0] - lo[0])).all()
    assert P.star_points(R.models("ard3", 1)[1]).shape == (3, 37)       # one training point: a box of no width


# ---- 2. BatchGPR pads unequal data sets and unequal test sets into the strided layout ------------------------------------------------------
class _StubLib:
    def __init__(self):
        self.fits, self.predicts, self.freed = [], [], []

    @staticmethod
    def _arr(addr, count, typ=C.c_double):
        return np.ctypeslib.as_array((typ * count).from_address(addr)).copy()

    def gprc_gpr_batch_fit(self, ctx, kid, B, params, n_params, ld_params, noise, X, d, n_max, x_stride, y, y_stride, n_each, model_out, logp, info):
        self.fits.append(dict(kid=kid, B=B, params=self._arr(params, B * ld_params).reshape(B, ld_params), n_params=n_params, noise=self._arr(noise, B),
                              X=self._arr(X, (B - 1) * x_stride + d * n_max), d=d, n_max=n_max, x_stride=x_stride,
                              y=self._arr(y, (B - 1) * y_stride + n_max), y_stride=y_stride, n_each=None if not n_each else self._arr(n_each, B, C.c_int64)))
        model_out._obj.value = 4242
        np.ctypeslib.as_array((C.c_double * B).from_address(logp))[:] = np.arange(B)
        np.ctypeslib.as_array((C.c_int * B).from_address(info))[:] = 0
        self.B, self.d = B, d
        return 0

    def gprc_gpr_batch_predict(self, model, Xs, ns_max, xs_stride, ns_each, mean, var, ld_out):
        B, d = self.B, self.d
        counts = None if not ns_each else self._arr(ns_each, B, C.c_int64)
        self.predicts.append(dict(model=model.value, Xs=self._arr(Xs, (B - 1) * xs_stride + d * ns_max), ns_max=ns_max, xs_stride=xs_stride, ns_each=counts,
                                  var=bool(var), ld_out=ld_out))
        for b in range(B):                       # what the library does: a model's count of entries, nothing behind it
            nb = ns_max if counts is None else int(counts[b])
            np.ctypeslib.as_array((C.c_double * nb).from_address(mean + 8 * b * ld_out))[:] = 100 * b + np.arange(nb)
            if var:
                np.ctypeslib.as_array((C.c_double * nb).from_address(var + 8 * b * ld_out))[:] = -(100 * b + np.arange(nb))
        return 0

    def gprc_batch_model_free(self, model):
        self.freed.append(model.value)
        return 0


class _StubCtx:
    handle = None


def test_batchgpr_pads_unequal_data_sets_and_unequal_test_sets(monkeypatch):
    stub = _StubLib()
    monkeypatch.setattr(nat, "lib", lambda: stub)
    rng = np.random.default_rng(5)
    d, sizes, stars = 3, [5, 1, 9, 4], [2, 7, 1, 3]
    Xs = [rng.normal(size=(d, n)) for n in sizes]
    ys = [rng.normal(size=n) for n in sizes]
    thetas = rng.uniform(0.5, 2.0, (4, d))
    g = BatchGPR(Xs, ys, [0.1, 0.2, 0.3, 0.4], "sqrexp_ard", thetas, ctx=_StubCtx())
    (c,) = stub.fits
    assert (c["B"], c["d"], c["n_max"], c["x_stride"], c["y_stride"], c["n_params"]) == (4, d, 9, d * 9, 9, d)
    assert c["kid"] == grad_dict["sqrexp_ard"].kernel_id
    assert np.array_equal(c["n_each"], sizes) and np.array_equal(c["noise"], [0.1, 0.2, 0.3, 0.4]) and np.array_equal(c["params"], thetas)
    for b, n in enumerate(sizes):
        slab = c["X"][b * d * 9:(b + 1) * d * 9]
        assert np.array_equal(slab[:d * n].reshape(n, d).T, Xs[b])        # point-major: coordinate r of point g at g d + r
        assert np.array_equal(c["y"][b * 9:b * 9 + n], ys[b])
    assert np.array_equal(g.logp, np.arange(4.0)) and np.array_equal(g.info, np.zeros(4)) and np.array_equal(g.n_each, sizes)
    # unequal test sets: one stride per model, the counts, lists back
    Ts = [rng.normal(size=(d, m)) for m in stars]
    mean, var = g.predict(Ts)
    q = stub.predicts[0]
    assert (q["model"], q["ns_max"], q["xs_stride"], q["ld_out"], q["var"]) == (4242, 7, d * 7, 7, True) and np.array_equal(q["ns_each"], stars)
    for b, m in enumerate(stars):
        assert np.array_equal(q["Xs"][b * d * 7:b * d * 7 + d * m].reshape(m, d).T, Ts[b])
        assert np.array_equal(mean[b], 100 * b + np.arange(m)) and np.array_equal(var[b], -(100 * b + np.arange(m)))
    # one shared set: no stride, no counts, arrays back; var=False passes NULL
    mean, var = g.predict(Ts[1], var=False)
    q = stub.predicts[1]
    assert (q["ns_max"], q["xs_stride"], q["ld_out"], q["var"]) == (7, 0, 7, False) and q["ns_each"] is None
    assert np.array_equal(q["Xs"].reshape(7, d).T, Ts[1]) and mean.shape == (4, 7) and var is None
    assert np.array_equal(mean[2], 200 + np.arange(7.0))
    with pytest.raises(ValueError):
        g.predict(Ts[:3])                                                  # one set per model
    with pytest.raises(ValueError):
        g.predict([rng.normal(size=(d + 1, 2))] * 4)                       # the models' d
    g.close()
    g.close()
    assert stub.freed == [4242]
    with pytest.raises(nat.GprcError):
        g.predict(Ts)
    # one shared data set: no strides, no n_each; more than 128 points is the single-model route's
    BatchGPR(Xs[2], ys[2], 0.25, "sqrexp_ard", thetas, ctx=_StubCtx())
    c = stub.fits[1]
    assert (c["x_stride"], c["y_stride"], c["n_max"]) == (0, 0, 9) and c["n_each"] is None and np.array_equal(c["noise"], np.full(4, 0.25))
    with pytest.raises(ValueError):
        BatchGPR(rng.normal(size=(d, 129)), rng.normal(size=129), 0.1, "sqrexp_ard", thetas, ctx=_StubCtx())
