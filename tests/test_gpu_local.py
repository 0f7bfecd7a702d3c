"""The local GPR on the device (gprc_lgpr_* and LocalGPR): against the float64 closed form on the reference neighbours, against the exact
GP when every point is a neighbour, the ordering of the variances in m, local models that are not positive definite among good ones,
the bit contract across the predict chunk, set_params, the neighbours, the Python round trip and the argument errors.  The references
of tests/local_ref.py are computed once per case and shared."""
import ctypes as C

import numpy as np
import pytest

import batch_predict_ref as P
import local_ref as LR
from conftest import TOL, nerr
from gprc_amd import LocalGPR, cov_func, matern32, matern52_ard, sqrexp
from gprc_amd import _native as nat
from gprc_amd.fit import grad_dict
from gpu_calls import kfun, step_time_limit  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu


def predict_once(name, theta, X, y, noise, m, Xs, **kw):
    rc, h = LR.lgpr_create(name, theta, X, y, noise, m)
    assert rc == nat.OK, nat.last_error()
    try:
        rc, mean, var, info = LR.lgpr_predict(h, Xs, **kw)
        assert rc == nat.OK, nat.last_error()
    finally:
        LR.lgpr_free(h)
    return mean, var, info


@pytest.mark.parametrize("m", LR.PREDICT_MS)
@pytest.mark.parametrize("case", LR.PREDICT_CASES)
def test_local_predict_against_the_closed_form_on_the_reference_neighbours(case, m):
    """n = 1000, 37 test points, five of them training points; mean normwise, variance per component relative to the variance itself"""
    name, theta, X, y, noise, Xs = LR.predict_case(case)
    want_m, want_v, _ = LR.predict_reference(case, m)
    mean, var, info = predict_once(name, theta, X, y, noise, m, Xs)
    assert not info.any()
    e_m, e_v = nerr(mean, want_m), P.var_err(var, want_v)
    print(f"local predict {case} m={m}: mean={e_m:.2e} var={e_v:.2e}")
    assert e_m <= TOL and e_v <= TOL


@pytest.mark.parametrize("case", ["sqrexp", "ard3", "matern52_ard8"])
def test_with_every_point_a_neighbour_it_is_the_exact_gp(case):
    name, theta, X, y, noise, Xs = LR.predict_case(case, 100)
    want_m, want_v = LR.exact_reference(case, 100)
    rc, h = LR.lgpr_create(name, theta, X, y, noise, 128)
    assert rc == nat.OK, nat.last_error()
    try:
        dims = [C.c_int64() for _ in range(3)]
        assert nat.lib().gprc_lgpr_dims(h, *[C.byref(v) for v in dims]) == nat.OK
        assert [v.value for v in dims] == [100, X.shape[0], 100]             # m is clamped to n
        rc, mean, var, info = LR.lgpr_predict(h, Xs)
        assert rc == nat.OK and not info.any()
    finally:
        LR.lgpr_free(h)
    e_m, e_v = nerr(mean, want_m), P.var_err(var, want_v)
    print(f"local predict, m >= n, {case}: mean={e_m:.2e} var={e_v:.2e}")
    assert e_m <= TOL and e_v <= TOL


@pytest.mark.parametrize("case", ["sqrexp", "ard3", "matern52_ard8"])
def test_more_neighbours_cannot_raise_the_variance(case):
    """var(m = 16) >= var(32) >= var(64) >= the exact GP's (the float64 closed form on all 1000 points), with the allowance of the CPU test"""
    name, theta, X, y, noise, Xs = LR.predict_case(case)
    vs = [predict_once(name, theta, X, y, noise, m, Xs)[1] for m in LR.ORDER_MS] + [LR.exact_reference(case)[1]]
    for a, b in zip(vs, vs[1:]):
        assert (a >= b - 1e-9).all(), float((b - a).max())


def test_flagged_local_models_are_nan_and_the_others_keep_their_bits():
    name, theta, X, Xdup, y, ydup, Xs, m = LR.flagged_data()
    mean, var, info = predict_once(name, theta, Xdup, ydup, 0.0, m, Xs)
    assert list(info[:2]) == [2, 2] and np.isnan(mean[:2]).all() and np.isnan(var[:2]).all()
    assert not info[2:].any() and np.isfinite(mean[2:]).all() and np.isfinite(var[2:]).all()
    mean0, var0, info0 = predict_once(name, theta, X, y, 0.0, m, Xs[:, 2:])      # the data without the duplicates, the other points
    assert not info0.any() and np.array_equal(mean[2:], mean0) and np.array_equal(var[2:], var0)
    mean1, _, _ = predict_once(name, theta, Xdup, ydup, 0.0, m, Xs, var=False, info=False)     # without var_out and info_out
    assert np.array_equal(mean1[2:], mean0) and np.isnan(mean1[:2]).all()


def test_a_point_s_bits_do_not_depend_on_the_chunk_or_its_place():
    """n* = 2049 straddles the predict chunk of 2048: points 0, 2047 and 2048 alone give the bits they have in the full call; so does
    a call from device pointers"""
    torch = pytest.importorskip("torch")
    name, theta, X, y, noise, _ = LR.predict_case("matern52_ard8")
    d = X.shape[0]
    rng = np.random.default_rng(2049)
    Xs = np.asfortranarray(rng.uniform(-2, 2, (d, 2049)))
    m = 8
    rc, h = LR.lgpr_create(name, theta, X, y, noise, m)
    assert rc == nat.OK, nat.last_error()
    try:
        rc, mean, var, info = LR.lgpr_predict(h, Xs)
        assert rc == nat.OK and not info.any() and np.isfinite(mean).all() and np.isfinite(var).all()
        for j in (0, 2047, 2048):
            rc, m1, v1, i1 = LR.lgpr_predict(h, Xs[:, j:j + 1])
            assert rc == nat.OK and m1[0] == mean[j] and v1[0] == var[j] and i1[0] == 0, j
        rc, m2, v2, _ = LR.lgpr_predict(h, Xs[:, 2040:])
        assert rc == nat.OK and np.array_equal(m2, mean[2040:]) and np.array_equal(v2, var[2040:])
        xd = torch.from_numpy(LR.flat(Xs)).cuda()
        mt = torch.full((2049,), -7.0, dtype=torch.float64, device="cuda")
        vt = torch.full((2049,), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert nat.lib().gprc_lgpr_predict(h, xd.data_ptr(), 2049, mt.data_ptr(), vt.data_ptr(), None) == nat.OK, nat.last_error()
        assert np.array_equal(mt.cpu().numpy(), mean) and np.array_equal(vt.cpu().numpy(), var)
    finally:
        LR.lgpr_free(h)
    want_m, want_v, _ = LR.local_predict_ref(name, theta, X, y, noise, Xs[:, 2040:], m)
    assert nerr(mean[2040:], want_m) <= TOL and P.var_err(var[2040:], want_v) <= TOL


def test_set_params_equals_a_fresh_model_and_neighbours_are_dev_knn():
    name, theta, X, y, noise, Xs = LR.predict_case("matern52_ard8")
    d, n = X.shape
    theta2, noise2, m = theta[::-1].copy() * 1.3, 0.03, 33
    fresh = predict_once(name, theta2, X, y, noise2, m, Xs)
    rc, h = LR.lgpr_create(name, theta, X, y, noise, m)
    assert rc == nat.OK, nat.last_error()
    try:
        first = LR.lgpr_predict(h, Xs)
        _, pp, npar = nat.params_array(theta2)
        assert nat.lib().gprc_lgpr_set_params(h, pp, npar, noise2) == nat.OK, nat.last_error()
        again = LR.lgpr_predict(h, Xs)
        assert again[0] == nat.OK and all(np.array_equal(a, b) for a, b in zip(again[1:], fresh))
        assert not np.array_equal(first[1], again[1])
        ns = Xs.shape[1]
        idx, dist = np.full((ns, m), -7, dtype=np.intc), np.full((ns, m), -7.0)
        assert nat.lib().gprc_lgpr_neighbours(h, Xs.ctypes.data, ns, idx.ctypes.data, dist.ctypes.data, m) == nat.OK, nat.last_error()
        rc, want_i, want_d = LR.call_knn(LR.flat(X), d, n, LR.flat(Xs), ns, m, 1.0 / theta2)
        assert rc == nat.OK and np.array_equal(idx, want_i) and np.array_equal(dist, want_d)
        assert np.array_equal(idx, LR.knn_ref(X, Xs, m, 1.0 / theta2)[0])
    finally:
        LR.lgpr_free(h)
    # an isotropic kernel searches in the Euclidean metric
    rc, h = LR.lgpr_create("matern52", [1.1], X, y, noise, m)
    assert rc == nat.OK, nat.last_error()
    try:
        assert nat.lib().gprc_lgpr_neighbours(h, Xs.ctypes.data, ns, idx.ctypes.data, dist.ctypes.data, m) == nat.OK
        rc, want_i, want_d = LR.call_knn(LR.flat(X), d, n, LR.flat(Xs), ns, m)
        assert rc == nat.OK and np.array_equal(idx, want_i) and np.array_equal(dist, want_d)
    finally:
        LR.lgpr_free(h)


def test_the_python_round_trip():
    name, theta, X, y, noise, Xs = LR.predict_case("matern52_ard8")
    want_m, want_v, want_i = LR.predict_reference("matern52_ard8", 64)
    with LocalGPR(X, y, noise, cov_func(matern52_ard, l=theta), m=64) as g:
        assert g.m == 64 and g.info is None
        out = g.predict(Xs)
        assert out.shape == (Xs.shape[1], 2) and not g.info.any()
        assert nerr(out[:, 0], want_m) <= TOL and P.var_err(out[:, 1], want_v) <= TOL
        assert np.array_equal(g.predict(Xs, pointwise_var=False), out[:, 0])
        idx, dist = g.neighbours(Xs)
        assert np.array_equal(idx, want_i) and dist.shape == idx.shape and (np.diff(dist, axis=1) >= 0).all()
        g.set_params(cov_func(matern52_ard, l=theta * 2.0), 0.05)
        again = g.predict(Xs)
        with LocalGPR(X, y, 0.05, kfun(name, theta * 2.0), m=64) as g2:
            assert np.array_equal(g2.predict(Xs), again)
        with pytest.raises(ValueError):
            g.set_params(cov_func(sqrexp, l=1.0), 0.05)
    with pytest.raises(nat.GprcError):
        g.predict(Xs)                                     # after close
    with pytest.raises(nat.GprcError):
        g.neighbours(Xs)
    g.close()                                             # twice is fine
    with LocalGPR(X[:, :40], y[:40], noise, cov_func(matern32, l=0.9), m=128) as g:
        assert g.m == 40 and g.predict(Xs).shape == (Xs.shape[1], 2)


def test_argument_errors():
    name, theta, X, y, noise, Xs = LR.predict_case("ard3")
    lib, ctx = nat.lib(), nat.default_context()
    d, n = X.shape
    _, pp, npar = nat.params_array(theta)
    h = C.c_void_p()
    mean, var = np.zeros(4), np.zeros(4)

    def bad(rc, word):
        assert rc == nat.ERR_ARG and word in nat.last_error(), (rc, nat.last_error())

    kid = grad_dict[name].kernel_id
    bad(lib.gprc_lgpr_create(None, kid, pp, npar, X.ctypes.data, d, n, y.ctypes.data, noise, 8, C.byref(h)), "null context")
    bad(lib.gprc_lgpr_create(ctx.handle, nat.LINEAR, pp, npar, X.ctypes.data, d, n, y.ctypes.data, noise, 8, C.byref(h)), "defined for")
    bad(lib.gprc_lgpr_create(ctx.handle, kid, pp, npar, None, d, n, y.ctypes.data, noise, 8, C.byref(h)), "null input")
    bad(lib.gprc_lgpr_create(ctx.handle, kid, pp, npar, X.ctypes.data, d, n, None, noise, 8, C.byref(h)), "null input")
    bad(lib.gprc_lgpr_create(ctx.handle, kid, pp, npar, X.ctypes.data, d, n, y.ctypes.data, noise, 8, None), "null output")
    bad(lib.gprc_lgpr_create(ctx.handle, kid, None, npar, X.ctypes.data, d, n, y.ctypes.data, noise, 8, C.byref(h)), "params")
    bad(lib.gprc_lgpr_create(ctx.handle, kid, pp, npar, X.ctypes.data, d, n, y.ctypes.data, noise, 0, C.byref(h)), "m < 1")
    bad(lib.gprc_lgpr_create(ctx.handle, kid, pp, npar, X.ctypes.data, d, 2 ** 31, y.ctypes.data, noise, 8, C.byref(h)), "2^31")
    bad(lib.gprc_lgpr_create(ctx.handle, kid, pp, npar - 1, X.ctypes.data, d, n, y.ctypes.data, noise, 8, C.byref(h)), "length scale")
    bad(lib.gprc_lgpr_create(ctx.handle, kid, pp, npar, X.ctypes.data, d, n, y.ctypes.data, -1.0, 8, C.byref(h)), "noise")
    assert not h
    bad(lib.gprc_lgpr_predict(None, Xs.ctypes.data, 4, mean.ctypes.data, var.ctypes.data, None), "null model")
    assert lib.gprc_lgpr_free(None) == nat.OK
    rc, h = LR.lgpr_create(name, theta, X, y, noise, 8)
    assert rc == nat.OK, nat.last_error()
    try:
        bad(lib.gprc_lgpr_predict(h, None, 4, mean.ctypes.data, var.ctypes.data, None), "null input")
        bad(lib.gprc_lgpr_predict(h, Xs.ctypes.data, 4, None, var.ctypes.data, None), "null output")
        bad(lib.gprc_lgpr_set_params(h, pp, npar, float("nan")), "noise")
        idx = np.zeros((4, 8), dtype=np.intc)
        bad(lib.gprc_lgpr_neighbours(h, Xs.ctypes.data, 4, idx.ctypes.data, None, 7), "ld_out < m")
        bad(lib.gprc_lgpr_neighbours(h, Xs.ctypes.data, 4, None, None, 8), "null output")
        assert lib.gprc_lgpr_predict(h, Xs.ctypes.data, 0, mean.ctypes.data, var.ctypes.data, None) == nat.OK    # no test points
    finally:
        LR.lgpr_free(h)
    # a model outlives its context only to be freed
    own = nat.Context(0)
    rc, h = LR.lgpr_create(name, theta, X, y, noise, 8, ctx=own)
    assert rc == nat.OK, nat.last_error()
    own.close()
    bad(lib.gprc_lgpr_predict(h, Xs.ctypes.data, 4, mean.ctypes.data, var.ctypes.data, None), "context has been destroyed")
    assert lib.gprc_lgpr_free(h) == nat.OK
