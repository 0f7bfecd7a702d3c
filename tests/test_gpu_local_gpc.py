"""The local classifier on the device (gprc_lgpc_* and LocalGPC): against the tightly converged numpy reference on the reference
neighbours, against the full classifier when every point is a neighbour, the bit contract across the predict chunk, set_params, the
neighbours, outputs left out, the argument errors and the Python round trip.  The references of tests/batch_gpc_ref.py are computed
once per case and shared; every mode search runs at batch_gpc_ref.EPS = 1e-12."""
import ctypes as C

import numpy as np
import pytest

import batch_gpc_ref as G
import batch_predict_ref as P
import local_ref as LR
from conftest import TOL, nerr
from gprc_amd import GPC, LocalGPC
from gprc_amd import _native as nat
from gprc_amd.fit import grad_dict
from gpu_calls import kfun, step_time_limit  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu


def predict_once(name, theta, X, y, m, Xs, **kw):
    rc, h = G.lgpc_create(name, theta, X, y, m)
    assert rc == nat.OK, nat.last_error()
    try:
        out = G.lgpc_predict(h, Xs, **kw)
        assert out[0] == nat.OK, nat.last_error()
    finally:
        G.lgpc_free(h)
    return out[1:]


@pytest.mark.parametrize("m", G.LOCAL_MS)
@pytest.mark.parametrize("case", list(G.CASES))
def test_local_classifier_against_the_converged_reference_on_the_reference_neighbours(case, m):
    """n = 1000, 37 test points, five of them training points; neighbourhoods of a single class (all 37 at m = 1) included"""
    name, theta, X, y, Xs = G.case_data(case)
    ref = G.local_reference(case, m)
    fs, vf, prob, iters, info = predict_once(name, theta, X, y, m, Xs)
    assert not info.any()
    e = dict(fs=nerr(fs, ref["fs"]), vf=G.var_err(vf, ref["vf"]), prob=float(np.abs(prob - ref["prob"]).max()))
    print(f"local gpc {case} m={m}:", {k: "%.2e" % v for k, v in e.items()}, "iterations", iters.min(), "..", iters.max(), "single-class", ref["single_class"])
    assert all(v <= TOL for v in e.values()), e
    assert np.abs(iters - ref["iters"]).max() <= 1


@pytest.mark.parametrize("case", ["sqrexp", "ard3", "matern52_ard8"])
def test_with_every_point_a_neighbour_it_is_the_full_classifier(case):
    name, theta, X, y, Xs = G.case_data(case, 100)
    rc, h = G.lgpc_create(name, theta, X, y, 128)
    assert rc == nat.OK, nat.last_error()
    try:
        dims = [C.c_int64() for _ in range(3)]
        assert nat.lib().gprc_lgpr_dims(h, *[C.byref(v) for v in dims]) == nat.OK
        assert [v.value for v in dims] == [100, X.shape[0], 100]             # m is clamped to n
        rc, fs, vf, prob, iters, info = G.lgpc_predict(h, Xs)
        assert rc == nat.OK and not info.any()
    finally:
        G.lgpc_free(h)
    # the order of a model's points is the neighbour order, another one per test point: to rounding, not to the bit
    with GPC(X, y, kfun(name, theta), G.EPS, reference_stop=False) as gc:
        gfs, gvf = gc.predict_latent(Xs)
        gprob = gc.predict_class(Xs)
        assert np.abs(iters - gc.iterations).max() <= 1
    e = dict(fs=nerr(fs, gfs), vf=P.var_err(vf, gvf), prob=float(np.abs(prob - gprob).max()))
    ref = G.converged(name, theta, X, y, Xs)
    r = dict(fs=nerr(fs, ref["fs"]), vf=G.var_err(vf, ref["vf"]), prob=float(np.abs(prob - ref["prob"]).max()))
    print(f"local gpc, m >= n, {case}: against gprc_gpc_fit", {k: "%.2e" % v for k, v in e.items()}, "against numpy", {k: "%.2e" % v for k, v in r.items()})
    assert all(v <= TOL for v in e.values()) and all(v <= TOL for v in r.values())


def test_a_point_s_bits_do_not_depend_on_the_chunk_or_its_place():
    """n* = 2049 straddles the predict chunk of 2048: points 0, 2047 and 2048 alone give the bits they have in the full call; so does
    a call from device pointers"""
    torch = pytest.importorskip("torch")
    name, theta, X, y, _ = G.case_data("matern52_ard8")
    d = X.shape[0]
    Xs = np.asfortranarray(np.random.default_rng(2049).uniform(-1, 1, (d, 2049)))
    m = 8
    rc, h = G.lgpc_create(name, theta, X, y, m)
    assert rc == nat.OK, nat.last_error()
    try:
        rc, fs, vf, prob, iters, info = G.lgpc_predict(h, Xs)
        assert rc == nat.OK and not info.any() and all(np.isfinite(v).all() for v in (fs, vf, prob)) and iters.min() >= 3
        for j in (0, 2047, 2048):
            rc, f1, v1, p1, it1, i1 = G.lgpc_predict(h, Xs[:, j:j + 1])
            assert rc == nat.OK and (f1[0], v1[0], p1[0], it1[0], i1[0]) == (fs[j], vf[j], prob[j], iters[j], 0), j
        rc, f2, v2, p2, _, _ = G.lgpc_predict(h, Xs[:, 2040:])
        assert rc == nat.OK and np.array_equal(f2, fs[2040:]) and np.array_equal(v2, vf[2040:]) and np.array_equal(p2, prob[2040:])
        xd = torch.from_numpy(LR.flat(Xs)).cuda()
        outs = [torch.full((2049,), -7.0, dtype=torch.float64, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        out = G.lgpc_predict(h, xd, 2049, *outs)
        assert out[0] == nat.OK, nat.last_error()
        assert all(np.array_equal(t.cpu().numpy(), want) for t, want in zip(outs, (fs, vf, prob)))
        assert np.array_equal(out[4], iters) and not out[5].any()
    finally:
        G.lgpc_free(h)
    tail = [G.converged(name, theta, X[:, nb], y[nb], Xs[:, 2040 + j:2041 + j]) for j, nb in enumerate(LR.knn_ref(X, Xs[:, 2040:], m, LR.metric_of(name, theta))[0])]
    assert nerr(fs[2040:], np.array([t["fs"][0] for t in tail])) <= TOL and np.abs(prob[2040:] - np.array([t["prob"][0] for t in tail])).max() <= TOL


def test_set_params_equals_a_fresh_model_and_neighbours_are_the_regression_object_s():
    name, theta, X, y, Xs = G.case_data("matern52_ard8")
    d, n = X.shape
    ns = Xs.shape[1]
    theta2, m = theta[::-1].copy() * 1.3, 33
    fresh = predict_once(name, theta2, X, y, m, Xs)
    rc, h = G.lgpc_create(name, theta, X, y, m)
    assert rc == nat.OK, nat.last_error()
    rc, hr = LR.lgpr_create(name, theta2, X, np.sin(X.sum(0)), 0.1, m)
    assert rc == nat.OK, nat.last_error()
    try:
        first = G.lgpc_predict(h, Xs)
        _, pp, npar = nat.params_array(theta2)
        assert nat.lib().gprc_lgpc_set_params(h, pp, npar) == nat.OK, nat.last_error()
        again = G.lgpc_predict(h, Xs)
        assert again[0] == nat.OK and all(np.array_equal(a, b) for a, b in zip(again[1:], fresh))
        assert not np.array_equal(first[1], again[1])
        got = [np.full((ns, m), -7, dtype=np.intc), np.full((ns, m), -7.0)]
        want = [np.full((ns, m), -7, dtype=np.intc), np.full((ns, m), -7.0)]
        assert nat.lib().gprc_lgpr_neighbours(h, Xs.ctypes.data, ns, got[0].ctypes.data, got[1].ctypes.data, m) == nat.OK, nat.last_error()
        assert nat.lib().gprc_lgpr_neighbours(hr, Xs.ctypes.data, ns, want[0].ctypes.data, want[1].ctypes.data, m) == nat.OK, nat.last_error()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(got[0], LR.knn_ref(X, Xs, m, 1.0 / theta2)[0])
    finally:
        G.lgpc_free(h)
        LR.lgpr_free(hr)


def test_outputs_left_out_keep_the_others_bits():
    name, theta, X, y, Xs = G.case_data("ard3")
    m = 17
    fs, vf, prob, iters, info = predict_once(name, theta, X, y, m, Xs)
    for want in ((True, False, False), (False, True, False), (False, False, True), (True, False, True), (False, True, True), (True, True, False)):
        out = predict_once(name, theta, X, y, m, Xs, fs=want[0], vf=want[1], prob=want[2], iters=False, info=False)
        for got, full, asked in zip(out[:3], (fs, vf, prob), want):
            assert (got is None) if not asked else np.array_equal(got, full), want
        assert out[3] is None and out[4] is None
    again = predict_once(name, theta, X, y, m, Xs)
    assert np.array_equal(again[3], iters) and np.array_equal(again[4], info)


def test_argument_errors():
    name, theta, X, y, Xs = G.case_data("ard3")
    lib, ctx = nat.lib(), nat.default_context()
    d, n = X.shape
    _, pp, npar = nat.params_array(theta)
    h = C.c_void_p()
    out = np.zeros((3, 4))
    o = [r.ctypes.data for r in out]

    def bad(rc, word):
        assert rc == nat.ERR_ARG and word in nat.last_error(), (rc, nat.last_error())

    kid = grad_dict[name].kernel_id
    bad(lib.gprc_lgpc_create(None, kid, pp, npar, X.ctypes.data, d, n, y.ctypes.data, 8, G.EPS, 0, C.byref(h)), "null context")
    bad(lib.gprc_lgpc_create(ctx.handle, nat.LINEAR, pp, npar, X.ctypes.data, d, n, y.ctypes.data, 8, G.EPS, 0, C.byref(h)), "defined for")
    bad(lib.gprc_lgpc_create(ctx.handle, kid, pp, npar, None, d, n, y.ctypes.data, 8, G.EPS, 0, C.byref(h)), "null input")
    bad(lib.gprc_lgpc_create(ctx.handle, kid, pp, npar, X.ctypes.data, d, n, None, 8, G.EPS, 0, C.byref(h)), "null input")
    bad(lib.gprc_lgpc_create(ctx.handle, kid, pp, npar, X.ctypes.data, d, n, y.ctypes.data, 8, G.EPS, 0, None), "null output")
    bad(lib.gprc_lgpc_create(ctx.handle, kid, None, npar, X.ctypes.data, d, n, y.ctypes.data, 8, G.EPS, 0, C.byref(h)), "params")
    bad(lib.gprc_lgpc_create(ctx.handle, kid, pp, npar, X.ctypes.data, d, n, y.ctypes.data, 0, G.EPS, 0, C.byref(h)), "m < 1")
    bad(lib.gprc_lgpc_create(ctx.handle, kid, pp, npar, X.ctypes.data, d, 2 ** 31, y.ctypes.data, 8, G.EPS, 0, C.byref(h)), "2^31")
    bad(lib.gprc_lgpc_create(ctx.handle, kid, pp, npar - 1, X.ctypes.data, d, n, y.ctypes.data, 8, G.EPS, 0, C.byref(h)), "length scale")
    bad(lib.gprc_lgpc_create(ctx.handle, kid, pp, npar, X.ctypes.data, d, n, y.ctypes.data, 8, 0.0, 0, C.byref(h)), "epsilon")
    bad(lib.gprc_lgpc_create(ctx.handle, kid, pp, npar, X.ctypes.data, d, n, y.ctypes.data, 8, G.EPS, 1001, C.byref(h)), "max_iter")
    assert not h
    bad(lib.gprc_lgpc_predict(None, Xs.ctypes.data, 4, o[0], o[1], o[2], None, None), "null model")
    rc, h = G.lgpc_create(name, theta, X, y, 8)
    assert rc == nat.OK, nat.last_error()
    rc, hr = LR.lgpr_create(name, theta, X, y, 0.1, 8)
    assert rc == nat.OK, nat.last_error()
    try:
        torch = pytest.importorskip("torch")
        bad(lib.gprc_lgpc_predict(h, None, 4, o[0], o[1], o[2], None, None), "null input")
        bad(lib.gprc_lgpc_predict(h, Xs.ctypes.data, 4, None, None, None, None, None), "not all three")
        bad(lib.gprc_lgpc_predict(h, Xs.ctypes.data, -1, o[0], o[1], o[2], None, None), "n_star < 0")
        dev = torch.zeros(4, dtype=torch.int32, device="cuda")
        bad(lib.gprc_lgpc_predict(h, Xs.ctypes.data, 4, o[0], o[1], o[2], dev.data_ptr(), None), "host memory")
        bad(lib.gprc_lgpc_predict(h, Xs.ctypes.data, 4, o[0], o[1], o[2], None, dev.data_ptr()), "host memory")
        assert lib.gprc_lgpc_predict(h, Xs.ctypes.data, 0, o[0], o[1], o[2], None, None) == nat.OK    # no test points
        assert not out.any()
        # the wrong kind, both ways
        bad(lib.gprc_lgpr_predict(h, Xs.ctypes.data, 4, o[0], o[1], None), "local classifier")
        bad(lib.gprc_lgpr_set_params(h, pp, npar, 0.1), "local classifier")
        bad(lib.gprc_lgpr_vecchia_prepare(h, 4), "local classifier")
        idx = np.zeros((n, 4), dtype=np.intc)
        bad(lib.gprc_lgpr_vecchia_neighbours(h, idx.ctypes.data, 4), "local classifier")
        lp = C.c_double()
        bad(lib.gprc_lgpr_vecchia_logp_grad(h, pp, npar, 0.1, C.byref(lp), None, None, None), "local classifier")
        bad(lib.gprc_lgpc_predict(hr, Xs.ctypes.data, 4, o[0], o[1], o[2], None, None), "local regression")
        bad(lib.gprc_lgpc_set_params(hr, pp, npar), "local regression")
        assert not out.any()
    finally:
        G.lgpc_free(h)
        LR.lgpr_free(hr)
    own = nat.Context(0)
    rc, h = G.lgpc_create(name, theta, X, y, 8, ctx=own)
    assert rc == nat.OK, nat.last_error()
    own.close()
    bad(lib.gprc_lgpc_predict(h, Xs.ctypes.data, 4, o[0], o[1], o[2], None, None), "context has been destroyed")
    assert lib.gprc_lgpr_free(h) == nat.OK


def test_localgpc_round_trip():
    case = "matern52_ard8"
    name, theta, X, y, Xs = G.case_data(case)
    ref = G.local_reference(case, 64)
    with LocalGPC(X, y, kfun(name, theta), m=64, epsilon=G.EPS) as g:
        assert g.m == 64 and g.info is None and g.iters is None
        fs, vf = g.predict_latent(Xs)
        assert not g.info.any() and np.abs(g.iters - ref["iters"]).max() <= 1
        prob = g.predict_class(Xs)
        assert nerr(fs, ref["fs"]) <= TOL and G.var_err(vf, ref["vf"]) <= TOL and np.abs(prob - ref["prob"]).max() <= TOL
        idx, dist = g.neighbours(Xs)
        assert np.array_equal(idx, G.local_neighbours(case, 64)) and (np.diff(dist, axis=1) >= 0).all()
        g.set_params(kfun(name, theta * 2.0))
        again = g.predict_class(Xs)
        with LocalGPC(X, y, kfun(name, theta * 2.0), m=64, epsilon=G.EPS) as g2:
            assert np.array_equal(g2.predict_class(Xs), again)
        assert not np.array_equal(again, prob)
        with pytest.raises(ValueError):
            g.set_params(kfun("sqrexp", [1.0]))
    with pytest.raises(nat.GprcError):
        g.predict_class(Xs)                               # after close
    g.close()                                             # twice is fine
    with LocalGPC(X[:, :40], y[:40], kfun("matern32", [0.9]), m=128) as g:
        assert g.m == 40 and g.predict_class(Xs).shape == (Xs.shape[1],)
