"""The batched Laplace classifier on the device (gprc_gpc_batch_* and BatchGPC): against the tightly converged numpy reference at the
16-row block edges, the bit contract of a model across batches, against the single-model path (gprc_gpc_fit), the iteration cap, a
model with a NaN coordinate among good ones, handles of the wrong kind, a handle that outlives its context and the Python round trip.
The references of tests/batch_gpc_ref.py are computed once and shared; every mode search runs at batch_gpc_ref.EPS = 1e-12.

Worst figures measured on an MI355X against the converged reference (bound conftest.TOL = 1e-10): see README.md, "Batched and local GPC"."""
import ctypes as C

import numpy as np
import pytest

import batch_gpc_ref as G
import batch_predict_ref as P
from conftest import TOL, nerr
from gprc_amd import GPC, BatchGPC
from gprc_amd import _native as nat
from gprc_amd.fit import grad_dict
from gpu_calls import kfun, raw_logq_grad, step_time_limit  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu

N_MAX = 128


def strided(case, sizes, poison=np.nan):
    """the first n_b points of the case's data set per model, in one strided array each; what lies behind a model's points is `poison`"""
    name, theta, X, y, Xs = G.case_data(case)
    d = X.shape[0]
    Xb, yb = np.full((len(sizes), d * N_MAX), poison), np.full((len(sizes), N_MAX), poison)
    for b, nb in enumerate(sizes):
        Xb[b, :d * nb] = G.flat(X[:, :nb])
        yb[b, :nb] = y[:nb]
    return name, theta, d, Xb, yb, G.flat(Xs)


def fit_and_predict(name, thetas, X, d, n_max, y, xs, B, **kw):
    """one fit and every output of it: [logq, iters, info, f_hat, fs_bar, Vfs, prob], the test points shared"""
    rc, h, logq, iters, info = G.call_fit(name, thetas, X, d, n_max, y, **kw)
    assert rc == nat.OK, nat.last_error()
    try:
        f_hat = G.get_f_hat(h, B, n_max)
        rc, fs, vf = G.call_latent(h, B, xs, G.NS)
        assert rc == nat.OK, nat.last_error()
        rc, prob = G.call_class(h, B, xs, G.NS)
        assert rc == nat.OK, nat.last_error()
    finally:
        G.free(h)
    return [logq, iters, info, f_hat, fs, vf, prob]


_RUNS = {}


def seven(case):
    """the batch that holds all seven sizes through n_each, fitted once per case"""
    if case not in _RUNS:
        name, theta, d, Xb, yb, xs = strided(case, G.SIZES)
        B = len(G.SIZES)
        _RUNS[case] = fit_and_predict(name, np.tile(theta, (B, 1)), Xb, d, N_MAX, yb, xs, B, x_stride=d * N_MAX, y_stride=N_MAX, n_each=G.SIZES)
    return _RUNS[case]


def row(out, b, nb=None):
    """model b's part of every output of fit_and_predict (f_hat cut to its n_b points)"""
    return [out[0][b], out[1][b], out[2][b], out[3][b, :nb], out[4][b], out[5][b], out[6][b]]


def same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("case", list(G.CASES))
def test_against_the_converged_reference(case):
    """f_hat and the latent mean normwise, the variance per component relative to itself, |delta logq| <= TOL max(1, |logq|), the
    probability absolute, the iterations to one step; 37 test points, five of them training points"""
    logq, iters, info, f_hat, fs, vf, prob = seven(case)
    assert not info.any()
    for b, nb in enumerate(G.SIZES):
        ref = G.batch_reference(case, nb)
        e = dict(f=nerr(f_hat[b, :nb], ref["f"]), fs=nerr(fs[b], ref["fs"]), vf=G.var_err(vf[b], ref["vf"]), prob=float(np.abs(prob[b] - ref["prob"]).max()),
                 logq=abs(logq[b] - ref["logq"]) / max(1.0, abs(ref["logq"])))
        print(f"batch gpc {case} n_b={nb}:", {k: "%.2e" % v for k, v in e.items()}, "iterations", iters[b], ref["iters"])
        assert all(v <= TOL for v in e.values()), (nb, e)
        assert abs(int(iters[b]) - ref["iters"]) <= 1
        assert not f_hat[b, nb:].any()                                   # zero behind n_b


@pytest.mark.parametrize("case", ["sqrexp", "matern52_ard8"])
def test_a_model_s_bits_do_not_depend_on_the_batch(case):
    torch = pytest.importorskip("torch")
    assert G.batch_reference(case, 1)["iters"] == 3 and G.batch_reference(case, 128)["iters"] >= 5     # the batch mixes iteration counts
    full = seven(case)
    name, theta, d, Xb, yb, xs = strided(case, G.SIZES)
    B = len(G.SIZES)
    thetas = np.tile(theta, (B, 1))
    kw = dict(x_stride=d * N_MAX, y_stride=N_MAX)
    # alone: B = 1, n_max = n_b, no n_each
    for b, nb in enumerate(G.SIZES):
        alone = fit_and_predict(name, theta, Xb[b, :d * nb].copy(), d, nb, yb[b, :nb].copy(), xs, 1)
        assert same(row(alone, 0, nb), row(full, b, nb)), nb
    # any permutation
    perm = np.random.default_rng(7).permutation(B)
    shuffled = fit_and_predict(name, thetas, Xb[perm].copy(), d, N_MAX, yb[perm].copy(), xs, B, n_each=np.array(G.SIZES)[perm], **kw)
    for k, b in enumerate(perm):
        assert same(row(shuffled, k, G.SIZES[b]), row(full, b, G.SIZES[b])), (k, b)
    # a second call; without iters_out; from device pointers
    again = fit_and_predict(name, thetas, Xb, d, N_MAX, yb, xs, B, n_each=G.SIZES, **kw)
    assert same(again, full)
    quiet = fit_and_predict(name, thetas, Xb, d, N_MAX, yb, xs, B, n_each=G.SIZES, iters=False, **kw)
    assert quiet[1] is None and same(quiet[:1] + quiet[2:], full[:1] + full[2:])
    clean = np.nan_to_num(Xb, nan=0.5), np.nan_to_num(yb, nan=1.0)       # (what lies behind n_b is never read: other padding, same bits)
    xd, yd, xsd = torch.from_numpy(clean[0]).cuda(), torch.from_numpy(clean[1]).cuda(), torch.from_numpy(xs).cuda()
    torch.cuda.synchronize()
    dev = fit_and_predict(name, thetas, xd, d, N_MAX, yd, xsd, B, n_each=G.SIZES, **kw)
    assert same(dev, full)
    # shared against strided data: three parameter vectors on the 127 points
    _, _, X, y, _ = G.case_data(case)
    th3 = np.stack([theta, 1.3 * theta, 0.8 * theta])
    shared = fit_and_predict(name, th3, G.flat(X[:, :127]), d, 127, y[:127].copy(), xs, 3)
    copies = fit_and_predict(name, th3, np.tile(G.flat(X[:, :127]), (3, 1)), d, 127, np.tile(y[:127], (3, 1)), xs, 3, x_stride=d * 127, y_stride=127)
    assert same(shared, copies) and same(row(shared, 0, 127), row(full, G.SIZES.index(127), 127))
    assert not same(row(shared, 1), row(shared, 0))


@pytest.mark.parametrize("case", list(G.CASES))
def test_against_the_single_model_path_on_the_device(case):
    """gprc_gpc_fit (flags 0, the same epsilon) + gprc_gpc_predict_latent + gprc_gpc_predict_class, and gprc_gpc_logq_grad's value at 128"""
    name, theta, X, y, Xs = G.case_data(case)
    full = seven(case)
    for nb in (17, 128):
        b = G.SIZES.index(nb)
        Xn = np.asfortranarray(X[:, :nb])
        with GPC(Xn, y[:nb], kfun(name, theta), G.EPS, reference_stop=False) as gc:
            fs, vf = gc.predict_latent(Xs)
            prob = gc.predict_class(Xs)
            e = dict(f=nerr(full[3][b, :nb], gc.f_hat), fs=nerr(full[4][b], fs), vf=P.var_err(full[5][b], vf), prob=float(np.abs(full[6][b] - prob).max()))
            assert abs(int(full[1][b]) - gc.iterations) <= 1
        if nb == 128:
            lq, _, _ = raw_logq_grad(grad_dict[name].kernel_id, theta, Xn.ctypes.data, X.shape[0], nb, y[:nb].ctypes.data, nat.default_context(), epsilon=G.EPS)
            e["logq"] = abs(full[0][b] - lq) / max(1.0, abs(lq))
        print(f"batch gpc against gprc_gpc_fit {case} n_b={nb}:", {k: "%.2e" % v for k, v in e.items()})
        assert all(v <= TOL for v in e.values()), e


def test_the_cap_flags_the_slow_models_and_keeps_the_fast_ones():
    """max_iter = c with models on both sides of it.  A model the reference finishes in <= c - 1 iterations finishes on the device by
    iteration c at the latest (a decrement within rounding of epsilon costs one more, and convergence is judged before the cap): it
    keeps the bits of the uncapped run.  A model the reference needs >= c + 1 iterations for, whose decrement at iteration c is above
    1.2 epsilon -- the margin within which device and numpy may differ -- cannot have converged by c: it reports the cap.  The others
    (exactly c in the reference, or a decrement inside the margin) are not judged."""
    case, c = "ard3", 4
    refs = [G.batch_reference(case, nb) for nb in G.SIZES]
    fast = [b for b, r in enumerate(refs) if r["iters"] <= c - 1]
    slow = [b for b, r in enumerate(refs) if r["iters"] >= c + 1 and r["decrements"][c - 2] > 1.2 * G.EPS]
    assert fast and slow, [r["iters"] for r in refs]
    full = seven(case)
    name, theta, d, Xb, yb, xs = strided(case, G.SIZES)
    B = len(G.SIZES)
    capped = fit_and_predict(name, np.tile(theta, (B, 1)), Xb, d, N_MAX, yb, xs, B, x_stride=d * N_MAX, y_stride=N_MAX, n_each=G.SIZES, max_iter=c)   # GPRC_OK
    for b in fast:
        assert same(row(capped, b, G.SIZES[b]), row(full, b, G.SIZES[b])), b
    for b in slow:
        nb = G.SIZES[b]
        assert capped[2][b] == G.MAXITER and capped[1][b] == c
        assert np.isnan(capped[0][b]) and np.isnan(capped[3][b, :nb]).all() and not capped[3][b, nb:].any()
        assert np.isnan(capped[4][b]).all() and np.isnan(capped[5][b]).all() and np.isnan(capped[6][b]).all()
    assert set(capped[2]) <= {0, G.MAXITER}


def test_a_model_with_a_nan_coordinate_is_flagged_and_its_neighbours_keep_their_bits():
    case, sizes = "matern52_ard8", (17, 128, 16)
    name, theta, d, Xb, yb, xs = strided(case, sizes)
    thetas = np.tile(theta, (3, 1))
    kw = dict(x_stride=d * N_MAX, y_stride=N_MAX, n_each=sizes)
    good = fit_and_predict(name, thetas, Xb, d, N_MAX, yb, xs, 3, **kw)
    bad = Xb.copy()
    bad[1, d * 5 + 2] = np.nan                                          # coordinate 2 of point 5 of the middle model
    out = fit_and_predict(name, thetas, bad, d, N_MAX, yb, xs, 3, max_iter=20, **kw)
    assert out[2][1] != 0 and 1 <= out[1][1] <= 20                      # flagged, within the bound
    assert np.isnan(out[0][1]) and np.isnan(out[3][1, :128]).all() and np.isnan(out[4][1]).all() and np.isnan(out[5][1]).all() and np.isnan(out[6][1]).all()
    for b in (0, 2):
        assert same(row(out, b, sizes[b]), row(good, b, sizes[b])) and out[2][b] == 0


def test_gaps_in_the_outputs_are_left_as_they_were():
    case, sizes = "sqrexp", (15, 128)
    name, theta, d, Xb, yb, xs = strided(case, sizes)
    rc, h, _, _, info = G.call_fit(name, np.tile(theta, (2, 1)), Xb, d, N_MAX, yb, x_stride=d * N_MAX, y_stride=N_MAX, n_each=sizes)
    assert rc == nat.OK and not info.any(), nat.last_error()
    try:
        _, fs0, vf0 = G.call_latent(h, 2, xs, G.NS)
        _, p0 = G.call_class(h, 2, xs, G.NS)
        counts, ld = (20, G.NS), G.NS + 3
        xs2 = np.tile(xs, (2, 1))
        rc, fs, vf = G.call_latent(h, 2, xs2, G.NS, xs_stride=d * G.NS, ns_each=counts, ld_out=ld)
        assert rc == nat.OK, nat.last_error()
        rc, p = G.call_class(h, 2, xs2, G.NS, xs_stride=d * G.NS, ns_each=counts, ld_out=ld)
        assert rc == nat.OK, nat.last_error()
        for b, k in enumerate(counts):
            for got, want in ((fs, fs0), (vf, vf0), (p, p0)):
                assert np.array_equal(got[b, :k], want[b, :k]) and (got[b, k:] == -7.0).all()
        rc, pw = G.call_class(h, 2, xs, G.NS, ld_out=ld)                   # a pitch beyond ns_max, no counts
        assert rc == nat.OK and np.array_equal(pw[:, :G.NS], p0) and (pw[:, G.NS:] == -7.0).all()
        rc, fs1, none = G.call_latent(h, 2, xs, G.NS, var=False)           # either output may be NULL
        assert rc == nat.OK and none is None and np.array_equal(fs1, fs0)
        rc, none, vf1 = G.call_latent(h, 2, xs, G.NS, mean=False)
        assert rc == nat.OK and none is None and np.array_equal(vf1, vf0)
        assert G.call_latent(h, 2, xs, G.NS, mean=False, var=False)[0] == nat.ERR_ARG
        assert nat.lib().gprc_gpc_batch_predict_class(h, xs.ctypes.data, G.NS, 0, None, None, G.NS) == nat.ERR_ARG
    finally:
        G.free(h)


def test_handles_of_the_wrong_kind_are_refused_both_ways():
    name, theta, X, y, Xs = G.case_data("sqrexp")
    d, n, xs = X.shape[0], 16, G.flat(Xs)
    Xn, yn = G.flat(X[:, :n]), y[:n].copy()
    rc, hc, _, _, _ = G.call_fit(name, theta, Xn, d, n, yn)
    assert rc == nat.OK, nat.last_error()
    rc, hr, _, _ = P.call_fit(name, theta, [0.1], Xn, d, n, yn)
    assert rc == nat.OK, nat.last_error()
    lib = nat.lib()
    out = np.full((4, max(d * G.NS, n)), -7.0)
    o = [r.ctypes.data for r in out]
    try:
        assert P.call_predict(hc, 1, xs, G.NS)[0] == nat.ERR_ARG and "classifier batch" in nat.last_error()
        assert lib.gprc_gpr_batch_predict_grad(hc, xs.ctypes.data, G.NS, 0, None, o[0], o[1], G.NS, o[2], o[3], d * G.NS) == nat.ERR_ARG
        assert lib.gprc_gpr_batch_loo(hc, o[0], o[1], o[2], n, None) == nat.ERR_ARG
        assert lib.gprc_gpr_batch_get_alpha(hc, o[0]) == nat.ERR_ARG
        assert G.call_latent(hr, 1, xs, G.NS)[0] == nat.ERR_ARG and "regression batch" in nat.last_error()
        assert G.call_class(hr, 1, xs, G.NS)[0] == nat.ERR_ARG
        assert lib.gprc_gpc_batch_get_f_hat(hr, o[0]) == nat.ERR_ARG
        assert (out == -7.0).all()
        for h in (hc, hr):                                                  # what serves both kinds
            dims = [C.c_int64() for _ in range(3)]
            assert lib.gprc_batch_model_dims(h, *[C.byref(v) for v in dims]) == nat.OK and [v.value for v in dims] == [1, d, n]
        assert P.call_predict(hr, 1, xs, G.NS)[0] == nat.OK and G.call_latent(hc, 1, xs, G.NS)[0] == nat.OK
    finally:
        G.free(hc)
        P.free(hr)


def test_a_classifier_batch_outlives_its_context():
    name, theta, X, y, Xs = G.case_data("sqrexp")
    d, n = X.shape[0], 16
    own = nat.Context(0)
    rc, h, logq, _, info = G.call_fit(name, theta, G.flat(X[:, :n]), d, n, y[:n].copy(), ctx=own)
    assert rc == nat.OK and not info.any() and np.isfinite(logq).all(), nat.last_error()
    assert G.call_latent(h, 1, G.flat(Xs), G.NS)[0] == nat.OK
    own.close()
    assert G.call_latent(h, 1, G.flat(Xs), G.NS)[0] == nat.ERR_ARG and nat.last_error() == "gpc_batch_predict_latent: the model's context has been destroyed"
    assert G.call_class(h, 1, G.flat(Xs), G.NS)[0] == nat.ERR_ARG
    out = np.zeros((1, n))
    assert nat.lib().gprc_gpc_batch_get_f_hat(h, out.ctypes.data) == nat.ERR_ARG
    assert nat.lib().gprc_batch_model_free(h) == nat.OK
    with nat.Context(0) as fresh:
        rc, h2, logq2, _, _ = G.call_fit(name, theta, G.flat(X[:, :n]), d, n, y[:n].copy(), ctx=fresh)
        assert rc == nat.OK and logq2[0] == logq[0]
        G.free(h2)


def test_batchgpc_round_trip():
    case = "matern52_ard8"
    name, theta, X, y, Xs = G.case_data(case)
    full = seven(case)
    sizes = (17, 128, 2)
    with BatchGPC([X[:, :nb] for nb in sizes], [y[:nb] for nb in sizes], name, np.tile(theta, (3, 1)), epsilon=G.EPS) as bg:
        assert not bg.info.any()
        f_hat = bg.f_hat
        fs, vf = bg.predict_latent(Xs)
        prob = bg.predict_class(Xs)
        sets = [Xs[:, :5], Xs, Xs[:, 30:]]
        fl, vl = bg.predict_latent(sets)
        pl = bg.predict_class(sets)
        assert bg.predict_latent(Xs, var=False)[1] is None
        for k, nb in enumerate(sizes):
            b = G.SIZES.index(nb)
            assert bg.logq[k] == full[0][b] and bg.iters[k] == full[1][b]
            assert np.array_equal(f_hat[k, :nb], full[3][b, :nb]) and not f_hat[k, nb:].any()
            assert np.array_equal(fs[k], full[4][b]) and np.array_equal(vf[k], full[5][b]) and np.array_equal(prob[k], full[6][b])
        assert np.array_equal(fl[0], fs[0, :5]) and np.array_equal(vl[1], vf[1]) and np.array_equal(pl[2], prob[2, 30:])
        assert [len(v) for v in pl] == [5, G.NS, G.NS - 30]
    with pytest.raises(nat.GprcError):
        bg.predict_class(Xs)                                               # closed
    with pytest.raises(ValueError):
        BatchGPC(X[:, :129], y[:129], name, theta)
