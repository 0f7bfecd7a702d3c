"""Prediction gradients of a fitted batch of small GPs on the device: gprc_gpr_batch_predict_grad against the float64 closed form and
against the single-model entry points, the conventions at a training point and far away, the bit contract (mean and variance are
gprc_gpr_batch_predict's; a point's gradient bits depend on its model and its coordinates alone), a model that is not positive definite
among good ones, the argument errors, and BatchGPR.predict_grad against central differences.  Every model is at most 128 points; the
references of batch_predict_grad_ref are computed once per grid entry and shared."""
import ctypes as C

import numpy as np
import pytest

import batch_predict_grad_ref as Q
import batch_predict_ref as P
import batch_ref as R
from conftest import TOL, nerr
from gprc_amd import BatchGPR
from gprc_amd import _native as nat
from gprc_amd.fit import grad_dict
from gpu_calls import grad_problem, step_time_limit  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu


def fitted(case, n):
    """the six models of a grid entry as one fitted batch: the handle"""
    name, X, y, thetas, noises = R.models(case, n)
    rc, h, _, info = P.call_fit(name, thetas, noises, X, X.shape[0], n, y)
    assert rc == nat.OK and not info.any(), nat.last_error()
    return h


# ---- 1. against the closed form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,n", R.GRID, ids=R.GRID_IDS)
def test_batch_predict_grad_against_the_closed_form(case, n):
    """37 test points (batch_predict_grad_ref.grid_points); dmean and dvar normwise per model over the d x 37 block, the mean normwise
    and the variance per component relative to itself, as tests/test_gpu_batch_predict.py checks them."""
    d = R.models(case, n)[1].shape[0]
    h = fitted(case, n)
    try:
        rc, mean, var, dm, dv = Q.call_predict_grad(h, 6, P.flat(Q.grid_points(case, n)), Q.NS, d)
        assert rc == nat.OK, nat.last_error()
    finally:
        P.free(h)
    worst = dict(mean=0.0, var=0.0, dmean=0.0, dvar=0.0)
    for b, (want_m, want_v, want_dm, want_dv) in enumerate(Q.grad_references(case, n)):
        worst["mean"] = max(worst["mean"], nerr(mean[b], want_m))
        worst["var"] = max(worst["var"], P.var_err(var[b], want_v))
        worst["dmean"] = max(worst["dmean"], nerr(Q.by_coordinate(dm[b], d, Q.NS), want_dm))
        worst["dvar"] = max(worst["dvar"], nerr(Q.by_coordinate(dv[b], d, Q.NS), want_dv))
    print(f"batch predict_grad {case} n={n}: " + " ".join("%s=%.2e" % kv for kv in worst.items()))
    assert all(v <= TOL for v in worst.values()), worst


# ---- 2. against the single-model entry points -------------------------------------------------------------------------------------------
def single_model(name, theta, X, y, noise, Xs):
    """gprc_gpr_fit + gprc_gpr_predict_grad, the raw calls: (mean, var, dmean[d, ns], dvar[d, ns])"""
    lib, ctx = nat.lib(), nat.default_context()
    _, pp, npar = nat.params_array(theta)
    X, Xs = np.asfortranarray(X), np.asfortranarray(Xs)
    d, n = X.shape
    ns = Xs.shape[1]
    m = C.c_void_p()
    nat.check(lib.gprc_gpr_fit(ctx.handle, grad_dict[name].kernel_id, pp, npar, X.ctypes.data, d, n, np.ascontiguousarray(y).ctypes.data, float(noise),
                               C.byref(m)))
    try:
        mean, var = np.empty(ns), np.empty(ns)
        dm, dv = np.empty((d, ns), order="F"), np.empty((d, ns), order="F")
        nat.check(lib.gprc_gpr_predict_grad(m, Xs.ctypes.data, ns, mean.ctypes.data, var.ctypes.data, dm.ctypes.data, dv.ctypes.data))
    finally:
        lib.gprc_model_free(m)
    return mean, var, dm, dv


@pytest.mark.parametrize("case,n", [("sqrexp", 1), ("gammaexp1.5", 17), ("ratquad", 127), ("ard33", 128), ("matern32", 16), ("matern52_ard17", 100)])
def test_batch_predict_grad_against_the_single_model_entry_points(case, n):
    name, X, y, thetas, noises = R.models(case, n)
    d = X.shape[0]
    Xs = Q.grid_points(case, n) if n in R.GRID_SIZES else P.star_points(X)
    h = fitted(case, n)
    try:
        rc, _, _, dm, dv = Q.call_predict_grad(h, 6, P.flat(Xs), Q.NS, d)
        assert rc == nat.OK, nat.last_error()
    finally:
        P.free(h)
    worst = dict(dmean=0.0, dvar=0.0)
    for b in range(6):
        _, _, want_dm, want_dv = single_model(name, thetas[b], X, y, noises[b], Xs)
        worst["dmean"] = max(worst["dmean"], nerr(Q.by_coordinate(dm[b], d, Q.NS), want_dm))
        worst["dvar"] = max(worst["dvar"], nerr(Q.by_coordinate(dv[b], d, Q.NS), want_dv))
    print(f"batch predict_grad vs gpr_fit + gpr_predict_grad {case} n={n}: " + " ".join("%s=%.2e" % kv for kv in worst.items()))
    assert all(v <= TOL for v in worst.values()), worst


# ---- 3. conventions ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["gammaexp1", "matern32", "matern52_ard8"])
def test_a_test_point_equal_to_a_training_point(case):
    """gammaexp with gamma = 1 has a kink at r = 0: that pair contributes 0 (the convention of gprc_gpr_predict_grad, which the
    reference shares) and the result is finite; the Matern weights are finite there and the difference is an exact 0"""
    n = 17
    name, X, y, thetas, noises = R.models(case, n)
    d = X.shape[0]
    h = fitted(case, n)
    try:
        rc, _, _, dm, dv = Q.call_predict_grad(h, 6, P.flat(X[:, :5]), 5, d)
        assert rc == nat.OK, nat.last_error()
    finally:
        P.free(h)
    assert np.isfinite(dm).all() and np.isfinite(dv).all()
    for b in range(6):
        _, _, want_dm, want_dv = Q.G.predict_grad(name, thetas[b], X, y, noises[b], X[:, :5])
        assert nerr(Q.by_coordinate(dm[b], d, 5), want_dm) <= TOL and nerr(Q.by_coordinate(dv[b], d, 5), want_dv) <= TOL


@pytest.mark.parametrize("n", [17, 128])
def test_far_points_of_sqrexp_have_gradients_that_are_exactly_zero(n):
    """50 box-widths away exp(-s / (2 l^2)) is 0 in float64: every weight is 0 and both gradients are exactly 0"""
    d = R.models("sqrexp", n)[1].shape[0]
    h = fitted("sqrexp", n)
    try:
        rc, _, _, dm, dv = Q.call_predict_grad(h, 6, P.flat(P.grid_points("sqrexp", n)), P.NS, d)
        assert rc == nat.OK, nat.last_error()
    finally:
        P.free(h)
    assert not dm[:, -3 * d:].any() and not dv[:, -3 * d:].any()
    assert dm[:, :-3 * d].any(axis=1).all() and dv[:, :-3 * d].any(axis=1).all()


# ---- 4. the bit contract -------------------------------------------------------------------------------------------------------------------
def test_mean_and_variance_are_batch_predict_s_and_a_points_gradient_bits_are_its_own():
    """T = 16 test points a wave, eight waves a workgroup: 128 points a turn.  384 points = 24 tiles = 3 turns: in a batch of 1 the
    host splits them over 3 workgroups, in the batch of 300 the split is 1 and every workgroup loops over its 3 turns."""
    torch = pytest.importorskip("torch")
    case, n, B, places = "matern52_ard8", 100, 300, (0, 255, 256, 299)
    T, NL = P.TILE, 3 * P.TURN
    name, X, y, thetas, noises = R.models(case, n)
    d = X.shape[0]
    xs = P.flat(P.star_points(X, ns=NL))                 # inside the box, five training points, three far points
    lib = nat.lib()
    subsets = [s for s in np.ndindex(2, 2, 2, 2) if any(s)]

    # every model alone (B = 1), all points together: the bits everything below must reproduce
    base = []
    for m in range(3):
        rc, h, _, info = P.call_fit(name, thetas[m], noises[m:m + 1], X, d, n, y)
        assert rc == nat.OK and info[0] == 0
        rc, pm, pv = P.call_predict(h, 1, xs, NL)
        assert rc == nat.OK, nat.last_error()
        rc, mean, var, dm, dv = Q.call_predict_grad(h, 1, xs, NL, d)
        assert rc == nat.OK, nat.last_error()
        assert np.array_equal(mean, pm) and np.array_equal(var, pv)
        base.append((mean[0].copy(), var[0].copy(), dm[0].copy(), dv[0].copy()))
        if m == 0:
            for s in subsets:                            # every non-empty subset of the four outputs
                rc, *out = Q.call_predict_grad(h, 1, xs, NL, d, mean=s[0], var=s[1], dmean=s[2], dvar=s[3])
                assert rc == nat.OK, nat.last_error()
                for want, got, asked in zip(base[0], out, s):
                    assert (got is None and not asked) or np.array_equal(got[0], want), s
            for j in (0, 1, 17, NL - 9, NL - 8, NL - 1):  # a point on its own (inside, a training point, far away)
                rc, _, _, d1, v1 = Q.call_predict_grad(h, 1, xs[j * d:(j + 1) * d].copy(), 1, d)
                assert rc == nat.OK and np.array_equal(d1[0], dm[0, j * d:(j + 1) * d]) and np.array_equal(v1[0], dv[0, j * d:(j + 1) * d]), j
            for ns in (T - 1, T, T + 1, 3 * T + 5):      # around the tile width
                rc, _, _, dp, vp = Q.call_predict_grad(h, 1, xs, ns, d)
                assert rc == nat.OK and np.array_equal(dp[0], dm[0, :d * ns]) and np.array_equal(vp[0], dv[0, :d * ns])
            rc, mp, _, dp, _ = Q.call_predict_grad(h, 1, xs, NL, d, ld_out=NL + 3, ld_grad=d * NL + 5)   # wider pitches
            assert rc == nat.OK and np.array_equal(dp[0, :d * NL], dm[0]) and np.array_equal(dp[0, d * NL:], np.full(5, -7.0))
            assert np.array_equal(mp[0, :NL], mean[0]) and np.array_equal(mp[0, NL:], np.full(3, -7.0))
        P.free(h)
    assert len({b[2][0] for b in base}) == 3 and np.isfinite(np.concatenate([np.concatenate(b) for b in base])).all()

    xs_rep = np.ascontiguousarray(np.tile(xs, (B, 1)))
    xs_dev, xs_rep_dev = torch.from_numpy(xs).cuda(), torch.from_numpy(xs_rep).cuda()
    torch.cuda.synchronize()
    which = (np.arange(B) + 1) % 3                        # the neighbours: the other models, in turn
    which[list(places)] = 0
    rc, h, _, info = P.call_fit(name, thetas[which], noises[which], X, d, n, y)
    assert rc == nat.OK and not info.any()

    def same(out, counts=None):
        for p in range(B):
            for got, want, w in zip(out, base[which[p]], (1, 1, d, d)):
                k = w * (NL if counts is None else counts[p])
                assert got is None or (np.array_equal(got[p, :k], want[:k]) and np.array_equal(got[p, k:], np.full(got.shape[1] - k, -7.0))), p

    try:
        for Xa, stride in ((xs, 0), (xs_rep, d * NL), (xs_dev, 0), (xs_rep_dev, d * NL)):    # shared / strided, host / device
            rc, *out = Q.call_predict_grad(h, B, Xa, NL, d, xs_stride=stride)
            assert rc == nat.OK, nat.last_error()
            same(out)
        counts = 1 + (np.arange(B) * 37) % NL              # unequal test sets: what lies behind a count comes back untouched
        counts[list(places)] = (NL, 1, 17, NL - 1)
        rc, *out = Q.call_predict_grad(h, B, xs_rep, NL, d, xs_stride=d * NL, ns_each=counts, ld_grad=d * NL + 2)
        assert rc == nat.OK, nat.last_error()
        same(out, counts)
        rc, *out = Q.call_predict_grad(h, B, xs, NL, d, mean=False, var=False, dvar=False)     # the mean's gradient alone
        assert rc == nat.OK, nat.last_error()
        same(out)
        dev = [torch.full((B, w * NL), -7.0, dtype=torch.float64, device="cuda") for w in (1, 1, d, d)]   # device outputs
        torch.cuda.synchronize()
        rc = lib.gprc_gpr_batch_predict_grad(h, xs_dev.data_ptr(), NL, 0, None, dev[0].data_ptr(), dev[1].data_ptr(), NL, dev[2].data_ptr(), dev[3].data_ptr(),
                                             d * NL)
        assert rc == nat.OK, nat.last_error()
        same([t.cpu().numpy() for t in dev])
    finally:
        P.free(h)


# ---- 5. a model that is not positive definite among good ones ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["sqrexp", "gammaexp1.5", "ard3", "matern52_ard8"])
def test_a_bad_model_gets_nan_and_the_others_keep_their_bits(case):
    n, B = 40, 5
    name, X, y, thetas, noises = R.models(case, n)
    d = X.shape[0]
    xs = P.flat(P.star_points(X))
    Xb = np.ascontiguousarray(np.tile(X.ravel(order="F"), (B, 1)))
    noises = noises[:B].copy()
    alone = []
    for b in range(B):
        rc, h, _, info = P.call_fit(name, thetas[b], noises[b:b + 1], X, d, n, y)
        assert rc == nat.OK and info[0] == 0
        rc, *out = Q.call_predict_grad(h, 1, xs, P.NS, d)
        P.free(h)
        assert rc == nat.OK
        alone.append([o[0] for o in out])
    Xb[2, d:2 * d] = Xb[2, :d]                                    # model 2: its first two points are one point, no noise:
    noises[2] = 0.0                                               # the second pivot is 1 - 1 * 1 = 0
    rc, h, lp, info = P.call_fit(name, thetas[:B], noises, Xb, d, n, y, x_stride=d * n)
    assert rc == nat.OK, nat.last_error()
    try:
        rc, *out = Q.call_predict_grad(h, B, xs, P.NS, d)
        assert rc == nat.OK, nat.last_error()
        rc, _, _, dm_only, _ = Q.call_predict_grad(h, B, xs, P.NS, d, mean=False, var=False, dvar=False)
        assert rc == nat.OK, nat.last_error()
    finally:
        P.free(h)
    assert list(info) == [0, 0, 2, 0, 0]
    assert all(np.isnan(o[2]).all() for o in out) and np.isnan(dm_only[2]).all()
    for b in (0, 1, 3, 4):
        assert all(np.array_equal(o[b], a) for o, a in zip(out, alone[b])) and np.array_equal(dm_only[b], alone[b][2])


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    d, n, ns = 3, 20, 7
    X, y, ell = grad_problem(n, d)
    X = np.asfortranarray(X)
    thetas, noises = np.tile(ell, (2, 1)), np.array([0.1, 0.2])
    xs = P.flat(P.star_points(X, ns=ns + 5)[:, :ns])
    lib = nat.lib()

    def err(rc, word):
        assert rc == nat.ERR_ARG
        assert word in nat.last_error(), nat.last_error()

    rc, h, _, info = P.call_fit("sqrexp_ard", thetas, noises, X, d, n, y)
    assert rc == nat.OK and not info.any()
    buf = np.empty(2 * d * ns)
    err(lib.gprc_gpr_batch_predict_grad(None, xs.ctypes.data, ns, 0, None, None, None, ns, buf.ctypes.data, None, d * ns), "null model")
    err(Q.call_predict_grad(h, 2, None, ns, d)[0], "X_star")
    err(Q.call_predict_grad(h, 2, xs, ns, d, mean=False, var=False, dmean=False, dvar=False)[0], "not all four")
    err(Q.call_predict_grad(h, 2, xs, 0, d)[0], "ns_max")
    err(Q.call_predict_grad(h, 2, xs, ns, d, ns_each=[0, ns])[0], "ns_each")
    err(Q.call_predict_grad(h, 2, xs, ns, d, ns_each=[ns, ns + 1])[0], "ns_each")
    err(Q.call_predict_grad(h, 2, xs, ns, d, xs_stride=d * ns - 1)[0], "xs_stride")
    err(Q.call_predict_grad(h, 2, xs, ns, d, xs_stride=-1)[0], "xs_stride")
    err(Q.call_predict_grad(h, 2, xs, ns, d, ld_out=ns - 1)[0], "ld_out")
    err(Q.call_predict_grad(h, 2, xs, ns, d, ld_grad=d * ns - 1)[0], "ld_grad")
    rc, mean, var, dm, dv = Q.call_predict_grad(h, 2, xs, ns, d)     # and the same arguments, as they should be, work
    assert rc == nat.OK and all(np.isfinite(o).all() for o in (mean, var, dm, dv))
    P.free(h)
    # a model whose context has been closed
    ctx = nat.Context()
    rc, h, _, _ = P.call_fit("sqrexp_ard", thetas, noises, X, d, n, y, ctx=ctx)
    assert rc == nat.OK
    ctx.close()
    err(Q.call_predict_grad(h, 2, xs, ns, d)[0], "context")
    P.free(h)


# ---- 7. BatchGPR.predict_grad against central differences -----------------------------------------------------------------------------------
def test_batchgpr_predict_grad_against_central_differences():
    """a check of signs and layout, not of accuracy: differences of BatchGPR.predict with step 1e-5 at interior points, 1e-6 normwise"""
    name, d, sizes, stars, noise, step = "matern52_ard", 3, (9, 128, 40), (6, 3, 20), 0.05, 1e-5
    data = [grad_problem(n, d) for n in sizes]
    thetas = np.array([ell for _, _, ell in data])
    pts = [P.star_points(X, ns=m + 8)[:, :m] for (X, _, _), m in zip(data, stars)]     # points inside the box
    with BatchGPR([X for X, _, _ in data], [y for _, y, _ in data], noise, name, thetas) as g:
        mean, var, dmean, dvar = g.predict_grad(pts)
        pm, pv = g.predict(pts)
        mean_only, none_v, dmean_only, none_dv = g.predict_grad(pts, var=False)
        shared = g.predict_grad(pts[0])
        num_m, num_v = [np.empty((d, m)) for m in stars], [np.empty((d, m)) for m in stars]
        for c in range(d):
            e = np.zeros((d, 1))
            e[c] = step
            (mp, vp), (mm, vm) = g.predict([S + e for S in pts]), g.predict([S - e for S in pts])
            for b in range(3):
                num_m[b][c] = (mp[b] - mm[b]) / (2 * step)
                num_v[b][c] = (vp[b] - vm[b]) / (2 * step)
    assert none_v is None and none_dv is None
    assert shared[0].shape == (3, stars[0]) and shared[2].shape == (3, d, stars[0]) and shared[3].shape == (3, d, stars[0])
    assert np.array_equal(shared[2][0], dmean[0]) and np.array_equal(shared[3][0], dvar[0])
    for b in range(3):
        assert np.array_equal(mean[b], pm[b]) and np.array_equal(var[b], pv[b])
        assert np.array_equal(mean_only[b], pm[b]) and np.array_equal(dmean_only[b], dmean[b])
        assert dmean[b].shape == (d, stars[b]) and dvar[b].shape == (d, stars[b])
        e = (nerr(dmean[b], num_m[b]), nerr(dvar[b], num_v[b]))
        print(f"central differences n={sizes[b]}: dmean %.2e dvar %.2e" % e)
        assert max(e) <= 1e-6
