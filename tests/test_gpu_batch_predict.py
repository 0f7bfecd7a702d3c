"""A fitted batch of small GPs on the device: gprc_gpr_batch_fit + gprc_gpr_batch_predict against the closed form and against the
single-model entry points, the fit's bits against gprc_gpr_batch_logp_grad, the predict's bit contract, unequal sizes, a model that is
not positive definite among good ones, far test points, the argument errors, and BatchGPR.  Every model is at most 128 points; the
references of batch_predict_ref are computed once per grid entry and shared."""
import ctypes as C

import numpy as np
import pytest

import batch_predict_ref as P
import batch_ref as R
from conftest import TOL, nerr
from gprc_amd import BatchGPR
from gprc_amd import _native as nat
from gprc_amd.fit import grad_dict
from gpu_calls import grad_problem, step_time_limit  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu


def fitted(case, n):
    """the six models of a grid entry as one fitted batch: (handle, logp, info)"""
    name, X, y, thetas, noises = R.models(case, n)
    rc, h, lp, info = P.call_fit(name, thetas, noises, X, X.shape[0], n, y)
    assert rc == nat.OK, nat.last_error()
    return h, lp, info


# ---- 1. against the closed form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,n", R.GRID, ids=R.GRID_IDS)
def test_batch_predict_against_the_closed_form(case, n):
    """37 test points of the three kinds (inside the box, training points themselves, 50 box-widths away); mean normwise, variance per
    component relative to the variance itself."""
    h, _, info = fitted(case, n)
    try:
        assert not info.any()
        Xs = P.grid_points(case, n)
        rc, mean, var = P.call_predict(h, 6, P.flat(Xs), P.NS)
        assert rc == nat.OK, nat.last_error()
    finally:
        P.free(h)
    worst = dict(mean=0.0, var=0.0)
    for b, (want_m, want_v) in enumerate(P.references(case, n)):
        worst["mean"] = max(worst["mean"], nerr(mean[b], want_m))
        worst["var"] = max(worst["var"], P.var_err(var[b], want_v))
    print(f"batch predict {case} n={n}: " + " ".join("%s=%.2e" % kv for kv in worst.items()))
    assert all(v <= TOL for v in worst.values()), worst


# ---- 2. against the single-model entry points -------------------------------------------------------------------------------------------
def single_model(name, theta, X, y, noise, Xs):
    """gprc_gpr_fit + gprc_gpr_predict(pointwise = 1), the raw calls: (mean, var)"""
    lib, ctx = nat.lib(), nat.default_context()
    _, pp, npar = nat.params_array(theta)
    X, Xs = np.asfortranarray(X), np.asfortranarray(Xs)
    d, n = X.shape
    m = C.c_void_p()
    nat.check(lib.gprc_gpr_fit(ctx.handle, grad_dict[name].kernel_id, pp, npar, X.ctypes.data, d, n, np.ascontiguousarray(y).ctypes.data, float(noise),
                               C.byref(m)))
    try:
        mean, var = np.empty(Xs.shape[1]), np.empty(Xs.shape[1])
        nat.check(lib.gprc_gpr_predict(m, Xs.ctypes.data, Xs.shape[1], 1, mean.ctypes.data, var.ctypes.data))
    finally:
        lib.gprc_model_free(m)
    return mean, var


@pytest.mark.parametrize("case,n", R.GRID, ids=R.GRID_IDS)
def test_batch_predict_against_the_single_model_entry_points(case, n):
    name, X, y, thetas, noises = R.models(case, n)
    Xs = P.grid_points(case, n)
    h, _, _ = fitted(case, n)
    try:
        rc, mean, var = P.call_predict(h, 6, P.flat(Xs), P.NS)
        assert rc == nat.OK, nat.last_error()
    finally:
        P.free(h)
    worst = dict(mean=0.0, var=0.0)
    for b in range(6):
        want_m, want_v = single_model(name, thetas[b], X, y, noises[b], Xs)
        worst["mean"] = max(worst["mean"], nerr(mean[b], want_m))
        worst["var"] = max(worst["var"], P.var_err(var[b], want_v))
    print(f"batch predict vs gpr_fit + gpr_predict {case} n={n}: " + " ".join("%s=%.2e" % kv for kv in worst.items()))
    assert all(v <= TOL for v in worst.values()), worst


# ---- 3. the fit's bits are gprc_gpr_batch_logp_grad's --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,n", [("sqrexp", 1), ("gammaexp1.5", 17), ("ratquad", 127), ("ard33", 128), ("matern32", 16), ("matern52_ard17", 100)])
def test_fit_bits_are_the_batched_evidence_call_s(case, n):
    name, X, y, thetas, noises = R.models(case, n)
    rc, lp, g, al, info = R.call_batch(name, thetas, noises, X, X.shape[0], n, y)
    assert rc == nat.OK and not info.any()
    h, lp2, info2 = fitted(case, n)
    try:
        al2 = P.get_alpha(h, 6, n)
        dims = [C.c_int64(), C.c_int64(), C.c_int64()]
        nat.check(nat.lib().gprc_batch_model_dims(h, *[C.byref(v) for v in dims]))
    finally:
        P.free(h)
    assert np.array_equal(lp, lp2) and np.array_equal(info, info2) and np.array_equal(al, al2)
    assert [v.value for v in dims] == [6, X.shape[0], n]


def test_fit_bits_across_the_launch_boundary_and_with_unequal_sizes():
    """B = 300 crosses the 256-model launch; models of unequal sizes in strides, one of them not positive definite"""
    case, n, B = "matern52_ard8", 100, 300
    name, X, y, thetas, noises = R.models(case, n)
    d = X.shape[0]
    which = np.arange(B) % 6
    rc, lp, _, al, info = R.call_batch(name, thetas[which], noises[which], X, d, n, y, want_grad=False)
    assert rc == nat.OK and not info.any()
    rc, h, lp2, info2 = P.call_fit(name, thetas[which], noises[which], X, d, n, y)
    assert rc == nat.OK, nat.last_error()
    try:
        al2 = P.get_alpha(h, B, n)
    finally:
        P.free(h)
    assert np.array_equal(lp, lp2) and np.array_equal(info, info2) and np.array_equal(al, al2)
    assert len(set(lp[:6])) == 6 and np.array_equal(lp[256:262], lp[which[256:262]])
    # unequal sizes, strided; model 1's first two points are one point and it has no noise: flagged, NaN, in both calls alike
    sizes, n_max = (1, 16, 17, 100, 128), 128
    data = [grad_problem(m, 3) for m in sizes]
    th = np.array([ell for _, _, ell in data])
    Xb, yb = np.zeros((5, 3 * n_max)), np.zeros((5, n_max))
    for b, (Xm, ym, _) in enumerate(data):
        Xb[b, :Xm.size] = Xm.ravel(order="F")
        yb[b, :ym.size] = ym
    Xb[1, 3:6] = Xb[1, :3]
    nz = np.array([0.05, 0.0, 0.05, 0.05, 0.05])
    rc, lp, _, al, info = R.call_batch("sqrexp_ard", th, nz, Xb, 3, n_max, yb, x_stride=3 * n_max, y_stride=n_max, n_each=sizes, want_grad=False)
    assert rc == nat.OK and list(info) == [0, 2, 0, 0, 0]
    rc, h, lp2, info2 = P.call_fit("sqrexp_ard", th, nz, Xb, 3, n_max, yb, x_stride=3 * n_max, y_stride=n_max, n_each=sizes)
    assert rc == nat.OK, nat.last_error()
    try:
        al2 = P.get_alpha(h, 5, n_max)
    finally:
        P.free(h)
    assert np.array_equal(lp, lp2, equal_nan=True) and np.array_equal(info, info2) and np.array_equal(al, al2, equal_nan=True)
    assert np.isnan(lp2[1]) and np.isnan(al2[1, :16]).all() and not np.isnan(np.delete(lp2, 1)).any()


# ---- 4. the predict's bit contract ---------------------------------------------------------------------------------------------------------
def test_a_test_points_bits_depend_on_its_model_and_its_coordinates_alone():
    """T = 16 test points a wave, eight waves a workgroup: a workgroup takes 128 points a turn.  The long set has 2 * 128 + 5 = 261
    points = 17 tiles = 3 turns.  In a batch of 1 the host splits them over 3 workgroups (split = 3 > 1: 256 CUs / 1 model allows more
    than the 3 turns there are); in the batch of 300 the split is 1 (300 models already exceed the CUs), so every workgroup LOOPS over
    its 3 turns and waves 0 of the third turn run a tile with 5 live columns."""
    torch = pytest.importorskip("torch")
    case, n, B, places = "matern52_ard8", 100, 300, (0, 255, 256, 299)
    T, NL = P.TILE, 2 * P.TURN + 5
    name, X, y, thetas, noises = R.models(case, n)
    d = X.shape[0]
    Xs = P.star_points(X, ns=NL)                       # inside the box, five training points, three far points
    xs = P.flat(Xs)
    ctx = nat.default_context()
    lib = nat.lib()

    # every model alone (B = 1), all points together: the bits everything below must reproduce
    base = []
    for m in range(6):
        rc, h, _, info = P.call_fit(name, thetas[m], noises[m:m + 1], X, d, n, y)
        assert rc == nat.OK and info[0] == 0
        rc, mean, var = P.call_predict(h, 1, xs, NL)
        assert rc == nat.OK, nat.last_error()
        base.append((mean[0].copy(), var[0].copy()))
        if m == 0:
            for j in range(NL):                          # each point on its own
                rc, m1, v1 = P.call_predict(h, 1, xs[j * d:(j + 1) * d].copy(), 1)
                assert rc == nat.OK and m1[0, 0] == mean[0, j] and v1[0, 0] == var[0, j], j
            for ns in (T - 1, T, T + 1, 3 * T + 5):      # around the tile width
                rc, mp, vp = P.call_predict(h, 1, xs, ns)
                assert rc == nat.OK and np.array_equal(mp[0], mean[0, :ns]) and np.array_equal(vp[0], var[0, :ns])
            rc, mo, vo = P.call_predict(h, 1, xs, NL, var=False)               # without var_out
            assert rc == nat.OK and vo is None and np.array_equal(mo[0], mean[0])
            rc, mo, vo = P.call_predict(h, 1, xs, NL, mean=False)              # without mean_out
            assert rc == nat.OK and mo is None and np.array_equal(vo[0], var[0])
            rc, mp, vp = P.call_predict(h, 1, xs, NL, ld_out=NL + 3)            # a wider pitch
            assert rc == nat.OK and np.array_equal(mp[0, :NL], mean[0]) and np.array_equal(mp[0, NL:], np.full(3, -7.0))
        P.free(h)
    assert len({b[0][0] for b in base}) == 6            # six different models
    assert np.isfinite(np.concatenate([np.concatenate(b) for b in base])).all()

    xs_rep = np.ascontiguousarray(np.tile(xs, (B, 1)))
    xs_dev, xs_rep_dev = torch.from_numpy(xs).cuda(), torch.from_numpy(xs_rep).cuda()
    torch.cuda.synchronize()

    def check(m, h, which, **kw):
        dev_out = kw.pop("dev_out", False)
        if dev_out:
            mt, vt = torch.full((B, NL), -7.0, dtype=torch.float64, device="cuda"), torch.full((B, NL), -7.0, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            rc = lib.gprc_gpr_batch_predict(h, nat.ptr(kw["Xa"]), NL, kw.get("xs_stride", 0), None, mt.data_ptr(), vt.data_ptr(), NL)
            assert rc == nat.OK, nat.last_error()
            mean, var = mt.cpu().numpy(), vt.cpu().numpy()
        else:
            rc, mean, var = P.call_predict(h, B, kw.pop("Xa"), NL, **kw)
            assert rc == nat.OK, nat.last_error()
        for p in range(B):                                # the places hold model m, every neighbour is its own model's bits
            assert mean is None or np.array_equal(mean[p], base[which[p]][0]), p
            assert var is None or np.array_equal(var[p], base[which[p]][1]), p

    for m in range(3):
        which = (np.arange(B) + 1 + m) % 6                # the neighbours: the other models, in turn
        which[list(places)] = m
        rc, h, _, info = P.call_fit(name, thetas[which], noises[which], X, d, n, y)
        assert rc == nat.OK and not info.any()
        try:
            check(m, h, which, Xa=xs)                                           # shared, host
            if m == 0:
                check(m, h, which, Xa=xs_rep, xs_stride=d * NL)                 # strided, host
                check(m, h, which, Xa=xs_dev)                                   # shared, device
                check(m, h, which, Xa=xs_rep_dev, xs_stride=d * NL)             # strided, device
                check(m, h, which, Xa=xs_rep_dev, xs_stride=d * NL, dev_out=True)   # ... into device outputs
                check(m, h, which, Xa=xs, var=False)
                check(m, h, which, Xa=xs, mean=False)
                check(m, h, which, Xa=xs)                                       # twice in a row
                nat.check(lib.gprc_ctx_trim(ctx.handle))
                check(m, h, which, Xa=xs)                                       # after the pool was emptied
        finally:
            P.free(h)


# ---- 5. unequal sizes ------------------------------------------------------------------------------------------------------------------
def test_unequal_sizes_and_unequal_test_sets_in_one_strided_call():
    name, d, sizes, stars, noise = "sqrexp_ard", 3, (1, 16, 17, 100, 128), (1, 16, 17, 33, 5), 0.05
    n_max, ns_max, B = 128, 33, 5
    data = [grad_problem(n, d) for n in sizes]
    thetas = np.array([ell for _, _, ell in data])
    pts = [P.star_points(X, ns=m + 3, seed=1)[:, :m] for (X, _, _), m in zip(data, stars)]   # points inside the box, then training points
    Xb, yb, Sb = np.zeros((B, d * n_max)), np.zeros((B, n_max)), np.zeros((B, d * ns_max))
    for b, ((X, y, _), S) in enumerate(zip(data, pts)):
        Xb[b, :X.size] = X.ravel(order="F")
        yb[b, :y.size] = y
        Sb[b, :S.size] = S.ravel(order="F")
    noises = np.full(B, noise)

    def run():
        rc, h, lp, info = P.call_fit(name, thetas, noises, Xb, d, n_max, yb, x_stride=d * n_max, y_stride=n_max, n_each=sizes)
        assert rc == nat.OK and not info.any(), nat.last_error()
        try:
            rc, mean, var = P.call_predict(h, B, Sb, ns_max, xs_stride=d * ns_max, ns_each=stars)
            assert rc == nat.OK, nat.last_error()
        finally:
            P.free(h)
        return lp, mean, var

    lp, mean, var = run()
    for b, ((X, y, ell), S) in enumerate(zip(data, pts)):
        want_m, want_v = P.closed_form(name, ell, X, y, noise, S)
        e = (nerr(mean[b, :stars[b]], want_m), P.var_err(var[b, :stars[b]], want_v))
        print(f"unequal n={sizes[b]} n*={stars[b]}: mean %.2e var %.2e" % e)
        assert max(e) <= TOL
        assert np.array_equal(mean[b, stars[b]:], np.full(ns_max - stars[b], -7.0))      # behind a model's count: left as it was
        assert np.array_equal(var[b, stars[b]:], np.full(ns_max - stars[b], -7.0))
    for b in range(B):                                                # what lies behind a count is never read
        Xb[b, d * sizes[b]:] = np.nan
        yb[b, sizes[b]:] = np.nan
        Sb[b, d * stars[b]:] = np.nan
    lp2, mean2, var2 = run()
    assert np.array_equal(lp, lp2) and np.array_equal(mean, mean2) and np.array_equal(var, var2)


# ---- 6. a model that is not positive definite among good ones ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["sqrexp", "gammaexp1.5", "ratquad", "ard3", "matern32", "matern52_ard8"])
def test_a_bad_model_predicts_nan_and_the_others_keep_their_bits(case):
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
        rc, m1, v1 = P.call_predict(h, 1, xs, P.NS)
        P.free(h)
        assert rc == nat.OK
        alone.append((m1[0], v1[0]))
    Xb[2, d:2 * d] = Xb[2, :d]                                    # model 2: its first two points are one point, no noise:
    noises[2] = 0.0                                               # the second pivot is 1 - 1 * 1 = 0
    rc, h, lp, info = P.call_fit(name, thetas[:B], noises, Xb, d, n, y, x_stride=d * n)
    assert rc == nat.OK, nat.last_error()
    try:
        rc, mean, var = P.call_predict(h, B, xs, P.NS)
        assert rc == nat.OK, nat.last_error()
        rc, mean_only, _ = P.call_predict(h, B, xs, P.NS, var=False)
        assert rc == nat.OK, nat.last_error()
    finally:
        P.free(h)
    assert list(info) == [0, 0, 2, 0, 0] and np.isnan(lp[2])
    assert np.isnan(mean[2]).all() and np.isnan(var[2]).all() and np.isnan(mean_only[2]).all()
    for b in (0, 1, 3, 4):
        assert np.array_equal(mean[b], alone[b][0]) and np.array_equal(var[b], alone[b][1]) and np.array_equal(mean_only[b], alone[b][0])


# ---- 7. far points -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [17, 128])
def test_far_points_of_sqrexp_give_the_prior_exactly(n):
    """50 box-widths away exp(-s / (2 l^2)) is 0 in float64: the mean is exactly 0 and the variance exactly k(x*, x*) = 1"""
    h, _, info = fitted("sqrexp", n)
    try:
        rc, mean, var = P.call_predict(h, 6, P.flat(P.grid_points("sqrexp", n)), P.NS)
        assert rc == nat.OK and not info.any()
    finally:
        P.free(h)
    assert np.array_equal(mean[:, -3:], np.zeros((6, 3))) and np.array_equal(var[:, -3:], np.ones((6, 3)))
    assert (mean[:, :-3] != 0).all() and (var[:, :-3] < 1).all()


# ---- 8. argument errors ----------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    d, n, ns = 3, 20, 7
    X, y, ell = grad_problem(n, d)
    X = np.asfortranarray(X)
    thetas, noises = np.tile(ell, (2, 1)), np.array([0.1, 0.2])
    xs = P.flat(P.star_points(X, ns=ns + 5)[:, :ns])
    Xbig, ybig = np.zeros((d, 129), order="F"), np.zeros(129)
    lib = nat.lib()

    def err(rc, word):
        assert rc == nat.ERR_ARG
        assert word in nat.last_error(), nat.last_error()

    def fit_err(word, *a, **kw):
        rc, h, _, _ = P.call_fit(*a, **kw)
        assert not h.value                                          # no object after an error
        err(rc, word)

    # the fit: gprc_gpr_batch_logp_grad's errors, and the handle
    fit_err("single-model", "sqrexp_ard", thetas, noises, Xbig, d, 129, ybig)
    fit_err("n_each", "sqrexp_ard", thetas, noises, X, d, n, y, n_each=[0, n])
    fit_err("n_each", "sqrexp_ard", thetas, noises, X, d, n, y, n_each=[n, n + 1])
    fit_err("defined for", nat.LINEAR, thetas, noises, X, d, n, y)
    fit_err("noise", "sqrexp_ard", thetas, np.array([0.1, -0.2]), X, d, n, y)
    fit_err("noise", "sqrexp_ard", thetas, np.array([0.1, np.inf]), X, d, n, y)
    fit_err("logp_out", "sqrexp_ard", thetas, noises, X, d, n, y, logp=False)
    fit_err("info_out", "sqrexp_ard", thetas, noises, X, d, n, y, info=False)
    fit_err("model_out", "sqrexp_ard", thetas, noises, X, d, n, y, model=False)
    fit_err("x_stride", "sqrexp_ard", thetas, noises, X, d, n, y, x_stride=d * n - 1)
    fit_err("y_stride", "sqrexp_ard", thetas, noises, X, d, n, y, y_stride=n - 1)
    fit_err("null input", "sqrexp_ard", thetas, noises, None, d, n, y)
    rc, h, lp, info = P.call_fit("sqrexp_ard", thetas, noises, X, d, n, y)
    assert rc == nat.OK and not info.any() and np.isfinite(lp).all()
    rc, h2, _, _ = P.call_fit("sqrexp_ard", thetas, noises, X, d, n, y)
    assert rc == nat.OK
    # the predict
    err(lib.gprc_gpr_batch_predict(None, xs.ctypes.data, ns, 0, None, np.empty(2 * ns).ctypes.data, None, ns), "null model")
    err(P.call_predict(h, 2, None, ns)[0], "X_star")
    err(P.call_predict(h, 2, xs, ns, mean=False, var=False)[0], "not both")
    err(P.call_predict(h, 2, xs, 0)[0], "ns_max")
    err(P.call_predict(h, 2, xs, ns, ns_each=[0, ns])[0], "ns_each")
    err(P.call_predict(h, 2, xs, ns, ns_each=[ns, ns + 1])[0], "ns_each")
    err(P.call_predict(h, 2, xs, ns, xs_stride=d * ns - 1)[0], "xs_stride")
    err(P.call_predict(h, 2, xs, ns, xs_stride=-1)[0], "xs_stride")
    err(P.call_predict(h, 2, xs, ns, ld_out=ns - 1)[0], "ld_out")
    err(lib.gprc_batch_model_dims(None, None, None, None), "null model")
    err(lib.gprc_gpr_batch_get_alpha(h, None), "alpha_out")
    rc, mean, var = P.call_predict(h, 2, xs, ns)                     # and the same arguments, as they should be, work
    assert rc == nat.OK and np.isfinite(mean).all() and np.isfinite(var).all()
    P.free(h)
    assert lib.gprc_batch_model_free(None) == nat.OK
    rc, mean2, var2 = P.call_predict(h2, 2, xs, ns)                  # after the first handle is gone the second still works
    assert rc == nat.OK and np.array_equal(mean, mean2) and np.array_equal(var, var2)
    P.free(h2)
    # no models: no object
    hz = C.c_void_p(1)
    assert lib.gprc_gpr_batch_fit(nat.default_context().handle, nat.SQREXP_ARD, 0, None, d, d, None, None, d, n, 0, None, 0, None, C.byref(hz), None, None) == nat.OK
    assert not hz.value


# ---- 9. BatchGPR ---------------------------------------------------------------------------------------------------------------------------
def test_batchgpr_through_lists_gives_the_raw_call_s_bits():
    name, d, sizes, stars, noise = "matern52_ard", 3, (9, 128, 40), (20, 3, 130), 0.05
    data = [grad_problem(n, d) for n in sizes]
    thetas = np.array([ell for _, _, ell in data])
    pts = [P.star_points(X, ns=m + 8)[:, 2:2 + m] for (X, _, _), m in zip(data, stars)]   # points inside the box, then two training points
    with BatchGPR([X for X, _, _ in data], [y for _, y, _ in data], noise, name, thetas) as g:
        mean, var = g.predict(pts)
        mean_only, none = g.predict(pts, var=False)
        alpha, logp, info = g.alpha, g.logp.copy(), g.info.copy()
        shared_m, shared_v = g.predict(pts[0])
    assert none is None and not info.any() and alpha.shape == (3, 128)
    for b, ((X, y, ell), S) in enumerate(zip(data, pts)):                # every model alone through the raw calls
        rc, h, lp, _ = P.call_fit(name, ell, [noise], np.asfortranarray(X), d, sizes[b], y)
        assert rc == nat.OK, nat.last_error()
        try:
            rc, m1, v1 = P.call_predict(h, 1, P.flat(S), stars[b])
            rc0, m0, v0 = P.call_predict(h, 1, P.flat(pts[0]), stars[0])
            al = P.get_alpha(h, 1, sizes[b])
        finally:
            P.free(h)
        assert rc == nat.OK and rc0 == nat.OK
        assert mean[b].shape == (stars[b],) and np.array_equal(mean[b], m1[0]) and np.array_equal(var[b], v1[0]) and np.array_equal(mean_only[b], m1[0])
        assert np.array_equal(shared_m[b], m0[0]) and np.array_equal(shared_v[b], v0[0])
        assert logp[b] == lp[0] and np.array_equal(alpha[b, :sizes[b]], al[0]) and not alpha[b, sizes[b]:].any()
        want_m, want_v = P.closed_form(name, ell, X, y, noise, S)
        assert nerr(mean[b], want_m) <= TOL and P.var_err(var[b], want_v) <= TOL
