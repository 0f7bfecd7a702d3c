"""Leave-one-out cross-validation of a fitted batch of small GPs on the device: gprc_gpr_batch_loo against loo_ref.loo, against
models refitted without each point, its bit contract, unequal sizes and a flagged model, the argument errors, and BatchGPR.loo.  Every
model is at most 128 points; the references of batch_predict_grad_ref are computed once per grid entry and shared."""
import numpy as np
import pytest

import batch_predict_grad_ref as Q
import batch_predict_ref as P
import batch_ref as R
from conftest import TOL, nerr
from gprc_amd import BatchGPR
from gprc_amd import _native as nat
from gpu_calls import grad_problem, step_time_limit  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu


# ---- 8. against the closed form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,n", R.GRID, ids=R.GRID_IDS)
def test_batch_loo_against_the_closed_form(case, n):
    """the four measures of tests/test_batch_predict_grad_cpu.py: the mean relative to max |y|, the variance per component relative to
    itself, logdens normwise, the score relative"""
    name, X, y, thetas, noises = R.models(case, n)
    rc, h, _, info = P.call_fit(name, thetas, noises, X, X.shape[0], n, y)
    assert rc == nat.OK and not info.any(), nat.last_error()
    try:
        rc, mean, var, dens, score = Q.call_loo(h, 6, n)
        assert rc == nat.OK, nat.last_error()
    finally:
        P.free(h)
    worst = dict(mean=0.0, var=0.0, logdens=0.0, score=0.0)
    for b, ref in enumerate(Q.loo_references(case, n)):
        for k, e in Q.loo_errors(dict(mean=mean[b], var=var[b], ell=dens[b], loo=score[b]), ref, y).items():
            worst[k] = max(worst[k], e)
    print(f"batch loo {case} n={n}: " + " ".join("%s=%.2e" % kv for kv in worst.items()))
    assert all(v <= TOL for v in worst.values()), worst


# ---- 9. against refitted models ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["sqrexp", "gammaexp1", "ard3", "matern52_ard8"])
def test_batch_loo_against_models_refitted_without_each_point(case):
    """n = 17: seventeen models of 16 points, each leaving one point out, in strided data, predict at their own left-out point"""
    n = 17
    name, X, y, thetas, noises = R.models(case, n)
    d = X.shape[0]
    Xb, yb = np.empty((n, d * (n - 1))), np.empty((n, n - 1))
    for i in range(n):
        keep = np.arange(n) != i
        Xb[i] = X[:, keep].ravel(order="F")
        yb[i] = y[keep]
    left_out = np.ascontiguousarray(X.T)                               # model i's one test point: x_i
    for b in (0, 3):
        rc, h, _, info = P.call_fit(name, thetas[b], noises[b:b + 1], X, d, n, y)
        assert rc == nat.OK and info[0] == 0, nat.last_error()
        rc, mean, var, _, _ = Q.call_loo(h, 1, n)
        P.free(h)
        assert rc == nat.OK, nat.last_error()
        rc, h, _, info = P.call_fit(name, np.tile(thetas[b], (n, 1)), np.full(n, noises[b]), Xb, d, n - 1, yb, x_stride=d * (n - 1), y_stride=n - 1)
        assert rc == nat.OK and not info.any(), nat.last_error()
        rc, pm, pv = P.call_predict(h, n, left_out, 1, xs_stride=d)
        P.free(h)
        assert rc == nat.OK, nat.last_error()
        e = (float(np.abs(mean[0] - pm[:, 0]).max() / np.abs(y).max()), P.var_err(var[0], pv[:, 0] + noises[b]))
        print(f"loo vs refits {case} model {b}: mean %.2e var %.2e" % e)
        assert max(e) <= TOL


# ---- 10. bits ------------------------------------------------------------------------------------------------------------------------------
def test_loo_bits_depend_on_the_model_alone_and_the_call_changes_nothing():
    case, n, B = "matern52_ard8", 100, 300
    name, X, y, thetas, noises = R.models(case, n)
    d = X.shape[0]
    xs = P.flat(P.star_points(X))
    rc, h, _, _ = P.call_fit(name, thetas[0], noises[:1], X, d, n, y)
    assert rc == nat.OK, nat.last_error()
    rc, *alone = Q.call_loo(h, 1, n)
    P.free(h)
    assert rc == nat.OK and all(np.isfinite(a).all() for a in alone)
    which = (np.arange(B) + 1) % 6
    which[[0, 255, 256, 299]] = 0
    rc, h, _, info = P.call_fit(name, thetas[which], noises[which], X, d, n, y)
    assert rc == nat.OK and not info.any()
    try:
        rc, pm, pv = P.call_predict(h, B, xs, P.NS)
        assert rc == nat.OK
        rc, *first = Q.call_loo(h, B, n)
        assert rc == nat.OK, nat.last_error()
        rc, *second = Q.call_loo(h, B, n)
        assert rc == nat.OK, nat.last_error()
        rc, _, _, _, score_only = Q.call_loo(h, B, n, mean=False, var=False, dens=False)
        assert rc == nat.OK, nat.last_error()
        rc, wide, _, _, none = Q.call_loo(h, B, n, var=False, dens=False, score=False, ld_out=n + 3)
        assert rc == nat.OK and none is None, nat.last_error()
        rc, pm2, pv2 = P.call_predict(h, B, xs, P.NS)
        assert rc == nat.OK
    finally:
        P.free(h)
    for p in (0, 255, 256, 299):
        assert all(np.array_equal(a[p], o[0]) for a, o in zip(first, alone)), p
    assert all(np.array_equal(a, b) for a, b in zip(first, second)) and np.array_equal(score_only, first[3])
    assert np.array_equal(wide[:, :n], first[0]) and np.array_equal(wide[:, n:], np.full((B, 3), -7.0))
    assert len(set(first[3][1:7])) == 6                                              # six different models, six different scores
    assert np.array_equal(pm, pm2) and np.array_equal(pv, pv2)                       # the predict after the LOO is unchanged


def test_unequal_sizes_a_flagged_model_and_device_outputs():
    torch = pytest.importorskip("torch")
    sizes, n_max, d = (1, 16, 17, 100, 128), 128, 3
    data = [grad_problem(m, d) for m in sizes]
    th = np.array([ell for _, _, ell in data])
    Xb, yb = np.zeros((5, d * n_max)), np.zeros((5, n_max))
    for b, (Xm, ym, _) in enumerate(data):
        Xb[b, :Xm.size] = Xm.ravel(order="F")
        yb[b, :ym.size] = ym
    nz = np.full(5, 0.05)
    rc, h, _, info = P.call_fit("sqrexp_ard", th, nz, Xb, d, n_max, yb, x_stride=d * n_max, y_stride=n_max, n_each=sizes)
    assert rc == nat.OK and not info.any(), nat.last_error()
    yb_copy = yb.copy()
    yb[:] = np.nan                                                   # the object keeps its own copy of y
    try:
        rc, *good = Q.call_loo(h, 5, n_max)
        assert rc == nat.OK, nat.last_error()
        dev = [torch.full((5, n_max), -7.0, dtype=torch.float64, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        score = np.full(5, -7.0)
        assert nat.lib().gprc_gpr_batch_loo(h, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), n_max, score.ctypes.data) == nat.OK
    finally:
        P.free(h)
    assert all(np.array_equal(t.cpu().numpy(), a) for t, a in zip(dev, good)) and np.array_equal(score, good[3])
    for b, ((Xm, ym, ell), m) in enumerate(zip(data, sizes)):
        ref = Q.loo_ref.loo("sqrexp_ard", ell, Xm, ym, 0.05)
        e = Q.loo_errors(dict(mean=good[0][b, :m], var=good[1][b, :m], ell=good[2][b, :m], loo=good[3][b]), ref, ym)
        print(f"unequal n={m}: " + " ".join("%s=%.2e" % kv for kv in e.items()))
        assert max(e.values()) <= TOL
        assert all(np.array_equal(a[b, m:], np.full(n_max - m, -7.0)) for a in good[:3])          # behind n_b: left as it was
    # model 1's first two points are one point and it has no noise: flagged, NaN; the others keep their bits
    Xb[1, d:2 * d] = Xb[1, :d]
    nz[1] = 0.0
    rc, h, _, info = P.call_fit("sqrexp_ard", th, nz, Xb, d, n_max, yb_copy, x_stride=d * n_max, y_stride=n_max, n_each=sizes)
    assert rc == nat.OK and list(info) == [0, 2, 0, 0, 0]
    try:
        rc, *bad = Q.call_loo(h, 5, n_max)
        assert rc == nat.OK, nat.last_error()
    finally:
        P.free(h)
    assert all(np.isnan(a[1, :16]).all() and np.array_equal(a[1, 16:], np.full(n_max - 16, -7.0)) for a in bad[:3]) and np.isnan(bad[3][1])
    for b in (0, 2, 3, 4):
        assert all(np.array_equal(a[b], g[b]) for a, g in zip(bad, good))


def test_argument_errors_and_batchgpr_loo():
    d, n = 3, 20
    X, y, ell = grad_problem(n, d)
    X = np.asfortranarray(X)
    thetas, noises = np.tile(ell, (2, 1)), np.array([0.1, 0.2])

    def err(rc, word):
        assert rc == nat.ERR_ARG
        assert word in nat.last_error(), nat.last_error()

    rc, h, _, _ = P.call_fit("sqrexp_ard", thetas, noises, X, d, n, y)
    assert rc == nat.OK
    err(nat.lib().gprc_gpr_batch_loo(None, None, None, None, n, np.empty(2).ctypes.data), "null model")
    err(Q.call_loo(h, 2, n, mean=False, var=False, dens=False, score=False)[0], "not all four")
    err(Q.call_loo(h, 2, n, ld_out=n - 1)[0], "ld_out")
    rc, mean, var, dens, score = Q.call_loo(h, 2, n)
    assert rc == nat.OK, nat.last_error()
    P.free(h)
    ctx = nat.Context()
    rc, h, _, _ = P.call_fit("sqrexp_ard", thetas, noises, X, d, n, y, ctx=ctx)
    assert rc == nat.OK
    ctx.close()
    err(Q.call_loo(h, 2, n)[0], "context")
    P.free(h)
    with BatchGPR([X, X[:, :9]], [y, y[:9]], noises, "sqrexp_ard", thetas) as g:
        lm, lv, ld = g.loo()
        sc = g.loo_score
    assert np.array_equal(lm[0], mean[0]) and np.array_equal(lv[0], var[0]) and np.array_equal(ld[0], dens[0]) and sc[0] == score[0]
    assert np.isfinite(lm[1, :9]).all() and np.isnan(lm[1, 9:]).all() and np.isnan(lv[1, 9:]).all() and np.isnan(ld[1, 9:]).all()
    assert nerr([sc[1]], [np.sum(ld[1, :9])]) <= 1e-14
