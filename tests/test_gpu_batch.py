"""Small GPs in batches on the device: gprc_gpr_batch_logp_grad against the closed form and against gprc_gpr_logp_grad, its bit
contract, unequal sizes, a model that is not positive definite among good ones, the argument errors, and optimize_multistart.  Every
shape is at most 128 points; the references of batch_ref are computed once per grid entry and shared."""
import importlib
import math
import time

import numpy as np
import pytest

import ard_grad_ref
import batch_ref as R
from conftest import TOL, nerr
from gprc_amd import _native as nat
from gpu_calls import grad_problem, step_time_limit  # noqa: F401  (autouse fixture)

F = importlib.import_module("gprc_amd.fit")   # (the package's attribute `fit` is the function)

pytestmark = pytest.mark.gpu


def batch_of(case, n):
    """the six models of a grid entry through one call: (logp, grad, alpha, info)"""
    name, X, y, thetas, noises = R.models(case, n)
    rc, lp, g, al, info = R.call_batch(name, thetas, noises, X, X.shape[0], n, y)
    assert rc == nat.OK, nat.last_error()
    return lp, g, al, info


# ---- 1. against the closed form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,n", R.GRID, ids=R.GRID_IDS)
def test_batch_against_the_closed_form(case, n):
    lp, g, al, info = batch_of(case, n)
    assert not info.any()
    worst = dict(logp=0.0, grad=0.0, block=0.0, alpha=0.0)
    for b, (want_lp, want_g, want_a) in enumerate(R.references(case, n)):
        worst["logp"] = max(worst["logp"], abs(lp[b] - want_lp) / abs(want_lp))
        worst["grad"] = max(worst["grad"], nerr(g[b], want_g))
        if R.block_also(case):
            worst["block"] = max(worst["block"], nerr(g[b, :-1], want_g[:-1]))
        worst["alpha"] = max(worst["alpha"], nerr(al[b], want_a))
    print(f"batch {case} n={n}: " + " ".join("%s=%.2e" % kv for kv in worst.items()))
    assert all(v <= TOL for v in worst.values()), worst


# ---- 2. against the existing entry point ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,n", R.GRID, ids=R.GRID_IDS)
def test_batch_against_the_single_model_entry_point(case, n):
    name, X, y, thetas, noises = R.models(case, n)
    lp, g, _, _ = batch_of(case, n)
    worst = dict(logp=0.0, grad=0.0)
    for b in range(len(noises)):
        want_lp, want_g = F.logp_grad(X, y, noises[b], name, thetas[b])
        worst["logp"] = max(worst["logp"], abs(lp[b] - want_lp) / abs(want_lp))
        worst["grad"] = max(worst["grad"], nerr(g[b], want_g))
    print(f"batch vs logp_grad {case} n={n}: " + " ".join("%s=%.2e" % kv for kv in worst.items()))
    assert all(v <= TOL for v in worst.values()), worst


# ---- 3. the bit contract ---------------------------------------------------------------------------------------------------------------
def test_a_models_bits_do_not_depend_on_the_batch_around_it():
    t_begin = time.perf_counter()
    torch = pytest.importorskip("torch")
    case, n, B, places = "matern52_ard8", 100, 300, (0, 255, 256, 299)
    name, X, y, thetas, noises = R.models(case, n)
    d = X.shape[0]
    alone = []
    for m in range(6):
        rc, lp, g, al, info = R.call_batch(name, thetas[m], noises[m:m + 1], X, d, n, y)
        assert rc == nat.OK and info[0] == 0
        alone.append((lp[0], g[0], al[0]))
    assert len({a[0] for a in alone}) == 6                       # six different models
    Xrep = np.ascontiguousarray(np.tile(X.ravel(order="F"), (B, 1)))
    yrep = np.ascontiguousarray(np.tile(y, (B, 1)))
    Xdev, ydev, Xrdev, yrdev = (torch.from_numpy(np.ascontiguousarray(a.ravel(order="F") if a is X else a)).cuda() for a in (X, y, Xrep, yrep))
    torch.cuda.synchronize()
    print("bit contract: torch and its device context are up after %.1f s of this test" % (time.perf_counter() - t_begin))
    ctx = nat.default_context()

    def check(m, **kw):
        which = (np.arange(B) + 1 + m) % 6                       # the neighbours: the other models, in turn
        which[list(places)] = m
        rc, lp, g, al, info = R.call_batch(name, thetas[which], noises[which], kw.pop("Xa", X), d, n, kw.pop("ya", y), **kw)
        assert rc == nat.OK and not info.any()
        for p in places:
            assert lp[p] == alone[m][0]
            assert g is None or np.array_equal(g[p], alone[m][1])
            assert al is None or np.array_equal(al[p], alone[m][2])
        for p in range(B):                                       # and every neighbour is its own model's bits
            assert lp[p] == alone[which[p]][0]

    for m in range(6):
        check(m)                                                                             # shared, host
    check(0, Xa=Xrep, ya=yrep, x_stride=d * n, y_stride=n)                                    # strided, host
    check(1, Xa=Xdev, ya=ydev)                                                               # shared, device
    check(2, Xa=Xrdev, ya=yrdev, x_stride=d * n, y_stride=n)                                  # strided, device
    check(3, Xa=Xrep, ya=ydev, x_stride=d * n)                                               # mixed
    check(4, want_grad=False)
    check(5, want_alpha=False)
    check(0, want_grad=False, want_alpha=False)
    check(1)
    check(1)                                                                                 # two calls in a row
    nat.check(nat.lib().gprc_ctx_trim(ctx.handle))
    check(2)                                                                                 # after the pool was emptied


# ---- 4. unequal sizes ------------------------------------------------------------------------------------------------------------------
def test_unequal_sizes_in_one_strided_batch():
    name, d, sizes, noise = "sqrexp_ard", 3, (1, 16, 17, 100, 128), 0.05
    n_max, B = 128, 5
    data = [grad_problem(n, d) for n in sizes]
    thetas = np.array([ell for _, _, ell in data])
    Xb, yb = np.zeros((B, d * n_max)), np.zeros((B, n_max))
    for b, (X, y, _) in enumerate(data):
        Xb[b, :X.size] = X.ravel(order="F")
        yb[b, :y.size] = y
    noises = np.full(B, noise)
    rc, lp, g, al, info = R.call_batch(name, thetas, noises, Xb, d, n_max, yb, x_stride=d * n_max, y_stride=n_max, n_each=sizes)
    assert rc == nat.OK and not info.any()
    for b, (X, y, ell) in enumerate(data):
        want_lp, want_g = ard_grad_ref.logp_grad(name, ell, X, y, noise)
        want_a = ard_grad_ref.gpr_fit(name, ell, X, y, noise)["alpha"]
        e = (abs(lp[b] - want_lp) / abs(want_lp), nerr(g[b], want_g), nerr(g[b, :-1], want_g[:-1]), nerr(al[b, :sizes[b]], want_a))
        print(f"unequal n={sizes[b]}: logp %.2e grad %.2e block %.2e alpha %.2e" % e)
        assert max(e) <= TOL
        assert np.array_equal(al[b, sizes[b]:], np.zeros(n_max - sizes[b]))
    for b, n in enumerate(sizes):                                 # the padding is never read
        Xb[b, d * n:] = np.nan
        yb[b, n:] = np.nan
    rc, lp2, g2, al2, info2 = R.call_batch(name, thetas, noises, Xb, d, n_max, yb, x_stride=d * n_max, y_stride=n_max, n_each=sizes)
    assert rc == nat.OK and not info2.any()
    assert np.array_equal(lp, lp2) and np.array_equal(g, g2) and np.array_equal(al, al2)
    # through fit.logp_grad_batch, which pads the lists itself
    lp3, g3, info3 = F.logp_grad_batch([X for X, _, _ in data], [y for _, y, _ in data], noise, name, thetas)
    assert np.array_equal(lp, lp3) and np.array_equal(g, g3) and not info3.any()


# ---- 5. a model that is not positive definite among good ones ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["sqrexp", "gammaexp1.5", "ratquad", "ard3", "matern32", "matern52_ard8"])
def test_a_bad_model_is_flagged_and_the_others_keep_their_bits(case):
    n, B = 40, 5
    name, X, y, thetas, noises = R.models(case, n)
    d = X.shape[0]
    Xb = np.ascontiguousarray(np.tile(X.ravel(order="F"), (B, 1)))
    noises = noises[:B].copy()
    good = R.call_batch(name, thetas[:B], noises, Xb, d, n, y, x_stride=d * n)
    assert good[0] == nat.OK and not good[4].any()
    Xb[2, d:2 * d] = Xb[2, :d]                                    # model 2: its first two points are one point, no noise:
    noises[2] = 0.0                                               # the second pivot is 1 - 1 * 1 = 0
    rc, lp, g, al, info = R.call_batch(name, thetas[:B], noises, Xb, d, n, y, x_stride=d * n)
    assert rc == nat.OK, nat.last_error()
    assert list(info) == [0, 0, 2, 0, 0]
    assert np.isnan(lp[2]) and np.isnan(g[2]).all() and np.isnan(al[2]).all()
    for b in (0, 1, 3, 4):
        assert lp[b] == good[1][b] and np.array_equal(g[b], good[2][b]) and np.array_equal(al[b], good[3][b])


# ---- 6. argument errors ----------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    d, n = 3, 20
    X, y, ell = grad_problem(n, d)
    X = np.asfortranarray(X)
    thetas, noises = np.tile(ell, (2, 1)), np.array([0.1, 0.2])
    Xbig, ybig = np.zeros((d, 129), order="F"), np.zeros(129)

    def err(rc, word):
        assert rc == nat.ERR_ARG
        assert word in nat.last_error(), nat.last_error()

    err(R.call_batch("sqrexp_ard", thetas, noises, Xbig, d, 129, ybig)[0], "single-model")
    err(R.call_batch("sqrexp_ard", thetas, noises, X, d, n, y, n_each=[0, n])[0], "n_each")
    err(R.call_batch("sqrexp_ard", thetas, noises, X, d, n, y, n_each=[n, n + 1])[0], "n_each")
    err(R.call_batch(nat.LINEAR, thetas, noises, X, d, n, y)[0], "defined for")
    err(R.call_batch("sqrexp_ard", thetas, np.array([0.1, -0.2]), X, d, n, y)[0], "noise")
    err(R.call_batch("sqrexp_ard", thetas, np.array([0.1, np.inf]), X, d, n, y)[0], "noise")
    err(R.call_batch("sqrexp_ard", thetas, noises, X, d, n, y, logp=False)[0], "logp_out")
    err(R.call_batch("sqrexp_ard", thetas, noises, X, d, n, y, info=False)[0], "info_out")
    err(R.call_batch("sqrexp_ard", thetas, noises, X, d, n, y, x_stride=d * n - 1)[0], "x_stride")
    err(R.call_batch("sqrexp_ard", thetas, noises, X, d, n, y, y_stride=n - 1)[0], "y_stride")
    ctx = nat.default_context()
    assert nat.lib().gprc_gpr_batch_logp_grad(ctx.handle, nat.SQREXP_ARD, 0, None, d, d, None, None, d, n, 0, None, 0, None, None, None, None, None) == nat.OK
    rc, lp, g, al, info = R.call_batch("sqrexp_ard", thetas, noises, X, d, n, y)      # and the same arguments, as they should be, work
    assert rc == nat.OK and not info.any() and np.isfinite(lp).all()


# ---- 7. optimize_multistart on the device ------------------------------------------------------------------------------------------------
def test_multistart_on_the_device(monkeypatch):
    name, d, n, noise = "matern52_ard", 3, 120, 0.05
    X, y, _ = grad_problem(n, d)
    # the documented default: the default start, then log-uniform multiples of it in [1/8, 8] from rng
    starts = np.vstack([np.ones(d), np.exp(np.random.default_rng(2024).uniform(math.log(1.0 / 8.0), math.log(8.0), (5, d)))])
    begin, _, info = F.logp_grad_batch(X, y, noise, name, starts)
    assert not info.any()
    calls = []
    real = F.logp_grad_batch
    monkeypatch.setattr(F, "logp_grad_batch", lambda *a, **k: (calls.append(np.atleast_2d(a[4]).shape[0]), real(*a, **k))[1])
    r = F.optimize_multistart(X, y, noise, name, n_starts=6, rng=np.random.default_rng(2024))
    monkeypatch.undo()
    assert len(r["all"]) == 6 and r["best_index"] == int(np.argmax([a["value"] for a in r["all"]]))
    rounds = max(a["counts"][0] for a in r["all"])
    print(f"multistart: {len(calls)} device calls for {sum(calls)} evaluations, the longest instance {rounds} values; from "
          f"{[round(float(v), 3) for v in begin]} to {[round(a['value'], 6) for a in r['all']]}, best {r['best_index']}")
    assert calls[0] == 6 and len(calls) <= rounds              # once per lockstep round, not once per start
    assert sum(calls) > 2 * len(calls)
    for a, v0 in zip(r["all"], begin):
        assert a["value"] >= v0                                # every start ends no lower than it began
        again, _ = F.logp_grad(X, y, a["noise"], name, np.array(a["par"]))
        assert abs(a["value"] - again) <= TOL * abs(again)
    one = F.optimize(X, y, noise, name, np.ones(d))
    print(f"multistart: best {r['value']!r}, optimize from the default start {one['value']!r}")
    assert r["value"] >= one["value"] - 1e-6 * abs(one["value"])
