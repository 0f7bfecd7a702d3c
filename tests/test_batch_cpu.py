"""Small GPs in batches, what needs no GPU: the generator form of vmmin driven in lockstep, the multi-start optimiser on a numpy objective,
the numpy model of the batched kernel's algorithm against the closed form, and the padding of unequal data sets."""
import importlib

import numpy as np
import pytest

import ard_grad_ref
import batch_ref as R
from conftest import TOL, nerr
from gprc_amd import _native as nat
from gpu_calls import grad_problem

F = importlib.import_module("gprc_amd.fit")   # (the package's attribute `fit` is the function)


# ---- 1. vmmin_steps in lockstep -----------------------------------------------------------------------------------------------------
def _objective(x):
    """Rosenbrock on the first two entries plus a quadratic on all of them"""
    w = np.arange(1, x.size + 1, dtype=float)
    return 100.0 * (x[1] - x[0] ** 2) ** 2 + (1.0 - x[0]) ** 2 + 0.5 * float(np.sum(w * (x - 0.3) ** 2))


def _gradient(x):
    w = np.arange(1, x.size + 1, dtype=float)
    g = w * (x - 0.3)
    g[0] += -400.0 * x[0] * (x[1] - x[0] ** 2) - 2.0 * (1.0 - x[0])
    g[1] += 200.0 * (x[1] - x[0] ** 2)
    return g


def test_vmmin_steps_in_lockstep_gives_the_bits_of_separate_vmmin_calls():
    starts = [np.array([-1.2, 1.0, 0.0]), np.array([2.0, -1.5, 1.0]), np.array([0.0, 0.0, 0.0]), np.array([3.0, 3.0, -2.0]), np.array([-0.5, 2.5, 0.7])]
    alone = [F.vmmin(s, _objective, _gradient) for s in starts]
    gens = [F.vmmin_steps(s) for s in starts]
    want = [next(g) for g in gens]
    done = [None] * len(starts)
    rounds = 0
    while any(w is not None for w in want):
        rounds += 1
        answers = [None if w is None else (_objective(w[1].copy()) if w[0] == "f" else _gradient(w[1].copy())) for w in want]   # the whole round first
        for i, g in enumerate(gens):
            if want[i] is None:
                continue
            try:
                want[i] = g.send(answers[i])
            except StopIteration as stop:
                want[i], done[i] = None, stop.value
    assert rounds > 5
    for a, b in zip(alone, done):
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:], (a, b)
    assert len({a[2] for a in alone}) > 1          # the instances do finish at different times


def test_vmmin_steps_asks_for_one_value_when_maxit_is_zero():
    g = F.vmmin_steps(np.array([1.0, 2.0]), maxit=0)
    kind, point = next(g)
    assert kind == "f"
    with pytest.raises(StopIteration) as stop:
        g.send(3.5)
    par, value, fn, gr, fail = stop.value.value
    assert np.array_equal(par, [1.0, 2.0]) and (value, fn, gr, fail) == (3.5, 0, 0, 0)


# ---- 2. optimize_multistart on a numpy objective ---------------------------------------------------------------------------------------
NAME, D, N, NOISE = "matern52_ard", 3, 40, 0.05


def _problem():
    X, y, ell = grad_problem(N, D)
    rng = np.random.default_rng(5)
    starts = np.vstack([np.ones(D), ell, ell * np.exp(rng.uniform(-1.0, 1.0, (2, D)))])
    return X, y, starts


def _single_hook(X, y, bad=None, calls=None):
    def hook(theta, nz):
        if calls is not None:
            calls.append(1)
        if bad is not None and bad(theta, nz):
            raise nat.NotPositiveDefinite(3)
        return ard_grad_ref.logp_grad(NAME, theta, X, y, nz)
    return hook


def _batch_hook(X, y, bad=None, sizes=None):
    def hook(thetas, noises):
        if sizes is not None:
            sizes.append(len(noises))
        vals, grads, infos = [], [], []
        for th, nz in zip(thetas, noises):
            if bad is not None and bad(th, nz):
                vals.append(np.nan), grads.append(np.full(D + 1, np.nan)), infos.append(3)
            else:
                v, g = ard_grad_ref.logp_grad(NAME, th, X, y, nz)
                vals.append(v), grads.append(g), infos.append(0)
        return np.array(vals), np.array(grads), np.array(infos)
    return hook


def _same(a, b):
    return (a["par"] == b["par"] and a["noise"] == b["noise"] and a["value"] == b["value"] and a["counts"] == b["counts"]
            and a["convergence"] == b["convergence"])


def test_multistart_gives_optimize_from_every_start_bit_for_bit():
    X, y, starts = _problem()
    sizes, calls = [], []
    r = F.optimize_multistart(X, y, NOISE, NAME, starts, value_and_grad_batch=_batch_hook(X, y, sizes=sizes))
    alone = [F.optimize(X, y, NOISE, NAME, s, value_and_grad=_single_hook(X, y, calls=calls)) for s in starts]
    assert len(r["all"]) == len(starts)
    for a, b in zip(r["all"], alone):
        assert _same(a, b), (a, b)
        assert b["value"] > -1000.0
    best = int(np.argmax([a["value"] for a in alone]))
    assert r["best_index"] == best and _same(r, alone[best])
    assert sum(sizes) == len(calls)                 # the same evaluations, batched:
    assert len(sizes) < len(calls) and max(sizes) == len(starts) and min(sizes) < len(starts)   # one call a round; finished instances drop out


def test_multistart_without_the_noise_and_with_default_starts():
    X, y, _ = _problem()
    r = F.optimize_multistart(X, y, NOISE, NAME, n_starts=3, rng=np.random.default_rng(11), optimize_noise=False, value_and_grad_batch=_batch_hook(X, y))
    again = F.optimize_multistart(X, y, NOISE, NAME, n_starts=3, rng=np.random.default_rng(11), optimize_noise=False, value_and_grad_batch=_batch_hook(X, y))
    assert len(r["all"]) == 3 and all(a["noise"] == NOISE for a in r["all"])
    assert all(_same(a, b) for a, b in zip(r["all"], again["all"]))
    first = F.optimize(X, y, NOISE, NAME, optimize_noise=False, value_and_grad=_single_hook(X, y))   # the default start is the first
    assert _same(r["all"][0], first)
    ratios = np.array([a["par"] for a in r["all"]])
    assert len({tuple(row) for row in ratios}) == 3


def test_a_start_that_fails_at_its_first_point_raises():
    X, y, starts = _problem()
    first = starts[2].copy()
    bad = lambda th, nz: np.array_equal(th, first)   # noqa: E731
    with pytest.raises(ArithmeticError):
        F.optimize_multistart(X, y, NOISE, NAME, starts, value_and_grad_batch=_batch_hook(X, y, bad))
    with pytest.raises(ArithmeticError):                                  # ... as optimize does from that start
        F.optimize(X, y, NOISE, NAME, first, value_and_grad=_single_hook(X, y, bad))


def test_a_start_that_fails_later_takes_the_sentinel_and_the_others_do_not_notice():
    X, y, starts = _problem()
    seen = []

    def record(th, nz):
        seen.append((th.copy(), nz))
        return False

    F.optimize(X, y, NOISE, NAME, starts[3], value_and_grad=_single_hook(X, y, record))
    assert len(seen) > 3
    t_bad, n_bad = seen[1]                            # the second point start 3 evaluates: the first trial of its first line search
    bad = lambda th, nz: np.array_equal(th, t_bad) and nz == n_bad   # noqa: E731
    r = F.optimize_multistart(X, y, NOISE, NAME, starts, value_and_grad_batch=_batch_hook(X, y, bad))
    alone = [F.optimize(X, y, NOISE, NAME, s, value_and_grad=_single_hook(X, y, bad)) for s in starts]
    clean = [F.optimize(X, y, NOISE, NAME, s, value_and_grad=_single_hook(X, y)) for s in starts[:3]]
    for a, b in zip(r["all"], alone):
        assert _same(a, b), (a, b)
    for a, b in zip(r["all"][:3], clean):             # the other starts: as if nothing had failed
        assert _same(a, b)
    assert r["all"][3]["value"] > -1000.0             # the sentinel was a rejected trial point, not the result


# ---- 3. the numpy model of the batched algorithm stays inside the bound the GPU tests use ----------------------------------------------
@pytest.mark.parametrize("case", R.GRID_CASES)
def test_model_of_the_batched_algorithm_is_within_tol_of_the_closed_form(case):
    worst = dict(logp=0.0, grad=0.0, block=0.0, alpha=0.0)
    for n in R.GRID_SIZES:
        name, X, y, thetas, noises = R.models(case, n)
        for (want_lp, want_g, want_a), th, nz in zip(R.references(case, n), thetas, noises):
            lp, g, al = R.numpy_model(name, th, X, y, nz)
            worst["logp"] = max(worst["logp"], abs(lp - want_lp) / abs(want_lp))
            worst["grad"] = max(worst["grad"], nerr(g, want_g))
            worst["block"] = max(worst["block"], nerr(g[:-1], want_g[:-1]))
            worst["alpha"] = max(worst["alpha"], nerr(al, want_a))
    print(case, {k: "%.2e" % v for k, v in worst.items()})
    assert all(v <= TOL for v in worst.values()), worst


# ---- 4. unequal data sets are padded into the strided layout -----------------------------------------------------------------------------
class _StubLib:
    def __init__(self):
        self.calls = []

    def gprc_gpr_batch_logp_grad(self, ctx, kid, B, params, n_params, ld_params, noise, X, d, n_max, x_stride, y, y_stride, n_each, logp, grad, alpha, info):
        import ctypes as C

        def arr(addr, count, typ=C.c_double):
            return np.ctypeslib.as_array((typ * count).from_address(addr)).copy()

        self.calls.append(dict(kid=kid, B=B, params=arr(params, B * ld_params).reshape(B, ld_params), n_params=n_params, noise=arr(noise, B),
                               X=arr(X, (B - 1) * x_stride + d * n_max), d=d, n_max=n_max, x_stride=x_stride, y=arr(y, (B - 1) * y_stride + n_max),
                               y_stride=y_stride, n_each=None if not n_each else arr(n_each, B, C.c_int64), alpha=alpha))
        np.ctypeslib.as_array((C.c_double * B).from_address(logp))[:] = np.arange(B)
        np.ctypeslib.as_array((C.c_double * (B * (n_params + 1))).from_address(grad))[:] = 2.0
        np.ctypeslib.as_array((C.c_int * B).from_address(info))[:] = 0
        return 0


class _StubCtx:
    handle = None


def test_unequal_data_sets_go_into_their_slabs(monkeypatch):
    stub = _StubLib()
    monkeypatch.setattr(nat, "lib", lambda: stub)
    rng = np.random.default_rng(3)
    d, sizes = 3, [5, 1, 9, 4]
    Xs = [rng.normal(size=(d, n)) for n in sizes]
    ys = [rng.normal(size=n) for n in sizes]
    thetas = rng.uniform(0.5, 2.0, (4, d))
    logp, grad, info = F.logp_grad_batch(Xs, ys, [0.1, 0.2, 0.3, 0.4], "sqrexp_ard", thetas, ctx=_StubCtx())
    (c,) = stub.calls
    assert (c["B"], c["d"], c["n_max"], c["x_stride"], c["y_stride"], c["n_params"]) == (4, d, 9, d * 9, 9, d)
    assert c["kid"] == F.grad_dict["sqrexp_ard"].kernel_id and c["alpha"] is None
    assert np.array_equal(c["n_each"], sizes) and np.array_equal(c["noise"], [0.1, 0.2, 0.3, 0.4]) and np.array_equal(c["params"], thetas)
    for b, n in enumerate(sizes):
        slab = c["X"][b * d * 9:(b + 1) * d * 9]
        assert np.array_equal(slab[:d * n].reshape(n, d).T, Xs[b])        # point-major: coordinate r of point g at g d + r
        assert np.array_equal(c["y"][b * 9:b * 9 + n], ys[b])
    assert np.array_equal(logp, np.arange(4.0)) and grad.shape == (4, d + 1) and np.array_equal(info, np.zeros(4))
    # one shared data set: no strides, no n_each; a scalar noise is one value per model
    F.logp_grad_batch(Xs[2], ys[2], 0.25, "sqrexp_ard", thetas, ctx=_StubCtx())
    c = stub.calls[1]
    assert (c["x_stride"], c["y_stride"], c["n_max"]) == (0, 0, 9) and c["n_each"] is None
    assert np.array_equal(c["noise"], np.full(4, 0.25)) and np.array_equal(c["X"].reshape(9, d).T, Xs[2])
    with pytest.raises(ValueError):
        F.logp_grad_batch(rng.normal(size=(d, 129)), rng.normal(size=129), 0.1, "sqrexp_ard", thetas, ctx=_StubCtx())
