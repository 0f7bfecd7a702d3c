"""The Vecchia likelihood on the device (gprc_lgpr_vecchia_* and LocalGPR.vecchia_*, fit.vecchia_logp_grad, fit.optimize_local) against
the difference-of-marginals reference of tests/vecchia_ref.py on the reference's neighbours: the stored neighbours, every conditional,
the value and the gradient at model sizes on both sides of every 16-block boundary and at 128; the exact likelihood at m_cond >= n - 1;
the bit contract (chunks, groups of 256, pointers, outputs asked for, prefixes); flagged points; frozen neighbours; the optimiser against
the same call driven by the numpy model; the lifecycle.  conftest.TOL = 1e-10 throughout, as elsewhere in the suite."""
import ctypes as C
import math
import sys

import numpy as np
import pytest

import local_ref as LR
import vecchia_ref as V
from conftest import TOL, nerr
from gprc_amd import LocalGPR, _native as nat
from gpu_calls import kfun, step_time_limit  # noqa: F401  (autouse fixture)

F = sys.modules["gprc_amd.fit"]   # the module: the package attribute `fit` is the function

pytestmark = pytest.mark.gpu


class Model:
    """a raw gprc_local_model for the length of a with block"""

    def __init__(self, name, theta, X, y, noise, ctx=None):
        rc, self.h = LR.lgpr_create(name, theta, X, y, noise, 16, ctx=ctx)
        assert rc == nat.OK, nat.last_error()

    def __enter__(self):
        return self.h

    def __exit__(self, *exc):
        LR.lgpr_free(self.h)


@pytest.mark.parametrize("m_cond", V.M_CONDS)
@pytest.mark.parametrize("case", V.CASES)
def test_conditionals_value_and_gradient_against_the_reference(case, m_cond):
    name, theta, X, y, noise = V.case(case)
    n = X.shape[1]
    want_idx, _ = V.case_neighbours(case, m_cond)
    cond_ref, grad_ref = V.case_reference(case, m_cond)
    with Model(name, theta, X, y, noise) as h:
        assert V.vecchia_prepare(h, m_cond) == nat.OK, nat.last_error()
        rc, idx = V.vecchia_neighbours(h, n, m_cond)
        assert rc == nat.OK and np.array_equal(idx, want_idx)
        rc, logp, grad, cond, flagged = V.vecchia_call(h, theta, noise, n)
        assert rc == nat.OK, nat.last_error()
    assert flagged == 0
    e_cond = np.abs(cond - cond_ref).max()
    e_val = abs(logp - cond_ref.sum())
    want = grad_ref.sum(0)
    e_grad = nerr(grad, want)
    print(f"vecchia {case} m={m_cond}: max|dcond|={e_cond:.3e} (max|ref|={np.abs(cond_ref).max():.3g}) |dvalue|={e_val:.3e} "
          f"(sum|cond|={np.abs(cond_ref).sum():.4g}) nerr(grad)={e_grad:.3e} nerr(parameter block)={nerr(grad[:-1], want[:-1]):.3e}")
    assert e_cond <= TOL * max(1.0, np.abs(cond_ref).max())
    assert e_val <= TOL * np.abs(cond_ref).sum()
    assert e_grad <= TOL
    if V.block_also(case):
        assert nerr(grad[:-1], want[:-1]) <= TOL


@pytest.mark.parametrize("case", V.CASES)
def test_every_predecessor_gives_the_exact_likelihood(case):
    """n = 100, m_cond = 127 (clamped to 99): the sum is the log marginal likelihood, against gprc_gpr_logp_grad"""
    name, theta, X, y, noise = V.case(case, 100)
    want, want_g = F.logp_grad(X, y, noise, name, theta)
    with Model(name, theta, X, y, noise) as h:
        assert V.vecchia_prepare(h, 127) == nat.OK, nat.last_error()
        rc, logp, grad, cond, flagged = V.vecchia_call(h, theta, noise, 100)
        assert rc == nat.OK and flagged == 0
    print(f"vecchia exact {case}: |dvalue|={abs(logp - want):.3e} sum|cond|={np.abs(cond).sum():.4g} nerr(grad)={nerr(grad, want_g):.3e}")
    assert abs(logp - want) <= TOL * np.abs(cond).sum()
    assert nerr(grad, want_g) <= TOL
    if V.block_also(case):
        assert nerr(grad[:-1], want_g[:-1]) <= TOL
    value, g = F.vecchia_logp_grad(X, y, noise, name, theta, m=127)          # the Python front: the same call
    assert value == logp and np.array_equal(g, grad)


def test_bits_do_not_depend_on_chunks_pointers_or_outputs():
    """n = 2 chunks + 257 at m_cond = 4: launch chunks and groups of 256 are straddled"""
    torch = pytest.importorskip("torch")
    X, y = V.bits_data()
    n = X.shape[1]
    name, theta, noise = "matern52_ard", np.array([0.3, 0.5]), 0.05
    with Model(name, theta, X, y, noise) as h:
        assert V.vecchia_prepare(h, 4) == nat.OK, nat.last_error()
        rc, logp, grad, cond, flagged = V.vecchia_call(h, theta, noise, n)
        assert rc == nat.OK and flagged == 0 and np.isfinite(cond).all(), nat.last_error()
        again = V.vecchia_call(h, theta, noise, n)
        assert again[1] == logp and np.array_equal(again[2], grad) and np.array_equal(again[3], cond)
        rc, lp, g, c, _ = V.vecchia_call(h, theta, noise, n, grad=False)                      # the value alone
        assert rc == nat.OK and lp == logp and g is None and np.array_equal(c, cond)
        rc, lp, g, c, _ = V.vecchia_call(h, theta, noise, n, cond=False, flagged=False)      # without cond_out and flagged_out
        assert rc == nat.OK and lp == logp and c is None and np.array_equal(g, grad)
        ct = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rc, lp, g, _, _ = V.vecchia_call(h, theta, noise, n, cond_out=ct)                      # cond_out in device memory
        assert rc == nat.OK and lp == logp and np.array_equal(g, grad) and np.array_equal(ct.cpu().numpy(), cond)
        rc, idx = V.vecchia_neighbours(h, n, 4, ld=6)
        assert rc == nat.OK and (idx[:, 4:] == -7).all()
    # a second object, its points and targets handed over in device memory
    xd, yd = torch.from_numpy(LR.flat(X)).cuda(), torch.from_numpy(y).cuda()
    kid, (_, pp, npar) = V.kernel_id(name), nat.params_array(theta)
    h2 = C.c_void_p()
    assert nat.lib().gprc_lgpr_create(nat.default_context().handle, kid, pp, npar, xd.data_ptr(), 2, n, yd.data_ptr(), noise, 16, C.byref(h2)) == nat.OK
    try:
        assert V.vecchia_prepare(h2, 4) == nat.OK, nat.last_error()
        rc, idx2 = V.vecchia_neighbours(h2, n, 4)
        assert rc == nat.OK and np.array_equal(idx2, idx[:, :4])
        second = V.vecchia_call(h2, theta, noise, n)
        assert second[1] == logp and np.array_equal(second[2], grad) and np.array_equal(second[3], cond)
    finally:
        LR.lgpr_free(h2)
    # the groups' sums: the value is the conditionals added 256 at a time in the documented order, so it is close to their plain sum
    assert abs(logp - cond.sum()) <= 1e-12 * np.abs(cond).sum()


@pytest.mark.parametrize("m_cond", [15, 64])
def test_a_conditional_does_not_depend_on_the_points_behind_it(m_cond):
    """cond_i of a one-point-shorter and of a longer set with the same first points: N(i) is the same, so are the bits"""
    name, theta, X, y, noise = V.case("ratquad", 400)
    conds = {}
    for n in (299, 300, 400):
        with Model(name, theta, X[:, :n], y[:n], noise) as h:
            assert V.vecchia_prepare(h, m_cond) == nat.OK, nat.last_error()
            rc, _, _, conds[n], _ = V.vecchia_call(h, theta, noise, n)
            assert rc == nat.OK
    assert np.array_equal(conds[300][:299], conds[299]) and np.array_equal(conds[400][:300], conds[300])


def test_flagged_points_are_nan_and_nobody_else_is_disturbed():
    name, theta, X, Xdup, y, ydup, _, m = LR.flagged_data()
    n = X.shape[1]
    with Model(name, theta, X, y, 0.0) as h:
        assert V.vecchia_prepare(h, m) == nat.OK, nat.last_error()
        rc, logp, grad, cond, flagged = V.vecchia_call(h, theta, 0.0, n)
        assert rc == nat.OK and flagged == 0 and np.isfinite(logp) and np.isfinite(grad).all() and np.isfinite(cond).all()
    with Model(name, theta, Xdup, ydup, 0.0) as h:
        assert V.vecchia_prepare(h, m) == nat.OK, nat.last_error()
        rc, logp2, grad2, cond2, flagged2 = V.vecchia_call(h, theta, 0.0, n + 2)
        assert rc == nat.OK, nat.last_error()                                      # the call does not fail
        with LocalGPR(Xdup, ydup, 0.0, kfun(name, theta), m=m) as model:           # the Python front reports the same
            model.vecchia_prepare(m)
            value, g = model.vecchia_logp_grad()
            assert math.isnan(value) and np.isnan(g).all() and model.vecchia_flagged == 2
    assert flagged2 == 2 and math.isnan(logp2) and np.isnan(grad2).all()
    assert np.array_equal(np.isnan(cond2), np.arange(n + 2) >= n)
    assert np.array_equal(cond2[:n], cond)


def test_neighbours_are_frozen_until_the_next_prepare():
    name, theta, X, y, noise = V.case("ard3")
    n, m = X.shape[1], 17
    other = theta[::-1] * np.array([0.5, 1.0, 3.0])
    want_other = V.knn_before_ref(X, m, 1.0 / other)[0]
    assert not np.array_equal(want_other, V.case_neighbours("ard3", m)[0])          # the two metrics order the points differently
    with LocalGPR(X, y, noise, kfun(name, theta), m=32) as model:
        assert model.vecchia_prepare(m) == m
        first = model.vecchia_neighbours
        assert np.array_equal(first, V.case_neighbours("ard3", m)[0])
        value, grad = model.vecchia_logp_grad()
        model.set_params(kfun(name, other), noise)
        assert np.array_equal(model.vecchia_neighbours, first)                       # frozen
        moved, _ = model.vecchia_logp_grad()                                        # the new parameters on the OLD neighbours
        back, gback = model.vecchia_logp_grad(theta, noise)                         # the parameters of the call, not the object's
        assert back == value and np.array_equal(gback, grad) and moved != value
        model.vecchia_prepare(m)
        assert np.array_equal(model.vecchia_neighbours, want_other)                  # the reference's in the new metric
        assert model.vecchia_prepare() == 32 and model.vecchia_neighbours.shape == (n, 32)   # the default: min(self.m, 127)


def test_the_optimiser_agrees_with_the_same_call_on_the_numpy_model():
    """n = 1500, d = 2, matern52_ard, m = 30, data drawn from that kernel: fit.optimize_local on the device against the same call driven
    by the numpy model through value_and_grad, from the same start.  vmmin stops when a step changes the value by less than
    reltol (|value| + reltol): the final values agree within 100 times that (the stop bounds the last step, not the distance from the
    optimum).  Reports (not bounds): the difference, and the distance of the learned parameters from fit.optimize's on the same data."""
    n, m = 1500, 30
    X, y, noise = V.optimiser_data(n)
    start = np.array([1.0, 1.0])
    got = F.optimize_local(X, y, 0.1, "matern52_ard", start, m=m, order="given")
    hook = V.ArdVecchia("matern52_ard", X, y, m)
    want = F.optimize_local(X, y, 0.1, "matern52_ard", start, m=m, order="given", value_and_grad=hook)
    reltol = math.sqrt(np.finfo(float).eps)
    diff = abs(got["value"] - want["value"])
    exact = F.optimize(X, y, 0.1, "matern52_ard", start)
    print(f"optimize_local n={n} m={m}: device {got['value']:.6f} par={got['par']} noise={got['noise']:.5f} counts={got['counts']}; numpy "
          f"{want['value']:.6f} par={want['par']} noise={want['noise']:.5f}; |dvalue|={diff:.3e}; fit.optimize (exact likelihood) "
          f"{exact['value']:.6f} par={exact['par']} noise={exact['noise']:.5f}; max rel distance of (par, noise) from it "
          f"{np.abs(np.array(got['par'] + (got['noise'],)) / np.array(exact['par'] + (exact['noise'],)) - 1).max():.3e}; data drawn with "
          f"l=(0.35, 0.8) noise={noise}")
    assert diff <= 100 * reltol * (abs(want["value"]) + reltol)
    assert got["rounds"] == 2 and hook.prepares == 2 and got["m"] == m and got["order"] == "given" and got["convergence"] in (0, 1)
    with LocalGPR(X, y, got["noise"], got["func"], m=m) as model:                   # the result goes straight into LocalGPR
        assert np.isfinite(model.predict(X[:, :3])).all()


def test_the_optimiser_far_below_the_siblings_sentinel():
    """targets 300 times larger: the likelihood starts near -1e8, far below -10000, and vmmin's first full step along a gradient of
    that size overshoots to where exp(z) overflows, underflows or is subnormal.  Those evaluations must count as failures that are never
    accepted (not as a value of -10000, which would look like an improvement): the run ends above its start, at a finite point"""
    X, y, _ = V.optimiser_data(1500)
    y = 300.0 * y
    with LocalGPR(X, y, 0.1, kfun("matern52_ard", [1.0, 1.0]), m=16) as model:
        model.vecchia_prepare(15)
        start = model.vecchia_logp_grad()[0]
    r = F.optimize_local(X, y, 0.1, "matern52_ard", [1.0, 1.0], m=15, order="given")
    print(f"optimize_local on 300 y: start {start:.6g} -> {r['value']:.6g} par={r['par']} noise={r['noise']:.5g} counts={r['counts']}")
    assert start < -10000.0 and math.isfinite(r["value"]) and r["value"] > start
    assert all(math.isfinite(v) and v > 0 for v in r["par"] + (r["noise"],)) and r["convergence"] in (0, 1)


def test_argument_errors_and_lifecycle():
    name, theta, X, y, noise = V.case("sqrexp", 50)
    lib = nat.lib()
    _, pp, npar = nat.params_array(theta)
    out, g = C.c_double(), np.zeros(npar + 1)

    def bad(rc, word):
        assert rc == nat.ERR_ARG and word in nat.last_error(), (rc, nat.last_error())

    bad(lib.gprc_lgpr_vecchia_prepare(None, 8), "null model")
    bad(lib.gprc_lgpr_vecchia_logp_grad(None, pp, npar, noise, C.byref(out), g.ctypes.data, None, None), "null model")
    with Model(name, theta, X, y, noise) as h:
        bad(lib.gprc_lgpr_vecchia_logp_grad(h, pp, npar, noise, C.byref(out), g.ctypes.data, None, None), "prepare")
        bad(lib.gprc_lgpr_vecchia_neighbours(h, None, 8), "prepare")
        for m in (0, 128):
            bad(V.vecchia_prepare(h, m), "outside 1 .. 127")
        assert V.vecchia_prepare(h, 8) == nat.OK
        bad(lib.gprc_lgpr_vecchia_logp_grad(h, None, npar, noise, C.byref(out), g.ctypes.data, None, None), "params")
        bad(lib.gprc_lgpr_vecchia_logp_grad(h, pp, npar, noise, None, g.ctypes.data, None, None), "null output")
        bad(lib.gprc_lgpr_vecchia_logp_grad(h, pp, npar, -1.0, C.byref(out), g.ctypes.data, None, None), "noise")
        bad(lib.gprc_lgpr_vecchia_logp_grad(h, pp, npar + 1, noise, C.byref(out), g.ctypes.data, None, None), "")
        bad(V.vecchia_neighbours(h, 50, 8, ld=7)[0], "ld_out < m_cond")
        bad(lib.gprc_lgpr_vecchia_neighbours(h, None, 8), "null output")
        assert V.vecchia_prepare(h, 127) == nat.OK                                    # clamped to n - 1; replaces the first
        rc, idx = V.vecchia_neighbours(h, 50, 49)
        assert rc == nat.OK and np.array_equal(idx, V.knn_before_ref(X, 49)[0])
    with Model(name, theta, X[:, :1], y[:1], noise) as h:                             # n = 1: nothing is kept, the sum is the one marginal
        assert V.vecchia_prepare(h, 5) == nat.OK
        rc, logp, grad, cond, flagged = V.vecchia_call(h, theta, noise, 1)
        want = -0.5 * y[0] ** 2 / (1 + noise) - 0.5 * math.log(1 + noise) - 0.5 * math.log(2 * math.pi)
        assert rc == nat.OK and flagged == 0 and abs(logp - want) <= 1e-14 * abs(want) and cond[0] == logp
    model = LocalGPR(X, y, noise, kfun(name, theta), m=8)
    with pytest.raises(ValueError):
        model.vecchia_logp_grad()                                                    # no prepare yet
    model.vecchia_prepare()
    assert model.vecchia_flagged is None and np.isfinite(model.vecchia_logp_grad()[0]) and model.vecchia_flagged == 0
    model.close()
    model.close()
    with pytest.raises(nat.GprcError):
        model.vecchia_prepare()
    with LocalGPR(X, y, noise, kfun(name, theta), m=8) as model:
        model.vecchia_prepare(3)
        assert model.vecchia_logp_grad(grad=False)[1] is None and model.vecchia_logp_grad(cond=True)[2].shape == (50,)
    with pytest.raises(nat.GprcError):
        model.vecchia_neighbours
    own = nat.Context(0)                                                            # a context destroyed first
    rc, h = LR.lgpr_create(name, theta, X, y, noise, 8, ctx=own)
    assert rc == nat.OK and V.vecchia_prepare(h, 8) == nat.OK
    own.close()
    bad(V.vecchia_prepare(h, 8), "context has been destroyed")
    bad(lib.gprc_lgpr_vecchia_logp_grad(h, pp, npar, noise, C.byref(out), g.ctypes.data, None, None), "context has been destroyed")
    assert lib.gprc_lgpr_free(h) == nat.OK
