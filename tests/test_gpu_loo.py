"""Leave-one-out cross-validation on the MI355X: gprc_gpr_loo (GPR.loo, GPR.loo_score) and gprc_gpr_loo_grad (fit.loo_grad,
fit.optimize(objective="loo")) against the float64 closed form of tests/loo_ref.py, which tests/test_loo_cpu.py ties to a brute force
that really leaves each point out.  Gates: the project's TOL = 1e-10, normwise (conftest.nerr) on vectors and relative on scalars; the
gradient 1e-10 normwise (the gate of tests/test_gpu_ard_grad.py); central differences 1e-6 (as for logp_grad).

Geometry: n = 5 (less than one tile), 300 (one panel, not a multiple of the tile), 700 (two panels), 1300 (three panels; eleven row tiles
of the contraction); d = 1, 3 and 20 (two staging passes of the ARD path).  Every case asserts in the test that numpy's cond(K_y) <= 1e4
and that the fit succeeded at the first attempt (the stored noise is the noise asked for / the call without a retry returned 0).

Measured on an MI355X (every test prints its figures): gprc_gpr_loo against the closed form <= 3.3e-13 (ell, sqrexp, n = 1300, d = 1,
cond 6.4e3); against a model fitted without the point <= 2.7e-15; gprc_gpr_loo_grad's gradient <= 1.9e-14 and value <= 4.6e-15; against
central differences of the library's own score <= 6.0e-11; the two paths to the score agree to the last bit on the two cases here.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import kernel_ref as K
import loo_ref as R
from conftest import TOL, nerr
from gprc_amd import GPC, GPR, GprcError, NotPositiveDefinite, cov_func, linear, sqrexp
from gprc_amd import _native as nat
from gprc_amd.fit import loo_grad, optimize
from gpu_calls import kfun, same_bits, step_time_limit  # noqa: F401  (the autouse fixture)

pytestmark = pytest.mark.gpu

NOISE = 0.1
COND_MAX = 1e4


def problem(n, d):
    rng = np.random.default_rng(4000 + 7 * n + d)
    X = np.asfortranarray(rng.uniform(-2.0, 2.0, (d, n)))
    y = np.sin(X.sum(0)) + 0.3 * np.cos(2.0 * X[0]) + 0.1 * rng.standard_normal(n)
    return X, y


def theta_of(name, d):
    """parameters in the ABI's order; the length scales grow with sqrt(d / 3): at the scales of d = 3 a kernel matrix of 20 coordinates is
    nearly the identity and its length-scale gradient vanishes beside the noise's"""
    s = max(1.0, np.sqrt(d / 3.0))
    if name.endswith("_ard"):
        return np.linspace(0.8, 1.9, d) * s
    return {"sqrexp": [0.9 * s], "gammaexp": [1.1 * s, 1.5], "gammaexp1": [1.2 * s, 1.0], "rationalquadratic": [0.9 * s, 1.7],
            "matern32": [0.9 * s], "matern52": [1.1 * s], "linear": [0.5]}[name]


def kname(name):
    return "gammaexp" if name == "gammaexp1" else name


def kernel_of(name, theta):
    if name == "linear":
        return cov_func(linear, sigma=theta[0])
    return kfun(kname(name), theta)


@functools.lru_cache(maxsize=None)
def reference(name, n, d, with_grad=False):
    """the closed form of (name, n, d) at NOISE, computed once and shared; the arrays are never written to"""
    X, y = problem(n, d)
    th = theta_of(name, d)
    cond = R.cond_Ky(kname(name), th, X, NOISE)
    r = R.loo(kname(name), th, X, y, NOISE)
    out = dict(X=X, y=y, theta=th, cond=cond, mean=r["mean"], var=r["var"], ell=r["ell"], loo=float(r["loo"]))
    if with_grad:
        out["grad"] = np.asarray(R.loo_grad(kname(name), th, X, y, NOISE)[1], dtype=float)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def raw_loo(model, n, mean=True, var=True, dens=True, score=True):
    """gprc_gpr_loo with host pointers; an output not asked for is passed as NULL and returned as None"""
    out = [np.full(n, np.nan) if want else None for want in (mean, var, dens)]
    sc = C.c_double(float("nan"))
    nat.check(nat.lib().gprc_gpr_loo(model, *[o.ctypes.data if o is not None else None for o in out], C.byref(sc) if score else None))
    return out + [sc.value if score else None]


# ---- 1. gprc_gpr_loo against the closed form --------------------------------------------------------------------------------------
LOO_CASES = [("sqrexp", 5, 1), ("linear", 300, 3), ("gammaexp", 300, 1), ("matern32_ard", 300, 3), ("rationalquadratic", 700, 3),
             ("sqrexp_ard", 700, 20), ("matern52", 700, 1), ("matern32", 1300, 3), ("matern52_ard", 1300, 20), ("sqrexp", 1300, 1)]


@pytest.mark.parametrize("name,n,d", LOO_CASES, ids=lambda v: str(v))
def test_loo_against_the_closed_form(name, n, d):
    ref = reference(name, n, d)
    assert ref["cond"] <= COND_MAX, ref["cond"]
    g = GPR(ref["X"], ref["y"], NOISE, kernel_of(name, ref["theta"]))
    assert g.noise == NOISE                                   # the fit succeeded at the first attempt
    got = g.loo()
    score = g.loo_score
    g.close()
    assert got.shape == (n, 3)
    errs = [nerr(got[:, 0], ref["mean"]), nerr(got[:, 1], ref["var"]), nerr(got[:, 2], ref["ell"]), abs(score - ref["loo"]) / abs(ref["loo"])]
    print("loo %s n %d d %d cond %.3g: mean %.2e var %.2e ell %.2e score %.2e" % (name, n, d, ref["cond"], *errs))
    assert max(errs) <= TOL, errs
    acc = np.longdouble(0)
    for v in got[:, 2]:                                       # the sum in index order in long double
        acc += np.longdouble(v)
    assert score == float(acc)


# ---- 2. end to end, no reference ---------------------------------------------------------------------------------------------------
def test_loo_is_the_prediction_of_a_model_without_the_point():
    n, d, name = 700, 3, "matern52_ard"
    X, y = problem(n, d)
    th = theta_of(name, d)
    g = GPR(X, y, NOISE, kernel_of(name, th))
    assert g.noise == NOISE
    got = g.loo()
    g.close()
    worst = 0.0
    for i in (0, 350, 699):
        keep = np.arange(n) != i
        h = GPR(np.asfortranarray(X[:, keep]), y[keep], NOISE, kernel_of(name, th))
        assert h.noise == NOISE
        pred = h.predict(X[:, i:i + 1])
        h.close()
        em, ev = abs(pred[0, 0] - got[i, 0]) / np.abs(got[:, 0]).max(), abs(pred[0, 1] + NOISE - got[i, 1]) / np.abs(got[:, 1]).max()
        print("left out %d: mean %.2e var %.2e" % (i, em, ev))
        worst = max(worst, em, ev)
    assert worst <= TOL, worst


# ---- 3. chunking and repetition ----------------------------------------------------------------------------------------------------
def test_loo_is_bitwise_chunk_invariant_and_repeatable(monkeypatch):
    ref = reference("rationalquadratic", 700, 3)
    k = kernel_of("rationalquadratic", ref["theta"])
    g = GPR(ref["X"], ref["y"], NOISE, k)
    whole = raw_loo(g._model, 700)
    assert same_bits(raw_loo(g._model, 700), whole)
    monkeypatch.setenv("GPRC_CHUNK_BYTES", str(256 * 1024 * 8))   # 256 rows per chunk at n_pad = 1024: three chunks
    ctx2 = nat.Context(0)
    g2 = GPR(ref["X"], ref["y"], NOISE, k, ctx=ctx2)
    parts = raw_loo(g2._model, 700)
    assert same_bits(parts, whole)
    assert same_bits(raw_loo(g2._model, 700), whole)
    g2.close()
    ctx2.close()
    g.close()


# ---- 4. pointer kinds, null outputs, refusals ---------------------------------------------------------------------------------------
def test_pointer_kinds_null_outputs_and_refusals():
    torch = pytest.importorskip("torch")
    n = 700
    ref = reference("rationalquadratic", n, 3)
    g = GPR(ref["X"], ref["y"], NOISE, kernel_of("rationalquadratic", ref["theta"]))
    host = raw_loo(g._model, n)
    dev = torch.device("cuda:0")
    outs = [torch.full((n,), float("nan"), dtype=torch.float64, device=dev) for _ in range(3)]
    torch.cuda.synchronize()
    sc = C.c_double()
    nat.check(nat.lib().gprc_gpr_loo(g._model, *[o.data_ptr() for o in outs], C.byref(sc)))
    assert same_bits([o.cpu().numpy() for o in outs] + [sc.value], host)
    for mask in ((True, False, False, False), (False, True, False, True), (False, False, True, False), (False, False, False, True)):
        sub = raw_loo(g._model, n, *mask)
        assert same_bits(sub, [h if want else None for h, want in zip(host, mask)]), mask
    with pytest.raises(GprcError, match="all four outputs are null") as ei:
        raw_loo(g._model, n, False, False, False, False)
    assert ei.value.status == nat.ERR_ARG
    g.close()
    rng = np.random.default_rng(3)
    Xc = rng.uniform(-1, 1, (2, 60))
    yc = np.sign(Xc[0] + 0.1 * rng.standard_normal(60))
    yc[yc == 0] = 1.0
    c = GPC(Xc, yc, cov_func(sqrexp, l=0.8))
    with pytest.raises(GprcError, match="not a GPR model") as ei:
        raw_loo(c._model, 60)
    assert ei.value.status == nat.ERR_ARG


# ---- 5. several (virtual) ranks ---------------------------------------------------------------------------------------------------
def test_loo_of_a_model_over_virtual_ranks_is_the_single_gpu_one():
    ref = reference("matern32", 1300, 3)
    k = kernel_of("matern32", ref["theta"])
    one = GPR(ref["X"], ref["y"], NOISE, k)
    two = GPR(ref["X"], ref["y"], NOISE, k, devices=[0, 0])
    a, b = one.loo(), two.loo()
    sa, sb = one.loo_score, two.loo_score
    two.close()
    one.close()
    assert np.array_equal(a, b) and sa == sb
    assert nerr(b[:, 2], ref["ell"]) <= TOL


# ---- 6. gprc_gpr_loo_grad against the closed form --------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(300, 3), (1300, 20)])
@pytest.mark.parametrize("name", K.NAMES)
def test_loo_grad_against_the_closed_form(name, n, d):
    ref = reference(name, n, d, True)
    assert ref["cond"] <= COND_MAX, ref["cond"]
    value, grad = loo_grad(ref["X"], ref["y"], NOISE, name, ref["theta"])     # no retry: returning at all is the first attempt's success
    assert grad.shape == (len(ref["theta"]) + 1,)
    ev, eg = abs(value - ref["loo"]) / abs(ref["loo"]), nerr(grad, ref["grad"])
    print("loo_grad %s n %d d %d cond %.3g: value %.2e grad %.2e (max|d/dtheta| %.3g, d/dnoise %.3g)"
          % (name, n, d, ref["cond"], ev, eg, np.abs(ref["grad"][:-1]).max(), ref["grad"][-1]))
    assert ev <= TOL and eg <= 1e-10, (ev, eg)


# ---- 7. gradient against central differences of the library's own score ------------------------------------------------------------
def library_score(X, y, noise, name, theta):
    g = GPR(X, y, noise, kernel_of(name, theta))
    assert g.noise == noise
    s = g.loo_score
    g.close()
    return s


@pytest.mark.parametrize("name", ["matern52_ard", "gammaexp1"])
def test_loo_grad_against_differences_of_the_loo_score(name):
    n, d, h = 300, 3, 1e-5
    X, y = problem(n, d)
    th = np.asarray(theta_of(name, d), dtype=float)
    grad = loo_grad(X, y, NOISE, kname(name), th)[1]
    fd = np.empty(th.size + 1)
    for k in range(th.size):
        e = np.zeros(th.size)
        e[k] = h * th[k]
        fd[k] = (library_score(X, y, NOISE, name, th + e) - library_score(X, y, NOISE, name, th - e)) / (2.0 * e[k])
    hn = h * NOISE
    fd[-1] = (library_score(X, y, NOISE + hn, name, th) - library_score(X, y, NOISE - hn, name, th)) / (2.0 * hn)
    err = nerr(grad, fd)
    print("loo_grad %s vs central differences of gprc_gpr_loo: %.2e" % (name, err))
    assert err <= 1e-6, err


# ---- 8. the two paths to the score ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,d", [("sqrexp", 300, 3), ("matern52_ard", 1300, 20)])
def test_the_score_of_both_entry_points_agrees(name, n, d):
    ref = reference(name, n, d, True)
    value = loo_grad(ref["X"], ref["y"], NOISE, name, ref["theta"])[0]
    score = library_score(ref["X"], ref["y"], NOISE, name, ref["theta"])
    print("loo_grad's value vs gprc_gpr_loo's %s n %d: %.2e" % (name, n, abs(value - score) / abs(score)))
    assert abs(value - score) <= TOL * abs(score)      # p_i comes from W's diagonal in one, from sums of squares in the other: not bitwise


# ---- 9. determinism and errors ----------------------------------------------------------------------------------------------------
def raw_loo_grad(kid, theta, X, y, noise, ctx, value=True, grad=True):
    _, pp, npar = nat.params_array(theta)
    g, v = np.empty(npar + 1), C.c_double()
    d, n = X.shape
    rc = nat.lib().gprc_gpr_loo_grad(ctx.handle, kid, pp, npar, X.ctypes.data, d, n, y.ctypes.data, noise, C.byref(v) if value else None,
                                     g.ctypes.data_as(C.POINTER(C.c_double)) if grad else None)
    return rc, v.value, g


def test_loo_grad_determinism_and_errors():
    ref = reference("matern52_ard", 1300, 20, True)
    a = loo_grad(ref["X"], ref["y"], NOISE, "matern52_ard", ref["theta"])
    b = loo_grad(ref["X"], ref["y"], NOISE, "matern52_ard", ref["theta"])
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.isfinite(a[1]).all()
    ctx = nat.default_context()
    rng = np.random.default_rng(5)
    X = np.asfortranarray(rng.uniform(-1, 1, (2, 40)))
    y = rng.normal(size=40)
    for kid, par in ((nat.POLYNOMIAL, [1.0, 2.0]), (nat.LINEAR, [1.0]), (nat.CONSTANT, [1.0])):
        rc, *_ = raw_loo_grad(kid, par, X, y, 0.1, ctx)
        assert rc == nat.ERR_ARG and "loo_grad: defined for" in nat.last_error()
    for value, grad in ((False, True), (True, False), (False, False)):
        rc, *_ = raw_loo_grad(nat.SQREXP, [1.0], X, y, 0.1, ctx, value, grad)
        assert rc == nat.ERR_ARG and "null output" in nat.last_error()
    Xdup = np.asfortranarray(np.hstack([X, X[:, :3]]))                # duplicate points, noise 0: singular
    with pytest.raises(NotPositiveDefinite) as ei:
        loo_grad(Xdup, np.concatenate([y, y[:3]]), 0.0, "sqrexp_ard", [1.0, 1.0])
    assert ei.value.info > 0


# ---- 10. fit.optimize(objective="loo") --------------------------------------------------------------------------------------------
def test_optimize_the_loo_score_end_to_end():
    rng = np.random.default_rng(12)
    n, d = 400, 3
    X = np.asfortranarray(rng.uniform(-2, 2, (d, n)))
    y = np.sin(2 * X[0]) + 0.5 * X[2] ** 2 + 0.1 * rng.normal(size=n)          # coordinate 1 is irrelevant
    start = loo_grad(X, y, NOISE, "matern52_ard", np.ones(d))[0]
    r = optimize(X, y, NOISE, "matern52_ard", objective="loo", maxit=30)
    print("optimize loo:", r["value"], r["par"], r["noise"], r["counts"], "start", start)
    assert r["value"] > start
    assert int(np.argmax(r["par"])) == 1
    g = GPR(X, y, r["noise"], r["func"])
    assert g.noise == r["noise"]
    score = g.loo_score
    g.close()
    assert abs(score - r["value"]) <= TOL * abs(r["value"])
