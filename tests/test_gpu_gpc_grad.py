"""GPC hyper-parameters on the MI355X: the Laplace log evidence and its exact gradient (gprc_gpc_logq_grad / fit.logq_grad /
fit.optimize_gpc).

The gradient and the value against the numpy float64 reference of tests/gpc_grad_ref.py (the book's per-parameter form; the device
contracts a rank-two form that shares no algebra with it) at the project's 1e-10; the value tied to the existing GPC path through
    logq = GPC$logq + sum(diag(L)) - sum(log(diag(L)));
the gradient against central differences of the library's own value (1e-6); pointer kinds, determinism, profile kinds, errors;
fit.optimize_gpc end to end.

epsilon is 1e-10 everywhere: the gradient is that of the CONVERGED mode.  With GPC$new's default 1e-5 the mode search stops one
Newton step short at n = 3000 and the gradient is off by 2.6e-9 (numpy reference).  Every case first asserts, on the reference
alone, that it converged in < 50 steps and that none of its objective decrements lies within a factor 1.2 of epsilon, so that the
step at which the search stops cannot depend on rounding and the iteration counts can be compared.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import TOL, nerr
from gprc_amd import GPC, GprcError
from gprc_amd import _native as nat
from gprc_amd.fit import grad_dict, logp_grad, logq_grad, optimize_gpc
from case_checks import (LOGQ_CASES as CASES, LOGQ_MATERN_CASES as MATERN_CASES, LOGQ_MATERN_WIDE as MATERN_WIDE, LOGQ_WIDE_CASES as WIDE_CASES,
                         check_value_is_tied_to_the_fitted_classifier, logq_case, logq_reference)
from gpu_calls import EPS, gpc_problem, raw_logq_grad, step_time_limit  # noqa: F401  (the autouse fixture)

pytestmark = pytest.mark.gpu


# ---- 1. closed form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,n", [(c, n) for n in [300, 600, 3000, 5000] for c in CASES] + [(c, 300) for c in WIDE_CASES]
                         + [(c, n) for n in [600, 1100] for c in MATERN_CASES] + [(c, 300) for c in MATERN_WIDE])
def test_gradient_against_the_closed_form(case, n):
    name, theta, X, y = logq_case(case, n)
    want_logq, want, want_iters = logq_reference(name, theta, X, y)
    Xf = np.asfortranarray(X)
    logq, grad, iters = raw_logq_grad(grad_dict[name].kernel_id, theta, Xf.ctypes.data, X.shape[0], n, y.ctypes.data, nat.default_context())
    assert grad.shape == (theta.size,)
    e = nerr(grad, want)
    print(f"logq_grad {case} n={n}: nerr(grad)={e:.3e} rel(logq)={abs(logq - want_logq) / abs(want_logq):.3e} iters={iters} ref={want_iters} "
          f"max|d/dtheta|={np.abs(want).max():.3g} min|d/dtheta|={np.abs(want).min():.3g}")
    assert e <= TOL
    assert abs(logq - want_logq) <= TOL * abs(want_logq)
    assert iters == want_iters
    lq2, g2 = logq_grad(X, y, name, theta)                         # the host mirror is the same call
    assert lq2 == logq and np.array_equal(g2, grad)


# ---- 2. tie to the existing path --------------------------------------------------------------------------------------------
# (the Matern cases of this check keep the name they have always had, in tests/test_gpu_matern.py)
@pytest.mark.parametrize("n", [300, 600, 3000])
@pytest.mark.parametrize("case", list(CASES))
def test_value_is_tied_to_the_fitted_classifier(case, n):
    check_value_is_tied_to_the_fitted_classifier(case, n)


# ---- 3. gradient against differences of the library's own value -------------------------------------------------------------
def test_gradient_against_differences_of_the_library_value():
    name, theta, X, y = logq_case("ard8", 3000)
    _, grad = logq_grad(X, y, name, theta)
    fd = np.empty(8)
    for k in range(8):
        e = np.zeros(8)
        e[k] = 1e-5 * theta[k]
        fd[k] = (logq_grad(X, y, name, theta + e)[0] - logq_grad(X, y, name, theta - e)[0]) / (2 * e[k])
    err = nerr(grad, fd)
    print("logq_grad vs central differences of its own value:", err)
    assert err <= 1e-6


# ---- 4. pointer kinds and determinism ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["ard8", "gammaexp1.5"])
def test_pointer_kinds_repeat_calls_and_trim_give_the_same_bits(case):
    torch = pytest.importorskip("torch")
    name, theta, X, y = logq_case(case, 1100)
    X = np.asfortranarray(X)
    d, n = X.shape
    kid = grad_dict[name].kernel_id
    ctx = nat.default_context()
    host = raw_logq_grad(kid, theta, X.ctypes.data, d, n, y.ctypes.data, ctx)
    again = raw_logq_grad(kid, theta, X.ctypes.data, d, n, y.ctypes.data, ctx)
    dev = torch.device("cuda:0")
    Xd, yd = torch.from_numpy(X.T.copy()).to(dev), torch.from_numpy(y).to(dev)
    torch.cuda.synchronize()
    device = raw_logq_grad(kid, theta, Xd.data_ptr(), d, n, yd.data_ptr(), ctx)
    nat.check(nat.lib().gprc_ctx_trim(ctx.handle))
    trimmed = raw_logq_grad(kid, theta, X.ctypes.data, d, n, y.ctypes.data, ctx)
    for other in (again, device, trimmed):
        assert other[0] == host[0] and np.array_equal(other[1], host[1]) and other[2] == host[2]
    assert np.isfinite(host[1]).all()


def test_regression_gradient_keeps_its_bits_around_a_classification_call():
    """gprc_gpr_logp_grad and gprc_gpc_logq_grad share the context's workspace slots"""
    rng = np.random.default_rng(31)
    Xr = rng.uniform(-2, 2, (3, 1300))
    yr = np.sin(Xr.sum(0)) + 0.1 * rng.normal(size=1300)
    before = logp_grad(Xr, yr, 0.05, "rationalquadratic", [1.1, 1.7])
    name, theta, X, y = logq_case("ard3", 900)
    logq_grad(X, y, name, theta)
    after = logp_grad(Xr, yr, 0.05, "rationalquadratic", [1.1, 1.7])
    assert after[0] == before[0] and np.array_equal(after[1], before[1])


def test_profile_kinds_of_the_stages():
    name, theta, X, y = logq_case("ard3", 1100)
    nat.lib().gprc_prof_enable(1)
    nat.lib().gprc_prof_reset()
    try:
        logq_grad(X, y, name, theta)
        prof = nat.prof_summary()
    finally:
        nat.lib().gprc_prof_enable(0)
        nat.lib().gprc_prof_reset()
    assert prof["inverse_gemm"]["count"] >= 1 and prof["inverse_gemm"]["ms"] > 0
    assert prof["gpc_grad_contract"]["count"] == 1 and prof["gpc_grad_contract"]["ms"] > 0
    assert prof["grad_contract"]["count"] == 0


# ---- 5. errors --------------------------------------------------------------------------------------------------------------
def test_errors():
    X, y = gpc_problem(40, 2)
    ctx = nat.default_context()
    Xf = np.asfortranarray(X)
    for kid, par in ((nat.POLYNOMIAL, [1.0, 2.0]), (nat.LINEAR, [1.0]), (nat.CONSTANT, [1.0])):
        with pytest.raises(GprcError, match="logq_grad: defined for sqrexp, gammaexp, rationalquadratic and sqrexp_ard") as ei:
            raw_logq_grad(kid, par, Xf.ctypes.data, 2, 40, y.ctypes.data, ctx)
        assert ei.value.status == nat.ERR_ARG
    for bad in ([1.0, 0.0], [1.0, -1.0], [float("nan"), 1.0], [float("inf"), 1.0], [1.0], [1.0, 1.0, 1.0]):
        with pytest.raises(GprcError) as ei:
            raw_logq_grad(nat.SQREXP_ARD, bad, Xf.ctypes.data, 2, 40, y.ctypes.data, ctx)
        assert ei.value.status == nat.ERR_ARG and "sqrexp_ard" in ei.value.message
    for eps in (0.0, -1.0, float("nan")):
        with pytest.raises(GprcError) as ei:
            raw_logq_grad(nat.SQREXP, [1.0], Xf.ctypes.data, 2, 40, y.ctypes.data, ctx, epsilon=eps)
        assert ei.value.status == nat.ERR_ARG
    _, pp, npar = nat.params_array([1.0])
    g, lq = np.empty(1), C.c_double()
    gp = g.ctypes.data_as(C.POINTER(C.c_double))
    lib = nat.lib()
    assert lib.gprc_gpc_logq_grad(ctx.handle, nat.SQREXP, pp, npar, Xf.ctypes.data, 2, 40, y.ctypes.data, EPS, 0, None, gp, None) == nat.ERR_ARG
    assert lib.gprc_gpc_logq_grad(ctx.handle, nat.SQREXP, pp, npar, Xf.ctypes.data, 2, 40, y.ctypes.data, EPS, 0, C.byref(lq), None, None) == nat.ERR_ARG
    # a case that needs 6 steps, capped at 2
    name, theta, Xb, yb = logq_case("ard3", 600)
    _, _, iters = logq_reference(name, theta, Xb, yb)
    assert iters >= 6
    Xbf = np.asfortranarray(Xb)
    with pytest.raises(GprcError) as ei:
        raw_logq_grad(nat.SQREXP_ARD, theta, Xbf.ctypes.data, 3, 600, yb.ctypes.data, ctx, max_iter=2)
    assert ei.value.status == nat.ERR_MAXITER


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------
def test_optimize_gpc_end_to_end():
    rng = np.random.default_rng(13)
    n, nh, d = 800, 400, 4
    Xa = rng.uniform(-1, 1, (d, n + nh))
    ya = np.sign(Xa[0] - 0.5 * Xa[2] + 0.3 * rng.normal(size=n + nh))
    ya[ya == 0] = 1.0
    X, y, Xh, yh = Xa[:, :n], ya[:n], Xa[:, n:], ya[n:]
    start_value = logq_grad(X, y, "sqrexp_ard", np.ones(d))[0]
    r = optimize_gpc(X, y, "sqrexp_ard")
    iso = optimize_gpc(X, y, "sqrexp")
    print("optimize_gpc ard:", r["value"], r["par"], r["counts"], "start", start_value, "isotropic", iso["value"], iso["par"])
    assert r["convergence"] == 0 and iso["convergence"] == 0
    assert r["value"] >= start_value and r["value"] >= iso["value"]
    assert set(np.argsort(r["par"])[-2:]) == {1, 3}                  # the irrelevant coordinates get the two largest length scales
    gc = GPC(X, y, r["func"], EPS, reference_stop=False)
    dl = np.diag(gc.L)
    value = gc.logq + dl.sum() - np.log(dl).sum()
    assert abs(value - r["value"]) <= 1e-10 * abs(r["value"])
    from gprc_amd import cov_func, sqrexp_ard
    g1 = GPC(X, y, cov_func(sqrexp_ard, l=np.ones(d)), EPS, reference_stop=False)
    acc = lambda m: float(np.mean((m.predict_class(Xh) > 0.5) == (yh > 0)))   # noqa: E731
    print("held-out accuracy (400 points): fitted kernel", acc(gc), "start kernel l = 1", acc(g1))
    gc.close()
    g1.close()
