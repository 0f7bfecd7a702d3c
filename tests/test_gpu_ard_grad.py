"""Exact marginal-likelihood gradient (gprc_gpr_logp_grad) and the ARD squared exponential on the MI355X.

ARD values and models against the CPU oracle's isotropic squared exponential on the scaled inputs X / l (the fills' 1e-13 and the
north-star 1e-10 gates); the gradient against the numpy float64 closed form of tests/ard_grad_ref.py (1e-10 normwise) and against
central differences of the library's own gprc_gpr_log_marginal (1e-6); pointer kinds, determinism, errors; fit.optimize end to end.

Every gradient case asserts that the oracle's fit of it succeeds at the FIRST attempt: no case tests a jittered matrix.
"""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import ard_grad_ref as ref
from conftest import TOL, nerr
from gprc_amd import (GPC, GPR, GPR_sqrexp_ard, GprcError, NotPositiveDefinite, cov_func, covariance_matrix, sqrexp, sqrexp_ard)
from gprc_amd import _native as nat
from gprc_amd.fit import dens, logp_grad, optimize
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

STEP_LIMIT_S = 900   # a hung step ends the process (with every thread's traceback) instead of holding the GPU


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# ---- 1. ARD values ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 8, 100])
def test_ard_kernel_values_equal_the_isotropic_kernel_on_scaled_inputs(d):
    rng = np.random.default_rng(200 + d)
    nA, nB = 333, 205                                                # neither a multiple of the 128 x 64 tile
    A, B = rng.uniform(-1, 1, (d, nA)), rng.uniform(-1, 1, (d, nB))
    ell = rng.uniform(0.7, 2.0, d)
    k = cov_func(sqrexp_ard, l=ell)
    want = orc.kernel_matrix(orc.SQREXP, [1.0], A / ell[:, None], B / ell[:, None])
    got = covariance_matrix(A, B, k)
    assert got.shape == (nA, nB)
    e1, e2 = nerr(got, want), nerr(k(A[:, :nB], B), np.diag(want[:nB]))
    print("ard fill / colwise vs oracle on scaled inputs:", d, e1, e2)
    assert e1 <= 1e-13 and e2 <= 1e-13
    sym = covariance_matrix(A, A, k)
    assert np.array_equal(sym, sym.T) and np.all(np.diag(sym) == 1.0)
    # all length scales equal: the isotropic kernel on the unscaled inputs
    keq = cov_func(sqrexp_ard, l=np.full(d, 1.3))
    want = orc.kernel_matrix(orc.SQREXP, [1.3], A, B)
    e1, e2 = nerr(covariance_matrix(A, B, keq), want), nerr(keq(A[:, :nB], B), np.diag(want[:nB]))
    print("ard with equal length scales vs isotropic:", d, e1, e2)
    assert e1 <= 1e-13 and e2 <= 1e-13
    assert nerr(covariance_matrix(A, B, keq), covariance_matrix(A, B, cov_func(sqrexp, l=1.3))) <= 1e-13


# ---- 2. ARD model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [700, 3000])
def test_ard_model_against_oracle_on_scaled_inputs(n):
    rng = np.random.default_rng(n)
    d, ns, noise = 5, 200, 0.1
    X = rng.uniform(-1, 1, (d, n))
    y = 0.1 * (X ** 3).sum(0) + rng.normal(0, 0.1, n)
    Xs = rng.uniform(-1, 1, (d, ns))
    ell = rng.uniform(0.7, 2.0, d)
    Xl, Xsl = X / ell[:, None], Xs / ell[:, None]
    f = orc.gpr_fit(orc.SQREXP, [1.0], Xl, y, noise)
    assert f["attempts"] == 1
    g = GPR_sqrexp_ard(X, y, noise, l=ell)
    assert g.noise == noise
    assert nerr(g.alpha, f["alpha"]) <= TOL and abs(g.logp - f["logp"]) <= TOL * abs(f["logp"]) and nerr(g.L, f["L"]) <= TOL
    mr, vr = orc.gpr_predict(orc.SQREXP, [1.0], Xl, f["L"], f["alpha"], Xsl)
    pr = g.predict(Xs)
    assert nerr(pr[:, 0], mr) <= TOL and nerr(pr[:, 1], vr) <= TOL
    mean, cov = g.predict(Xs, pointwise_var=False)
    _, cr = orc.gpr_predict(orc.SQREXP, [1.0], Xl, f["L"], f["alpha"], Xsl, pointwise=False)
    assert nerr(np.ravel(mean), mr) <= TOL and nerr(cov, cr) <= TOL
    # add_data of 37 points against a fresh fit
    Xn = rng.uniform(-1, 1, (d, 37))
    yn = 0.1 * (Xn ** 3).sum(0) + rng.normal(0, 0.1, 37)
    g.add_data(Xn, yn)
    fresh = GPR_sqrexp_ard(np.hstack([X, Xn]), np.concatenate([y, yn]), noise, l=ell)
    assert g.alpha.shape == (n + 37,)
    assert nerr(g.alpha, fresh.alpha) <= TOL and abs(g.logp - fresh.logp) <= TOL * abs(fresh.logp) and nerr(g.L, fresh.L) <= TOL
    p1, p0 = g.predict(Xs), fresh.predict(Xs)
    assert nerr(p1[:, 0], p0[:, 0]) <= TOL and nerr(p1[:, 1], p0[:, 1]) <= TOL
    m1, c1 = g.predict(Xs, pointwise_var=False)
    m0, c0 = fresh.predict(Xs, pointwise_var=False)
    assert nerr(m1, m0) <= TOL and nerr(c1, c0) <= TOL
    g.close()
    fresh.close()
    # the default: every length scale 1
    g1 = GPR_sqrexp_ard(X[:, :300], y[:300], noise)
    f1 = orc.gpr_fit(orc.SQREXP, [1.0], X[:, :300], y[:300], noise)
    assert nerr(g1.alpha, f1["alpha"]) <= TOL
    g1.close()


# ---- 3. gradient against the closed form ------------------------------------------------------------------------------------
def grad_problem(n, d):
    rng = np.random.default_rng(1000 + n + d)
    X = rng.uniform(-2, 2, (d, n))
    y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
    return X, y, rng.uniform(0.7, 2.0, d)


def grad_case(case, n):
    """(name, theta, oracle kernel id, oracle params, oracle inputs, X, y) of a named case at size n"""
    if case.startswith("ard"):
        d = int(case[3:])
        X, y, ell = grad_problem(n, d)
        if d > 16:
            ell = ell * np.sqrt(d / 3)       # (see WIDE_CASES)
        return "sqrexp_ard", ell, orc.SQREXP, [1.0], X / ell[:, None], X, y
    if case == "sqrexp_d17":
        X, y, _ = grad_problem(n, 17)
        theta = np.array([1.3 * np.sqrt(17 / 3)])
        return "sqrexp", theta, orc.SQREXP, list(theta), X, X, y
    name, theta = {"sqrexp": ("sqrexp", [1.3]), "gammaexp1.5": ("gammaexp", [0.9, 1.5]), "gammaexp1": ("gammaexp", [1.2, 1.0]),
                   "ratquad": ("rationalquadratic", [1.1, 1.7])}[case]
    X, y, _ = grad_problem(n, 3)
    return name, np.array(theta), orc.KERNEL_IDS[name], list(theta), X, X, y


# d > 16: the contraction stages the coordinates 16 at a time, so d = 17 takes two passes and d = 33 three, the last of one coordinate
# each, and ARD stages them again for its second pass.  The length scales are multiplied by sqrt(d / 3): at the scales of d = 3 the
# kernel matrix of 17 coordinates is nearly the identity, the length-scale gradient is ~1e-2 of the noise derivative and a normwise
# bound over the whole vector would hide a wrong coordinate.  With the scaling (numpy reference, ard17, n = 300, noise 0.1):
# max |d/dl| = 1.39, min |d/dl| = 0.018, d/dnoise = -28.9; these cases also bound the parameter block on its own.
WIDE_CASES = ["ard17", "sqrexp_d17", "ard33"]


@pytest.mark.parametrize("case,n,noise", [(c, n, noise) for n, noise in [(300, 0.1), (600, 0.01), (3000, 0.05), (5000, 0.05)]
                                          for c in ["sqrexp", "gammaexp1.5", "gammaexp1", "ratquad", "ard3", "ard8"]]
                         + [(c, 300, 0.1) for c in WIDE_CASES])
def test_gradient_against_the_closed_form(case, n, noise):
    name, theta, kid, opar, Xo, X, y = grad_case(case, n)
    assert orc.gpr_fit(kid, opar, Xo, y, noise)["attempts"] == 1
    want_logp, want = ref.logp_grad(name, theta, X, y, noise)
    logp, grad = logp_grad(X, y, noise, name, theta)
    assert grad.shape == (theta.size + 1,)
    e = nerr(grad, want)
    print(f"logp_grad {case} n={n} noise={noise}: nerr(grad)={e:.3e} rel(logp)={abs(logp - want_logp) / abs(want_logp):.3e}")
    assert e <= TOL
    if case in WIDE_CASES:
        eb = nerr(grad[:-1], want[:-1])
        print(f"logp_grad {case} n={n}: nerr(parameter block)={eb:.3e} max|d/dtheta|={np.abs(want[:-1]).max():.3g} "
              f"min|d/dtheta|={np.abs(want[:-1]).min():.3g} d/dnoise={want[-1]:.3g}")
        assert eb <= TOL
    assert abs(logp - want_logp) <= TOL * abs(want_logp)
    assert logp == dens(X, y, noise, name, theta)          # the value is the existing objective, bit for bit


# ---- 4. gradient against differences of the library's own value -------------------------------------------------------------
def test_gradient_against_differences_of_log_marginal():
    X, y, ell = grad_problem(3000, 8)
    noise = 0.05
    _, grad = logp_grad(X, y, noise, "sqrexp_ard", ell)
    fd = np.empty(9)
    for k in range(8):
        e = np.zeros(8)
        e[k] = 1e-5 * ell[k]
        fd[k] = (dens(X, y, noise, "sqrexp_ard", ell + e) - dens(X, y, noise, "sqrexp_ard", ell - e)) / (2 * e[k])
    h = 1e-5 * noise
    fd[8] = (dens(X, y, noise + h, "sqrexp_ard", ell) - dens(X, y, noise - h, "sqrexp_ard", ell)) / (2 * h)
    err = nerr(grad, fd)
    print("logp_grad vs central differences of gprc_gpr_log_marginal:", err)
    assert err <= 1e-6


# ---- 5. pointer kinds and determinism ---------------------------------------------------------------------------------------
def raw_logp_grad(kid, theta, Xptr, d, n, yptr, noise, ctx):
    _, pp, npar = nat.params_array(theta)
    g, lp = np.empty(npar + 1), C.c_double()
    nat.check(nat.lib().gprc_gpr_logp_grad(ctx.handle, kid, pp, npar, Xptr, d, n, yptr, noise, C.byref(lp), g.ctypes.data_as(C.POINTER(C.c_double))))
    return lp.value, g


@pytest.mark.parametrize("case", ["ard8", "gammaexp1.5"])
def test_pointer_kinds_repeat_calls_and_trim_give_the_same_bits(case):
    torch = pytest.importorskip("torch")
    name, theta, *_, X, y = grad_case(case, 1100)
    X = np.asfortranarray(X)
    d, n = X.shape
    kid = {"sqrexp_ard": nat.SQREXP_ARD, "gammaexp": nat.GAMMAEXP}[name]
    ctx = nat.default_context()
    host = raw_logp_grad(kid, theta, X.ctypes.data, d, n, y.ctypes.data, 0.05, ctx)
    again = raw_logp_grad(kid, theta, X.ctypes.data, d, n, y.ctypes.data, 0.05, ctx)
    dev = torch.device("cuda:0")
    Xd, yd = torch.from_numpy(X.T.copy()).to(dev), torch.from_numpy(y).to(dev)
    torch.cuda.synchronize()
    device = raw_logp_grad(kid, theta, Xd.data_ptr(), d, n, yd.data_ptr(), 0.05, ctx)
    nat.check(nat.lib().gprc_ctx_trim(ctx.handle))
    trimmed = raw_logp_grad(kid, theta, X.ctypes.data, d, n, y.ctypes.data, 0.05, ctx)
    for other in (again, device, trimmed):
        assert other[0] == host[0] and np.array_equal(other[1], host[1])
    assert np.isfinite(host[1]).all()


def test_profile_kinds_of_the_new_stages():
    name, theta, *_, X, y = grad_case("ard3", 1100)
    nat.lib().gprc_prof_enable(1)
    nat.lib().gprc_prof_reset()
    try:
        logp_grad(X, y, 0.05, name, theta)
        prof = nat.prof_summary()
    finally:
        nat.lib().gprc_prof_enable(0)
        nat.lib().gprc_prof_reset()
    assert prof["inverse_gemm"]["count"] >= 1 and prof["inverse_gemm"]["ms"] > 0
    assert prof["grad_contract"]["count"] == 1 and prof["grad_contract"]["ms"] > 0


# ---- 6. errors --------------------------------------------------------------------------------------------------------------
def test_errors():
    rng = np.random.default_rng(5)
    X = rng.uniform(-1, 1, (2, 40))
    y = rng.normal(size=40)
    Xdup = np.hstack([X, X[:, :3]])                                   # duplicate points, noise 0: singular
    with pytest.raises(NotPositiveDefinite):
        logp_grad(Xdup, np.concatenate([y, y[:3]]), 0.0, "sqrexp_ard", [1.0, 1.0])
    ctx = nat.default_context()
    Xf = np.asfortranarray(X)
    for kid, par in ((nat.POLYNOMIAL, [1.0, 2.0]), (nat.LINEAR, [1.0]), (nat.CONSTANT, [1.0])):
        with pytest.raises(GprcError, match="logp_grad: defined for sqrexp, gammaexp, rationalquadratic and sqrexp_ard") as ei:
            raw_logp_grad(kid, par, Xf.ctypes.data, 2, 40, y.ctypes.data, 0.1, ctx)
        assert ei.value.status == nat.ERR_ARG
    for bad in ([1.0, 0.0], [1.0, -1.0], [float("nan"), 1.0], [float("inf"), 1.0], [1.0], [1.0, 1.0, 1.0]):
        with pytest.raises(GprcError) as ei:
            raw_logp_grad(nat.SQREXP_ARD, bad, Xf.ctypes.data, 2, 40, y.ctypes.data, 0.1, ctx)
        assert ei.value.status == nat.ERR_ARG and "sqrexp_ard" in ei.value.message
        out = np.empty((40, 40), order="F")
        _, pp, npar = nat.params_array(bad)
        rc = nat.lib().gprc_kernel_matrix(ctx.handle, nat.SQREXP_ARD, pp, npar, Xf.ctypes.data, 2, 40, Xf.ctypes.data, 40, out.ctypes.data, 40)
        assert rc == nat.ERR_ARG


def test_ard_in_gpc_against_oracle_on_scaled_inputs():
    """gprc_gpc_* take the ARD kernel like any other (the fills are shared)."""
    rng = np.random.default_rng(4)
    X = rng.uniform(-1, 1, (3, 600))
    y = np.sign(X[0] - 0.5 * X[1] + 0.2 * rng.normal(size=600))
    y[y == 0] = 1.0
    Xs = rng.uniform(-1, 1, (3, 41))
    ell = np.array([0.8, 1.1, 1.9])
    Xl, Xsl = X / ell[:, None], Xs / ell[:, None]
    oc = orc.gpc_fit(orc.SQREXP, [1.0], Xl, y, 1e-5, divergence_stop=False)
    gc = GPC(X, y, cov_func(sqrexp_ard, l=ell), 1e-5, reference_stop=False)
    assert gc.iterations == oc["iters"]
    assert nerr(gc.f_hat, oc["f_hat"]) <= TOL and abs(gc.logq - oc["logq"]) <= TOL * abs(oc["logq"]) and nerr(gc.L, oc["L"]) <= TOL
    fs, vf = gc.predict_latent(Xs)
    ofs, ovf = orc.gpc_predict_latent(orc.SQREXP, [1.0], Xl, y, oc["f_hat"], oc["L"], Xsl)
    assert nerr(fs, ofs) <= TOL and nerr(vf, ovf) <= TOL


def test_ard_over_virtual_ranks_is_the_single_gpu_model():
    """gprc_mgpu_* (and through them gprc_dev_fill_panel / gprc_dev_fill_cross / gprc_gpr_model_from_device) take the ARD kernel:
    bitwise the single-GPU object, which test_ard_model_against_oracle_on_scaled_inputs ties to the oracle."""
    rng = np.random.default_rng(9)
    d, n, ns = 4, 1300, 150
    X = rng.uniform(-1, 1, (d, n))
    y = 0.1 * (X ** 3).sum(0) + rng.normal(0, 0.1, n)
    Xs = rng.uniform(-1, 1, (d, ns))
    ell = rng.uniform(0.7, 2.0, d)
    k = cov_func(sqrexp_ard, l=ell)
    one = GPR(X, y, 0.1, k)
    two = GPR(X, y, 0.1, k, devices=[0, 0])
    assert np.array_equal(two.alpha, one.alpha) and two.logp == one.logp
    assert np.array_equal(two.predict(Xs), one.predict(Xs))
    f = orc.gpr_fit(orc.SQREXP, [1.0], X / ell[:, None], y, 0.1)
    assert nerr(two.alpha, f["alpha"]) <= TOL
    two.close()
    one.close()


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------
def test_optimize_end_to_end():
    rng = np.random.default_rng(11)
    n, d = 800, 4
    X = rng.uniform(-2, 2, (d, n))
    y = np.sin(2 * X[0]) + 0.5 * X[2] ** 2 + 0.1 * rng.normal(size=n)
    start_value = logp_grad(X, y, 0.1, "sqrexp_ard", np.ones(d))[0]
    r = optimize(X, y, 0.1, "sqrexp_ard")
    iso = optimize(X, y, 0.1, "sqrexp")
    print("optimize ard:", r["value"], r["par"], r["noise"], r["counts"], "start", start_value, "isotropic", iso["value"], iso["par"])
    assert r["convergence"] == 0 and iso["convergence"] == 0
    assert r["value"] >= start_value and r["value"] >= iso["value"]
    assert set(np.argsort(r["par"])[-2:]) == {1, 3}                  # the irrelevant coordinates get the two largest length scales
    g = GPR(X, y, r["noise"], r["func"])
    assert g.noise == r["noise"]
    assert abs(g.logp - r["value"]) <= 1e-10 * abs(r["value"])
    g.close()
    # gammaexp moves away from its start (1, 1) with a finite gradient and a higher value: the reference-faithful path cannot
    v0, g0 = logp_grad(X, y, 0.1, "gammaexp", [1.0, 1.0])
    assert np.isfinite(g0).all()
    ge = optimize(X, y, 0.1, "gammaexp")
    print("optimize gammaexp:", ge["value"], ge["par"], ge["noise"], ge["counts"], "start", v0)
    assert ge["value"] > v0 and tuple(ge["par"]) != (1.0, 1.0) and np.isfinite(ge["par"]).all()
