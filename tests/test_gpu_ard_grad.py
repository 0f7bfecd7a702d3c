"""Exact marginal-likelihood gradient (gprc_gpr_logp_grad) and the ARD squared exponential on the MI355X.

ARD values and models against the CPU oracle's isotropic squared exponential on the scaled inputs X / l (the fills' 1e-13 and the
north-star 1e-10 gates); the gradient of every kernel of fit.grad_dict against the numpy float64 closed form of tests/ard_grad_ref.py
(1e-10 normwise) and against central differences of the library's own gprc_gpr_log_marginal (1e-6); pointer kinds, determinism, errors;
fit.optimize end to end.

Every gradient case of a kernel the oracle has asserts that the oracle's fit of it succeeds at the FIRST attempt; the oracle has no Matern
kernel, and there numpy's Cholesky of K_y as it stands is the precondition (it raises).  No case tests a jittered matrix.
"""
import numpy as np
import pytest

from conftest import TOL, nerr
from gprc_amd import (GPC, GPR, GPR_sqrexp_ard, GprcError, NotPositiveDefinite, cov_func, covariance_matrix, sqrexp, sqrexp_ard)
from gprc_amd import _native as nat
from case_checks import check_logp_grad_against_the_closed_form, logp_case
from gprc_amd.fit import dens, logp_grad, optimize
from gpu_calls import grad_problem, raw_logp_grad, step_time_limit  # noqa: F401  (the autouse fixture)
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


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
# (the Matern rows of case_checks.LOGP_CASES run at their own sizes, under the names they have always had, in tests/test_gpu_matern.py)
@pytest.mark.parametrize("case,n,noise", [(c, n, noise) for n, noise in [(300, 0.1), (600, 0.01), (3000, 0.05), (5000, 0.05)]
                                          for c in ["sqrexp", "gammaexp1.5", "gammaexp1", "ratquad", "ard3", "ard8"]]
                         + [(c, 300, 0.1) for c in ["ard17", "sqrexp_d17", "ard33"]])
def test_gradient_against_the_closed_form(case, n, noise):
    check_logp_grad_against_the_closed_form(case, n, noise)


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
@pytest.mark.parametrize("case", ["ard8", "gammaexp1.5"])
def test_pointer_kinds_repeat_calls_and_trim_give_the_same_bits(case):
    torch = pytest.importorskip("torch")
    name, theta, X, y, _ = logp_case(case, 1100)
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
    name, theta, X, y, _ = logp_case("ard3", 1100)
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
