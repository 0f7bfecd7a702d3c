"""The Matern 3/2 and 5/2 kernels, isotropic and ARD (GPRC_MATERN32 .. GPRC_MATERN52_ARD), on the MI355X, through every entry point
that takes a kernel id.  The numpy references are the ones every kernel shares (tests/kernel_ref.py holds the formulas; they judge themselves in the CPU tests).

  1. fills           longdouble values rounded to float64, 1e-13 normwise (the fills' gate); bitwise symmetry, unit diagonal
  2. models          fit, predict (pointwise and full covariance), add_data against the float64 reference, TOL = 1e-10
  3. logp_grad       every kernel's check (tests/case_checks.py: the closed form, TOL; the parameter block also on its own) on the Matern rows
  4. logq_grad       against the book's form: cases of tests/test_gpu_gpc_grad.py::test_gradient_against_the_closed_form; here the tie
                     to the fitted classifier, every kernel's check likewise
  5. predict_grad    against the longdouble reference, 1e-10 on each of mean, variance and the two gradients; a test point ON a training point
  6. plumbing        pointer kinds, virtual ranks, refusals
  7. end to end      fit.optimize learns the length scales of matern52_ard
The oracle has no Matern kernel: no case here reads it (the shared checks consult it for the kernels it has).  Every reference factorisation is numpy's own: it raises when K_y is not positive
definite, so no case compares against a jittered matrix.
"""
import ctypes as C

import numpy as np
import pytest

import ard_grad_ref as LP
from case_checks import LOGP_CASES, check_logp_grad_against_the_closed_form, check_value_is_tied_to_the_fitted_classifier
import kernel_ref as K
import pred_grad_ref as G
from conftest import TOL, nerr
from gprc_amd import GPR, GPR_matern32, GPR_matern32_ard, GPR_matern52, GPR_matern52_ard, GprcError, covariance_matrix
from gprc_amd import _native as nat
from gprc_amd.fit import logp_grad, optimize
from gpu_calls import EPS, call_predict_grad, grad_problem, kfun, raw_logp_grad, step_time_limit  # noqa: F401  (the autouse fixture)

pytestmark = pytest.mark.gpu

LD = np.longdouble
GPR_CLASS = {"matern32": GPR_matern32, "matern52": GPR_matern52, "matern32_ard": GPR_matern32_ard, "matern52_ard": GPR_matern52_ard}


# ---- 1. fills ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 8, 17])
@pytest.mark.parametrize("name", K.MATERN_NAMES)
def test_fill_against_longdouble_values(name, d):
    rng = np.random.default_rng(300 + d)
    nA, nB = 333, 205                                                # neither a multiple of the 128 x 64 tile
    A, B = rng.uniform(-1, 1, (d, nA)), rng.uniform(-1, 1, (d, nB))
    par = rng.uniform(0.7, 2.0, d) if K.is_ard(name) else [1.3]
    k = kfun(name, par)
    want = np.asarray(K.pairwise(name, par, A, B, LD)[0], dtype=np.float64)
    got = covariance_matrix(A, B, k)
    assert got.shape == (nA, nB)
    e1, e2 = nerr(got, want), nerr(k(A[:, :nB], B), np.diag(want[:nB]))
    print(f"fill {name} d={d}: matrix {e1:.2e} colwise {e2:.2e} (gate 1e-13)")
    assert e1 <= 1e-13 and e2 <= 1e-13
    sym = covariance_matrix(A, A, k)
    assert np.array_equal(sym, sym.T) and np.all(np.diag(sym) == 1.0)
    assert np.all(k(A, A) == 1.0)                                    # s = 0 gives exactly 1 in the column-wise kernel too
    # all length scales equal: the isotropic kernel
    order = name[:8]
    e3 = nerr(covariance_matrix(A, B, kfun(order + "_ard", np.full(d, 1.3))), covariance_matrix(A, B, kfun(order, [1.3])))
    print(f"fill {order} d={d}: ard with equal length scales vs isotropic {e3:.2e} (gate 1e-13)")
    assert e3 <= 1e-13


# ---- 2. models --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [700, 1300])
@pytest.mark.parametrize("name,d", [("matern52", 3), ("matern52_ard", 5)])
def test_model_against_the_float64_reference(name, d, n):
    rng = np.random.default_rng(n + d)
    ns, noise = 200, 0.1
    X = rng.uniform(-1, 1, (d, n))
    y = 0.1 * (X ** 3).sum(0) + rng.normal(0, 0.1, n)
    Xs = rng.uniform(-1, 1, (d, ns))
    par = rng.uniform(0.7, 2.0, d) if K.is_ard(name) else np.array([1.1])
    f = LP.gpr_fit(name, par, X, y, noise)                            # numpy's Cholesky: raises unless K_y is positive definite as it stands
    assert np.isfinite(f["L"]).all()
    g = GPR_CLASS[name](X, y, noise, l=par if K.is_ard(name) else par[0])
    assert g.noise == noise                                          # no jitter on the device either
    errs = dict(alpha=nerr(g.alpha, f["alpha"]), logp=abs(g.logp - f["logp"]) / abs(f["logp"]), L=nerr(g.L, f["L"]))
    mr, cr = G.predict_cov(name, par, X, f["L"], f["alpha"], Xs)
    pr = g.predict(Xs)
    mean, cov = g.predict(Xs, pointwise_var=False)
    errs.update(mean=nerr(pr[:, 0], mr), var=nerr(pr[:, 1], np.diag(cr)), mean_full=nerr(np.ravel(mean), mr), cov=nerr(cov, cr))
    print(f"model {name} n={n}:", {k: f"{v:.2e}" for k, v in errs.items()}, "(gate 1e-10)")
    assert all(e <= TOL for e in errs.values()), errs
    # add_data of 37 points against a fresh fit
    Xn = rng.uniform(-1, 1, (d, 37))
    yn = 0.1 * (Xn ** 3).sum(0) + rng.normal(0, 0.1, 37)
    g.add_data(Xn, yn)
    fresh = GPR(np.hstack([X, Xn]), np.concatenate([y, yn]), noise, kfun(name, par))
    assert g.alpha.shape == (n + 37,)
    p1, p0 = g.predict(Xs), fresh.predict(Xs)
    e2 = dict(alpha=nerr(g.alpha, fresh.alpha), logp=abs(g.logp - fresh.logp) / abs(fresh.logp), L=nerr(g.L, fresh.L),
              mean=nerr(p1[:, 0], p0[:, 0]), var=nerr(p1[:, 1], p0[:, 1]))
    print(f"add_data {name} n={n}+37:", {k: f"{v:.2e}" for k, v in e2.items()}, "(gate 1e-10)")
    assert all(e <= TOL for e in e2.values()), e2
    g.close()
    fresh.close()


def test_default_length_scales_are_one():
    rng = np.random.default_rng(2)
    X = rng.uniform(-1, 1, (3, 300))
    y = 0.1 * (X ** 3).sum(0) + rng.normal(0, 0.1, 300)
    for name in K.MATERN_NAMES:
        g = GPR_CLASS[name](X, y, 0.1)
        assert nerr(g.alpha, LP.gpr_fit(name, np.ones(3 if K.is_ard(name) else 1), X, y, 0.1)["alpha"]) <= TOL
        g.close()


# ---- 3. logp_grad -----------------------------------------------------------------------------------------------------------
# n = 4100: 33 row tiles, 33 * 34 = 1122 tiles > 1024 workgroups -- the smallest size at which a workgroup carries its per-kernel
# accumulators (a0 of the isotropic kernels, gacc[] of the ARD ones) over two tiles
LOGP_RUNS = ([(name, n, noise) for n, noise in [(300, 0.1), (600, 0.01), (1100, 0.05)] for name in K.MATERN_NAMES]
             + [("matern52_ard8", 300, 0.1), ("matern32_ard17", 300, 0.1), ("matern52_ard17", 300, 0.1)]
             + [("matern52", 4100, 0.05), ("matern32_ard", 4100, 0.05)])        # (row of case_checks.LOGP_CASES, n, noise)


# the ids are kernel-n-noise-d, as they have been since these cases arrived
@pytest.mark.parametrize("case,n,noise", LOGP_RUNS, ids=["%s-%d-%g-%d" % (LOGP_CASES[c][0], n, noise, LOGP_CASES[c][2]) for c, n, noise in LOGP_RUNS])
def test_logp_grad_against_the_closed_form(case, n, noise):
    check_logp_grad_against_the_closed_form(case, n, noise)


# ---- 4. logq_grad -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.MATERN_NAMES)
def test_logq_value_is_tied_to_the_fitted_classifier(name):
    check_value_is_tied_to_the_fitted_classifier(name, 600)


# ---- 5. predict_grad --------------------------------------------------------------------------------------------------------
# d = 17: three coordinate groups (blockIdx.z), the last of one coordinate, with ARD scaling
PRED_CASES = ([(case, size) for case in K.MATERN_CASES for size in K.SIZES]
              + [(("matern52_ard", list(np.linspace(1.0, 3.0, 17) * np.sqrt(17 / 3)), 17), (300, 0.1))])


def pred_case_id(cs):
    case, (n, noise) = cs
    return "%s-d%d-n%d-noise%g" % (case[0], case[2], n, noise)


@pytest.mark.parametrize("cs", PRED_CASES, ids=pred_case_id)
def test_predict_grad_against_the_longdouble_reference(cs):
    case, (n, noise) = cs
    name, par, d = case
    X, y, Xs = G.make_case(case, n, m=40)                            # test point 0 IS training point 5
    assert np.array_equal(Xs[:, 0], X[:, 5])
    ref = G.predict_grad(name, par, X, y, noise, Xs, LD)             # pred_grad_ref.chol asserts every pivot > 0
    g = GPR(X, y, noise, kfun(name, par))
    assert g.noise == noise
    got = call_predict_grad(g, Xs)
    for what, a, b in zip(("mean", "var", "dmean", "dvar"), got, ref):
        e = G.nerr(np.asarray(a, dtype=LD), b)
        print("predict_grad %s n %d %s %.2e (gate 1e-10)" % (K.case_id(case) if d < 17 else name + "-d17", n, what, e))
        assert np.isfinite(a).all() and e <= 1e-10, (what, e)
    pred = g.predict(Xs)
    assert np.array_equal(got[0], pred[:, 0]) and np.array_equal(got[1], pred[:, 1])    # the bits of gprc_gpr_predict(pointwise = 1)
    only_dmean = call_predict_grad(g, Xs, mean=False, var=False, dvar=False)     # the mean's gradient alone: one pass, no solve
    assert only_dmean[0] is None and only_dmean[3] is None and np.array_equal(only_dmean[2], got[2])
    pa, dm, dv = g.predict_grad(Xs)                                  # the public method is the same call
    assert np.array_equal(pa, pred) and np.array_equal(dm, got[2]) and np.array_equal(dv, got[3])
    g.close()


# ---- 6. plumbing ------------------------------------------------------------------------------------------------------------
def test_pointer_kinds_repeat_calls_and_trim_give_the_same_bits():
    torch = pytest.importorskip("torch")
    X, y, theta = grad_problem(1100, 3)
    X = np.asfortranarray(X)
    d, n = X.shape
    kid = nat.MATERN52_ARD
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


def test_virtual_ranks_give_the_single_gpu_model():
    """gprc_mgpu_* (and through them the device-level fills) take the new ids: bitwise the single-GPU object"""
    rng = np.random.default_rng(9)
    d, n, ns = 4, 1300, 150
    X = rng.uniform(-1, 1, (d, n))
    y = 0.1 * (X ** 3).sum(0) + rng.normal(0, 0.1, n)
    Xs = rng.uniform(-1, 1, (d, ns))
    ell = rng.uniform(0.7, 2.0, d)
    k = kfun("matern32_ard", ell)
    one = GPR(X, y, 0.1, k)
    two = GPR(X, y, 0.1, k, devices=[0, 0])
    assert np.array_equal(two.alpha, one.alpha) and two.logp == one.logp
    assert np.array_equal(two.predict(Xs), one.predict(Xs))
    assert nerr(two.alpha, LP.gpr_fit("matern32_ard", ell, X, y, 0.1)["alpha"]) <= TOL
    two.close()
    one.close()


def test_refusals_through_the_raw_abi():
    rng = np.random.default_rng(5)
    X = np.asfortranarray(rng.uniform(-1, 1, (2, 40)))
    y = rng.normal(size=40)
    ys = np.sign(y)
    ctx = nat.default_context()
    lib = nat.lib()
    out = np.empty((40, 40), order="F")
    bad_ard = ([1.0, 0.0], [1.0, -1.0], [float("nan"), 1.0], [float("inf"), 1.0], [1.0], [1.0, 1.0, 1.0])       # the last two: n_params != d
    bad_iso = ([0.0], [-1.0], [float("nan")], [float("inf")], [1.0, 1.0], [])                                      # the last two: n_params != 1
    for name in K.MATERN_NAMES:
        kid = K.KERNEL_ID[name]
        for bad in (bad_ard if K.is_ard(name) else bad_iso):
            _, pp, npar = nat.params_array(bad)
            rc = lib.gprc_kernel_matrix(ctx.handle, kid, pp, npar, X.ctypes.data, 2, 40, X.ctypes.data, 40, out.ctypes.data, 40)
            assert rc == nat.ERR_ARG and name + ":" in nat.last_error(), (name, bad, nat.last_error())
            with pytest.raises(GprcError) as ei:
                raw_logp_grad(kid, bad, X.ctypes.data, 2, 40, y.ctypes.data, 0.1, ctx)
            assert ei.value.status == nat.ERR_ARG and name + ":" in ei.value.message
            g, lq = np.empty(max(npar, 1)), C.c_double()
            rc = lib.gprc_gpc_logq_grad(ctx.handle, kid, pp, npar, X.ctypes.data, 2, 40, ys.ctypes.data, EPS, 0, C.byref(lq),
                                        g.ctypes.data_as(C.POINTER(C.c_double)), None)
            assert rc == nat.ERR_ARG and name + ":" in nat.last_error()
    # the reference's own fit() gradient (dens_deriv) stays the reference's: it knows no Matern kernel
    _, pp, npar = nat.params_array([1.0])
    g = np.empty(1)
    rc = lib.gprc_fit_gradient(ctx.handle, nat.MATERN52, pp, npar, X.ctypes.data, 2, 40, y.ctypes.data, g.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == nat.ERR_ARG
    # the gradients' refusal of the kernels without one now lists the Matern names after the four it always listed
    with pytest.raises(GprcError, match="logp_grad: defined for sqrexp, gammaexp, rationalquadratic and sqrexp_ard, matern32, matern52, matern32_ard and matern52_ard"):
        raw_logp_grad(nat.POLYNOMIAL, [1.0, 2.0], X.ctypes.data, 2, 40, y.ctypes.data, 0.1, ctx)


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------
def test_optimize_end_to_end():
    """the problem of tests/test_gpu_ard_grad.py::test_optimize_end_to_end with the standard prior of Bayesian optimisation"""
    rng = np.random.default_rng(11)
    n, d = 800, 4
    X = rng.uniform(-2, 2, (d, n))
    y = np.sin(2 * X[0]) + 0.5 * X[2] ** 2 + 0.1 * rng.normal(size=n)
    start_value = logp_grad(X, y, 0.1, "matern52_ard", np.ones(d))[0]
    r = optimize(X, y, 0.1, "matern52_ard")
    print("optimize matern52_ard:", r["value"], r["par"], r["noise"], r["counts"], "start", start_value)
    assert r["convergence"] == 0
    assert r["value"] >= start_value
    assert set(np.argsort(r["par"])[-2:]) == {1, 3}                  # the irrelevant coordinates get the two largest length scales
    assert r["func"].gprc_kernel[0] == nat.MATERN52_ARD
    g = GPR(X, y, r["noise"], r["func"])
    assert g.noise == r["noise"]
    assert abs(g.logp - r["value"]) <= 1e-10 * abs(r["value"])
    g.close()
