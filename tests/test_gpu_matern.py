"""The Matern 3/2 and 5/2 kernels, isotropic and ARD (GPRC_MATERN32 .. GPRC_MATERN52_ARD), on the MI355X through every entry point that
takes a kernel id, against tests/matern_ref.py (numpy, written from the formulas; it judges itself in tests/test_matern_cpu.py).

  1. fills           longdouble values rounded to float64, 1e-13 normwise (the fills' gate); bitwise symmetry, unit diagonal
  2. models          fit, predict (pointwise and full covariance), add_data against the float64 reference, TOL = 1e-10
  3. logp_grad       against the closed form, TOL; the parameter block also on its own (the noise entry dominates the norm)
  4. logq_grad       against the book's per-parameter form, TOL, with the two preconditions of tests/test_gpu_gpc_grad.py on the reference
  5. predict_grad    against the longdouble reference, 1e-10 on each of mean, variance and the two gradients; a test point ON a training point
  6. plumbing        pointer kinds, virtual ranks, refusals
  7. end to end      fit.optimize learns the length scales of matern52_ard
The oracle has no Matern kernel: nothing here reads it.  Every reference factorisation is numpy's or pred_grad_ref.chol's own: it raises
(asserts) when K_y is not positive definite, so no case compares against a jittered matrix.
"""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import matern_ref as M
import pred_grad_ref as G
from conftest import TOL, nerr
from gprc_amd import (GPC, GPR, GPR_matern32, GPR_matern32_ard, GPR_matern52, GPR_matern52_ard, CovFunc, GprcError, cov_func,
                      covariance_matrix, matern32, matern32_ard, matern52, matern52_ard)
from gprc_amd import _native as nat
from gprc_amd.fit import dens, grad_dict, logp_grad, logq_grad, optimize

pytestmark = pytest.mark.gpu

STEP_LIMIT_S = 900   # a hung step ends the process (with every thread's traceback) instead of holding the GPU
EPS = 1e-10
LD = np.longdouble
GENERIC = {"matern32": matern32, "matern52": matern52, "matern32_ard": matern32_ard, "matern52_ard": matern52_ard}
GPR_CLASS = {"matern32": GPR_matern32, "matern52": GPR_matern52, "matern32_ard": GPR_matern32_ard, "matern52_ard": GPR_matern52_ard}


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def kfun(name, par):
    par = np.atleast_1d(np.asarray(par, dtype=float))
    return cov_func(GENERIC[name], l=par if M.is_ard(name) else float(par[0]))


# ---- 1. fills ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 8, 17])
@pytest.mark.parametrize("name", M.NAMES)
def test_fill_against_longdouble_values(name, d):
    rng = np.random.default_rng(300 + d)
    nA, nB = 333, 205                                                # neither a multiple of the 128 x 64 tile
    A, B = rng.uniform(-1, 1, (d, nA)), rng.uniform(-1, 1, (d, nB))
    par = rng.uniform(0.7, 2.0, d) if M.is_ard(name) else [1.3]
    k = kfun(name, par)
    want = np.asarray(M.kernel_and_h(name, par, A, B, LD)[0], dtype=np.float64)
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
    par = rng.uniform(0.7, 2.0, d) if M.is_ard(name) else np.array([1.1])
    f = M.gpr_fit(name, par, X, y, noise)                            # numpy's Cholesky: raises unless K_y is positive definite as it stands
    assert np.isfinite(f["L"]).all()
    g = GPR_CLASS[name](X, y, noise, l=par if M.is_ard(name) else par[0])
    assert g.noise == noise                                          # no jitter on the device either
    errs = dict(alpha=nerr(g.alpha, f["alpha"]), logp=abs(g.logp - f["logp"]) / abs(f["logp"]), L=nerr(g.L, f["L"]))
    mr, cr = M.predict_cov(name, par, X, f["L"], f["alpha"], Xs)
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
    for name in M.NAMES:
        g = GPR_CLASS[name](X, y, 0.1)
        assert nerr(g.alpha, M.gpr_fit(name, np.ones(3 if M.is_ard(name) else 1), X, y, 0.1)["alpha"]) <= TOL
        g.close()


# ---- 3. logp_grad -----------------------------------------------------------------------------------------------------------
def grad_problem(n, d):
    """the inputs of tests/test_gpu_ard_grad.py"""
    rng = np.random.default_rng(1000 + n + d)
    X = rng.uniform(-2, 2, (d, n))
    y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
    return X, y, rng.uniform(0.7, 2.0, d)


def grad_case(name, n, d):
    """(theta, X, y).  d > 16: the length scales are multiplied by sqrt(d / 3) -- at the scales of d = 3 the kernel matrix of 17
    coordinates is nearly the identity and the length-scale gradient would vanish beside the noise derivative."""
    X, y, ell = grad_problem(n, d)
    theta = ell if M.is_ard(name) else np.array([0.9 if name == "matern32" else 1.1])
    if d > 16:
        theta = theta * np.sqrt(d / 3)
    return theta, X, y


# n = 4100: 33 row tiles, 33 * 34 = 1122 tiles > 1024 workgroups -- the smallest size at which a workgroup carries its per-kernel
# accumulators (a0 of the isotropic kernels, gacc[] of the ARD ones) over two tiles
LOGP_CASES = ([(name, n, noise, 3) for n, noise in [(300, 0.1), (600, 0.01), (1100, 0.05)] for name in M.NAMES]
              + [("matern52_ard", 300, 0.1, 8), ("matern32_ard", 300, 0.1, 17), ("matern52_ard", 300, 0.1, 17)]
              + [("matern52", 4100, 0.05, 3), ("matern32_ard", 4100, 0.05, 3)])


@pytest.mark.parametrize("name,n,noise,d", LOGP_CASES)
def test_logp_grad_against_the_closed_form(name, n, noise, d):
    theta, X, y = grad_case(name, n, d)
    want_logp, want = M.logp_grad(name, theta, X, y, noise)          # numpy's Cholesky of K_y as it stands
    logp, grad = logp_grad(X, y, noise, name, theta)
    assert grad.shape == (theta.size + 1,)
    e, eb = nerr(grad, want), nerr(grad[:-1], want[:-1])
    print(f"logp_grad {name} n={n} d={d} noise={noise}: nerr(grad)={e:.3e} nerr(parameter block)={eb:.3e} "
          f"rel(logp)={abs(logp - want_logp) / abs(want_logp):.3e} max|d/dtheta|={np.abs(want[:-1]).max():.3g} "
          f"min|d/dtheta|={np.abs(want[:-1]).min():.3g} d/dnoise={want[-1]:.3g} (gate 1e-10)")
    assert e <= TOL
    assert eb <= TOL
    assert abs(logp - want_logp) <= TOL * abs(want_logp)
    assert logp == dens(X, y, noise, name, theta)                    # the value is the existing objective, bit for bit


# ---- 4. logq_grad -----------------------------------------------------------------------------------------------------------
def gpc_problem(n, d):
    """the inputs of tests/test_gpu_gpc_grad.py"""
    rng = np.random.default_rng(7000 + n + d)
    X = rng.uniform(-1, 1, (d, n))
    y = np.sign(X[0] - 0.5 * X[d - 1] + 0.3 * rng.normal(size=n))
    y[y == 0] = 1.0
    return X, y


GPC_THETA = {"matern32": [0.8], "matern52": [0.9], "matern32_ard": [0.8, 1.1, 1.9], "matern52_ard": [0.8, 1.1, 1.9]}
# d = 17: two passes over the coordinates, ARD stages them again for its second pass; length scales times sqrt(17 / 3) as above
GPC_WIDE = [("matern52_ard", np.linspace(1.0, 3.0, 17) * np.sqrt(17 / 3), 17, 300), ("matern32", [0.8 * np.sqrt(17 / 3)], 17, 300)]


def gpc_reference(name, theta, X, y):
    """the numpy reference, with the two preconditions on it that make the comparison meaningful: it converged in < 50 steps and none
    of its objective decrements lies within a factor 1.2 of epsilon (the step at which the search stops cannot depend on rounding)"""
    want_logq, want, iters, decrements = M.logq_grad(name, theta, X, y, EPS)
    assert iters < 50
    assert not any(EPS / 1.2 <= dcr <= 1.2 * EPS for dcr in decrements), decrements
    return want_logq, want, iters


def raw_logq_grad(kid, theta, Xptr, d, n, yptr, ctx):
    _, pp, npar = nat.params_array(theta)
    g, lq, it = np.empty(npar), C.c_double(), C.c_int()
    nat.check(nat.lib().gprc_gpc_logq_grad(ctx.handle, kid, pp, npar, Xptr, d, n, yptr, EPS, 0, C.byref(lq),
                                           g.ctypes.data_as(C.POINTER(C.c_double)), C.byref(it)))
    return lq.value, g, it.value


@pytest.mark.parametrize("name,theta,d,n", [(name, GPC_THETA[name], 3, n) for n in (600, 1100) for name in M.NAMES] + GPC_WIDE)
def test_logq_grad_against_the_closed_form(name, theta, d, n):
    theta = np.asarray(theta, dtype=float)
    X, y = gpc_problem(n, d)
    want_logq, want, want_iters = gpc_reference(name, theta, X, y)
    Xf = np.asfortranarray(X)
    logq, grad, iters = raw_logq_grad(M.KERNEL_ID[name], theta, Xf.ctypes.data, d, n, y.ctypes.data, nat.default_context())
    assert grad.shape == (theta.size,)
    e = nerr(grad, want)
    print(f"logq_grad {name} n={n} d={d}: nerr(grad)={e:.3e} rel(logq)={abs(logq - want_logq) / abs(want_logq):.3e} iters={iters} ref={want_iters} "
          f"max|d/dtheta|={np.abs(want).max():.3g} min|d/dtheta|={np.abs(want).min():.3g} (gate 1e-10)")
    assert e <= TOL
    assert abs(logq - want_logq) <= TOL * abs(want_logq)
    assert iters == want_iters
    lq2, g2 = logq_grad(X, y, name, theta)                           # the host mirror is the same call
    assert lq2 == logq and np.array_equal(g2, grad)


@pytest.mark.parametrize("name", M.NAMES)
def test_logq_value_is_tied_to_the_fitted_classifier(name):
    """logq = GPC$logq + sum(diag(L)) - sum(log(diag(L))): the same mode search through the shared fills"""
    n, d = 600, 3
    theta = np.asarray(GPC_THETA[name], dtype=float)
    X, y = gpc_problem(n, d)
    func = grad_dict[name]
    k = CovFunc(func, {"l": theta} if M.is_ard(name) else func.bind(tuple(theta), {}))
    Xf = np.asfortranarray(X)                                        # kept alive: the call borrows its memory
    logq, _, iters = raw_logq_grad(func.kernel_id, theta, Xf.ctypes.data, d, n, y.ctypes.data, nat.default_context())
    gc = GPC(X, y, k, EPS, reference_stop=False)
    dl = np.diag(gc.L)
    want = gc.logq + dl.sum() - np.log(dl).sum()
    print(f"logq_grad {name} n={n}: logq={logq!r} from the classifier {want!r} iterations {gc.iterations} / {iters}")
    assert gc.iterations == iters
    assert abs(logq - want) <= TOL * abs(want)
    gc.close()


# ---- 5. predict_grad --------------------------------------------------------------------------------------------------------
# d = 17: three coordinate groups (blockIdx.z), the last of one coordinate, with ARD scaling
PRED_CASES = [(case, size) for case in M.CASES for size in M.SIZES] + [(("matern52_ard", list(np.linspace(1.0, 3.0, 17) * np.sqrt(17 / 3)), 17), (300, 0.1))]


def pred_case_id(cs):
    case, (n, noise) = cs
    return "%s-d%d-n%d-noise%g" % (case[0], case[2], n, noise)


def call_predict_grad(g, Xs, mean=True, var=True, dmean=True, dvar=True):
    """gprc_gpr_predict_grad with host pointers; an output not asked for is passed as NULL and returned as None"""
    d, ns = Xs.shape
    Xs = np.asfortranarray(Xs)
    out = [np.full(ns, np.nan) if mean else None, np.full(ns, np.nan) if var else None,
           np.full((d, ns), np.nan, order="F") if dmean else None, np.full((d, ns), np.nan, order="F") if dvar else None]
    nat.check(nat.lib().gprc_gpr_predict_grad(g._model, Xs.ctypes.data, ns, *[o.ctypes.data if o is not None else None for o in out]))
    return out


@pytest.mark.parametrize("cs", PRED_CASES, ids=pred_case_id)
def test_predict_grad_against_the_longdouble_reference(cs):
    case, (n, noise) = cs
    name, par, d = case
    X, y, Xs = G.make_case(case, n, m=40)                            # test point 0 IS training point 5
    assert np.array_equal(Xs[:, 0], X[:, 5])
    ref = M.predict_grad(name, par, X, y, noise, Xs, LD)             # pred_grad_ref.chol asserts every pivot > 0
    g = GPR(X, y, noise, kfun(name, par))
    assert g.noise == noise
    got = call_predict_grad(g, Xs)
    for what, a, b in zip(("mean", "var", "dmean", "dvar"), got, ref):
        e = G.nerr(np.asarray(a, dtype=LD), b)
        print("predict_grad %s n %d %s %.2e (gate 1e-10)" % (M.case_id(case) if d < 17 else name + "-d17", n, what, e))
        assert np.isfinite(a).all() and e <= 1e-10, (what, e)
    pred = g.predict(Xs)
    assert np.array_equal(got[0], pred[:, 0]) and np.array_equal(got[1], pred[:, 1])    # the bits of gprc_gpr_predict(pointwise = 1)
    only_dmean = call_predict_grad(g, Xs, mean=False, var=False, dvar=False)             # the mean's gradient alone: one pass, no solve
    assert only_dmean[0] is None and only_dmean[3] is None and np.array_equal(only_dmean[2], got[2])
    pa, dm, dv = g.predict_grad(Xs)                                  # the public method is the same call
    assert np.array_equal(pa, pred) and np.array_equal(dm, got[2]) and np.array_equal(dv, got[3])
    g.close()


# ---- 6. plumbing ------------------------------------------------------------------------------------------------------------
def raw_logp_grad(kid, theta, Xptr, d, n, yptr, noise, ctx):
    _, pp, npar = nat.params_array(theta)
    g, lp = np.empty(npar + 1), C.c_double()
    nat.check(nat.lib().gprc_gpr_logp_grad(ctx.handle, kid, pp, npar, Xptr, d, n, yptr, noise, C.byref(lp), g.ctypes.data_as(C.POINTER(C.c_double))))
    return lp.value, g


def test_pointer_kinds_repeat_calls_and_trim_give_the_same_bits():
    torch = pytest.importorskip("torch")
    theta, X, y = grad_case("matern52_ard", 1100, 3)
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
    assert nerr(two.alpha, M.gpr_fit("matern32_ard", ell, X, y, 0.1)["alpha"]) <= TOL
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
    for name in M.NAMES:
        kid = M.KERNEL_ID[name]
        for bad in (bad_ard if M.is_ard(name) else bad_iso):
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
