"""The iterative exact GPR on the MI355X through the C ABI: gprc_dev_pivoted_cholesky, gprc_igpr_fit / _solve / _predict / _get_alpha /
_stats, gprc_gpr_paths_create on an iterative model, and IterativeGPR.sample_paths / thompson_batch on top of them.

Every bound is derived in tests/igpr_ref.py (its docstring has the table and the reasoning), whose checks run here on the device's output
and in tests/test_igpr_cpu.py on a numpy model of the same algorithm: the eight paths_ref.CASES at noise 0.1 (n = 300 and 700, ragged
against the 128-row and 64-column tiles; d = 1, 3, 20; kappa(K_y) 202 .. 1570), conjugate-gradient tolerance 1e-10, ranks 0 and 32,
B = [y, E[:, :4]] for every case and E[:, :70] (over one block of 64 right-hand sides) for the four cases whose E has 70 columns.
Bitwise: a column alone or in a batch, a repeat of the call, device pointers with ldb = n + 5; alpha = solve(y); the mean with and
without the variance; paths_grad's values = paths'.

Measured on an MI355X (every test prints its figures), 40 passed in 16 s.  Pivoted Cholesky, r = 32: rank 32 in all eight cases,
interpolation <= 5.0e-16 (bound 3.8e-15), every pivot AT the replayed maximum (0 beside a slack of 6.0e-14); case 2 at r = 64: rank 33,
largest remaining diagonal 5.9e-14.  Solve of [y, E[:, :4]]: iterations 21 .. 154 at rank 0 and 1 .. 65 at rank 32 (per case e.g. 101 ..
107 against 61 .. 65, 148 .. 154 against 59 .. 61), true residual <= 9.9e-11, error <= 0.016 of its bound, the reported residual equal to
the test's own to three digits; the 70-column blocks: true residual <= 1.0e-10, error <= 0.0012 of its bound.  Predict: mean <= 0.0057
and variance <= 0.0013 of their bounds; against the library's exact GPR 1.0e-10 (mean) and 3.3e-11 (variance) normwise.  Paths: U
<= 2.0e-10 (bounds 4.0e-8 .. 3.1e-7), the values <= 6.1e-14 from prior + K* U_device.  Every bitwise comparison equal.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import igpr_ref as I
import paths_ref as R
from conftest import TOL, nerr
from gprc_amd import GPR, IterativeGPR, SparseGPR, cov_func, linear, polynomial, constant
from gprc_amd import _native as nat
from gpu_calls import kfun, step_time_limit  # noqa: F401  (the autouse fixture)
from kernel_ref import KERNEL_ID

pytestmark = pytest.mark.gpu

CASE_IDS = [R.case_id(i) for i in range(len(R.CASES))]
ALL = range(len(R.CASES))
DP = C.POINTER(C.c_double)


def ctx():
    return nat.default_context().handle


def raw_fit(ref, rank, tol=I.CG_TOL, max_iter=0, noise=I.NOISE, kid=None, par=None, X=None, y=None, out=True):
    """gprc_igpr_fit -> (rc, model handle)"""
    _, pp, npar = nat.params_array(ref["par"] if par is None else par)
    X = ref["X"] if X is None else X
    y = ref["y"] if y is None else y
    h = C.c_void_p()
    rc = nat.lib().gprc_igpr_fit(ctx(), KERNEL_ID[ref["name"]] if kid is None else kid, pp, npar, X.ctypes.data if X is not False else None, ref["d"],
                                 ref["n"], y.ctypes.data if y is not False else None, noise, tol, max_iter, rank, C.byref(h) if out else None)
    return rc, h


@functools.lru_cache(maxsize=None)
def model(index, rank):
    """the fitted model of (case, rank), shared by the tests and never freed before the process ends"""
    rc, h = raw_fit(I.reference(index), rank)
    nat.check(rc)
    return h


def raw_solve(h, B, n, ldb=None, ldx=None, bptr=None, xptr=None, stats=True):
    """gprc_igpr_solve -> (rc, X, iterations, reported true residual)"""
    S = B.shape[1]
    X = np.full((n, S), np.nan, order="F")
    iters, res = (C.c_int * S)(*([-1] * S)), np.full(S, np.nan)
    rc = nat.lib().gprc_igpr_solve(h, bptr or B.ctypes.data, ldb or n, S, xptr or X.ctypes.data, ldx or n, iters if stats else None,
                                   res.ctypes.data_as(DP) if stats else None)
    return rc, X, np.array(iters[:]), res


def raw_predict(h, Xs, variance=True):
    ns = Xs.shape[1]
    mean, var = np.full(ns, np.nan), np.full(ns, np.nan)
    nat.check(nat.lib().gprc_igpr_predict(h, Xs.ctypes.data, ns, mean.ctypes.data, var.ctypes.data if variance else None))
    return mean, var if variance else None


def raw_alpha(h, n):
    a = np.full(n, np.nan)
    nat.check(nat.lib().gprc_igpr_get_alpha(h, a.ctypes.data))
    return a


def raw_pchol(ref, r):
    n = ref["n"]
    _, pp, npar = nat.params_array(ref["par"])
    L, piv, rank = np.full((n, r), np.nan, order="F"), np.full(r, -7, dtype=np.int64), C.c_int64(-1)
    nat.check(nat.lib().gprc_dev_pivoted_cholesky(ctx(), KERNEL_ID[ref["name"]], pp, npar, ref["X"].ctypes.data, ref["d"], n, r, L.ctypes.data, n,
                                                  piv.ctypes.data, C.byref(rank)))
    return L, piv, rank.value


# ---- 1. pivoted Cholesky ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", ALL, ids=CASE_IDS)
def test_pivoted_cholesky(index):
    ref = I.reference(index)
    L, piv, rank = raw_pchol(ref, 32)
    fig = I.check_pivoted_cholesky(ref, 32, L, piv, rank)
    L2, piv2, rank2 = raw_pchol(ref, 32)
    assert rank2 == rank and np.array_equal(piv2, piv) and np.array_equal(L2, L)
    print("pivoted Cholesky %s: rank %d, interpolation %.2e (bound %.2e), greedy %.2e (slack %.2e)" % (CASE_IDS[index], rank, fig["interpolation"],
                                                                                                      fig["bound"], fig["greedy"], fig["slack"]))


def test_pivoted_cholesky_stops_early_on_a_one_dimensional_problem():
    ref = I.reference(2)                                            # rationalquadratic, d = 1
    L, piv, rank = raw_pchol(ref, 64)
    fig = I.check_pivoted_cholesky(ref, 64, L, piv, rank)           # zero columns and pivots -1 from the rank on; the remaining diagonal
    print("pivoted Cholesky case 2 at r = 64: rank %d, largest remaining diagonal %.2e" % (rank, fig["remaining"]))
    assert 1 <= rank < 64


# ---- 2. solve -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", ALL, ids=CASE_IDS)
def test_solve_inside_its_bounds_and_bitwise_invariant(index):
    torch = pytest.importorskip("torch")
    ref = I.reference(index)
    n, B = ref["n"], I.solve_rhs(ref)
    S = B.shape[1]
    iters = {}
    for rank in I.RANKS:
        h = model(index, rank)
        rc, X, it, res = raw_solve(h, B, n)
        assert rc == 0
        fig = I.check_solve(ref, B, X, res)
        iters[rank] = it
        print("solve %s rank %d: iterations %d .. %d, true residual %.2e, error %.2e (%.4f of its bound), report ratio %.3f" % (
            CASE_IDS[index], rank, it.min(), it.max(), fig["true"], fig["err"], fig["err_bound_ratio"], fig["report_ratio"]))
        # bits: y alone, a repeat, device pointers with ldb = n + 5 and ldx = n + 3
        _, X1, it1, _ = raw_solve(h, B[:, :1], n)
        assert np.array_equal(X1[:, 0], X[:, 0]) and it1[0] == it[0]
        _, Xr, itr, resr = raw_solve(h, B, n)
        assert np.array_equal(Xr, X) and np.array_equal(itr, it) and np.array_equal(resr, res)
        Bd = np.full((S, n + 5), np.nan)
        Bd[:, :n] = B.T
        bdev = torch.from_numpy(Bd).cuda()
        xdev = torch.full((S, n + 3), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rc, _, itd, _ = raw_solve(h, B, n, ldb=n + 5, ldx=n + 3, bptr=bdev.data_ptr(), xptr=xdev.data_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        got = xdev.cpu().numpy()
        assert np.array_equal(got[:, :n].T, X) and np.isnan(got[:, n:]).all() and np.array_equal(itd, it)
        # a zero column: zeros, 0 iterations, the other columns' bits unchanged
        Bz = B.copy(order="F")
        Bz[:, -1] = 0.0
        rc, Xz, itz, resz = raw_solve(h, Bz, n)
        assert rc == 0 and not Xz[:, -1].any() and itz[-1] == 0 and resz[-1] == 0.0 and np.array_equal(Xz[:, :-1], X[:, :-1])
    assert (iters[32] < iters[0]).all()                              # fewer iterations with the preconditioner, column by column


@pytest.mark.parametrize("index", [2, 3, 5, 7], ids=[CASE_IDS[i] for i in (2, 3, 5, 7)])
def test_solve_a_block_of_seventy_columns(index):
    ref = I.reference(index)
    n, B = ref["n"], np.asfortranarray(ref["E"][:, :70])
    for rank in I.RANKS:
        rc, X, it, res = raw_solve(model(index, rank), B, n)
        assert rc == 0
        fig = I.check_solve(ref, B, X, res)
        print("solve S = 70 %s rank %d: iterations %d .. %d, true residual %.2e, error %.4f of its bound" % (CASE_IDS[index], rank, it.min(), it.max(),
                                                                                                          fig["true"], fig["err_bound_ratio"]))
    _, X5, _, _ = raw_solve(model(index, 32), np.asfortranarray(B[:, 60:70]), n)   # columns of the second block alone: the same bits
    assert np.array_equal(X5, X[:, 60:70])


# ---- 3. fit and predict -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", ALL, ids=CASE_IDS)
def test_fit_and_predict(index):
    ref = I.reference(index)
    n, Xs = ref["n"], ref["Xs"]
    for rank in I.RANKS:
        h = model(index, rank)
        alpha = raw_alpha(h, n)
        _, X, it, res = raw_solve(h, np.asfortranarray(ref["y"][:, None]), n)
        assert np.array_equal(alpha, X[:, 0])
        its, rec, true, rk = C.c_int(), C.c_double(), C.c_double(), C.c_int64()
        nat.check(nat.lib().gprc_igpr_stats(h, C.byref(its), C.byref(rec), C.byref(true), C.byref(rk)))
        assert its.value == it[0] and true.value == res[0] and rec.value <= I.CG_TOL and rk.value == rank
        dims = C.c_int64(), C.c_int64()
        nat.check(nat.lib().gprc_model_dims(h, C.byref(dims[0]), C.byref(dims[1])))
        assert (dims[0].value, dims[1].value) == (n, ref["d"])
    h = model(index, 32)
    mean, var = raw_predict(h, Xs)
    fig = I.check_predict(ref, alpha, mean, var)
    mean_only, _ = raw_predict(h, Xs, variance=False)
    assert np.array_equal(mean_only, mean)
    print("predict %s (n* = %d): mean %.4f of its bound, variance %.4f of its bound" % (CASE_IDS[index], Xs.shape[1], fig["mean_ratio"], fig["var_ratio"]))


def test_predict_against_the_exact_model_of_the_library():
    ref = I.reference(4)                                            # matern32, n = 300, n* = 130
    g = GPR(ref["X"], ref["y"], I.NOISE, kfun(ref["name"], ref["par"]))
    assert g.noise == I.NOISE
    exact = g.predict(ref["Xs"])
    g.close()
    with IterativeGPR(ref["X"], ref["y"], I.NOISE, kfun(ref["name"], ref["par"]), tol=I.CG_TOL, precond_rank=32) as ig:
        fig = I.check_predict(ref, ig.alpha, exact[:, 0], exact[:, 1])   # the exact model inside the same bounds
        pred = ig.predict(ref["Xs"])
        assert ig.stats.rank == 32 and ig.stats.relres_recurrence <= I.CG_TOL
    print("against GPR: mean %.2e, variance %.2e (the exact model: %.4f and %.4f of the bounds)" % (nerr(pred[:, 0], exact[:, 0]), nerr(pred[:, 1], exact[:, 1]),
                                                                                                 fig["mean_ratio"], fig["var_ratio"]))
    I.check_predict(ref, ig.alpha, pred[:, 0], pred[:, 1])


# ---- 4. paths -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", ALL, ids=CASE_IDS)
def test_paths_of_an_iterative_model(index):
    ref = I.reference(index)
    Xs, W = ref["Xs"], ref["W"]
    ig = IterativeGPR(ref["X"], ref["y"], I.NOISE, kfun(ref["name"], ref["par"]), tol=I.CG_TOL, precond_rank=32)
    sp = ig.sample_paths(W.shape[1], W.shape[0], nu=ref["nu"], phase=ref["phase"], w=W, e=ref["E"])
    ig.close()                                                      # the paths survive the model
    U, F = sp.weights, sp.paths(Xs)
    Fg, dF = sp.paths_grad(Xs)
    sp.close()
    fig = I.check_weights(ref, U)
    prior = np.sqrt(2.0 / W.shape[0]) * (R.features(ref["nu"], ref["phase"], Xs) @ W)
    want = prior + I.pairwise(ref["name"], ref["par"], Xs, ref["X"], np.float64)[0] @ U
    err = nerr(F, want)
    print("paths %s: U %.2e (bound %.2e), values against prior + K* U_device %.2e" % (CASE_IDS[index], fig["err"], fig["bound"], err))
    assert err <= TOL and np.array_equal(Fg, F) and np.isfinite(dF).all()


def test_thompson_batch_of_an_iterative_model():
    ref = I.reference(0)                                            # sqrexp, d = 3, n = 300
    lower, upper = -2.0 * np.ones(3), 2.0 * np.ones(3)
    with IterativeGPR(ref["X"], ref["y"], I.NOISE, kfun(ref["name"], ref["par"]), tol=I.CG_TOL, precond_rank=32) as ig:
        xb = ig.thompson_batch(4, lower, upper, n_features=256, n_starts=4, rng=np.random.default_rng(5))
    assert xb.shape == (3, 4) and (xb >= lower[:, None]).all() and (xb <= upper[:, None]).all()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    lib = nat.lib()
    ref = I.reference(1)                                            # gammaexp, n = 300
    n, X, y, B = ref["n"], ref["X"], ref["y"], I.solve_rhs(ref)

    def refused(rc, status=nat.ERR_ARG):
        return rc == status and len(nat.last_error()) > 0

    # max_iter = 2: no model from fit; from solve the last iterate, its statistics and iterations = 2
    rc, h = raw_fit(ref, 0, max_iter=2)
    assert refused(rc, nat.ERR_MAXITER) and not h
    hz_rc, hz = raw_fit(ref, 0, max_iter=2, y=np.zeros(n))          # y = 0 is solved in 0 iterations: a model whose loops stop after two
    nat.check(hz_rc)
    rc, X2, it2, res2 = raw_solve(hz, B, n)
    assert refused(rc, nat.ERR_MAXITER) and (it2 == 2).all() and np.isfinite(X2).all() and (res2 > I.CG_TOL).all() and np.isfinite(res2).all()
    Xm = I.pcg(ref["K"], I.NOISE, B, I.CG_TOL, max_iter=2)[0]       # the model's iterate after two steps
    assert nerr(X2, Xm) <= TOL
    nat.check(lib.gprc_model_free(hz))
    hm = model(1, 0)
    # kernels outside the eight
    for kid, par in ((nat.CONSTANT, [1.0]), (nat.LINEAR, [1.3]), (nat.POLYNOMIAL, [0.5, 2.0])):
        rc, h = raw_fit(ref, 0, kid=kid, par=par)
        assert refused(rc) and not h
    # noise, rank, pointers
    for kw in (dict(noise=0.0), dict(noise=-0.1), dict(rank=-1), dict(rank=2000), dict(X=False), dict(y=False), dict(out=False)):
        rank = kw.pop("rank", 0)
        rc, h = raw_fit(ref, rank, **kw)
        assert refused(rc) and not h, kw
    assert refused(raw_solve(hm, B, n, ldx=n - 1)[0]) and refused(raw_solve(hm, B, n, ldb=n - 1)[0])
    assert refused(lib.gprc_igpr_solve(hm, None, n, 1, B.ctypes.data, n, None, None))
    assert refused(lib.gprc_igpr_solve(hm, B.ctypes.data, n, 1, None, n, None, None))
    assert refused(lib.gprc_igpr_solve(None, B.ctypes.data, n, 1, B.ctypes.data, n, None, None))
    # the other model calls refuse an iterative model, the iterative calls another model
    out = np.empty(n)
    assert refused(lib.gprc_gpr_predict(hm, ref["Xs"].ctypes.data, 1, 1, out.ctypes.data, out.ctypes.data))
    assert refused(lib.gprc_gpr_loo(hm, out.ctypes.data, None, None, None))
    assert refused(lib.gprc_sgpr_predict(hm, ref["Xs"].ctypes.data, 1, out.ctypes.data, out.ctypes.data))
    assert refused(lib.gprc_gpr_get_alpha(hm, out.ctypes.data)) and refused(lib.gprc_model_get_L(hm, out.ctypes.data, n))
    g = GPR(X, y, I.NOISE, kfun(ref["name"], ref["par"]))
    assert refused(lib.gprc_igpr_predict(g._model, ref["Xs"].ctypes.data, 1, out.ctypes.data, out.ctypes.data))
    assert refused(lib.gprc_igpr_solve(g._model, B.ctypes.data, n, 1, out.ctypes.data, n, None, None))
    assert refused(lib.gprc_igpr_get_alpha(g._model, out.ctypes.data)) and refused(lib.gprc_igpr_stats(g._model, None, None, None, None))
    g.close()
    sg = SparseGPR(X, y, I.NOISE, kfun(ref["name"], ref["par"]), X[:, :40])
    assert refused(lib.gprc_igpr_predict(sg._model, ref["Xs"].ctypes.data, 1, out.ctypes.data, out.ctypes.data))
    sg.close()
    for k in (cov_func(polynomial, sigma=0.5, p=2.0), cov_func(linear, sigma=1.3), cov_func(constant, c=1.0)):
        with pytest.raises(nat.GprcError):
            IterativeGPR(X, y, I.NOISE, k)
    rc, X3, _, _ = raw_solve(hm, B, n)                              # the shared model is as usable as before
    assert rc == 0 and np.isfinite(X3).all()
