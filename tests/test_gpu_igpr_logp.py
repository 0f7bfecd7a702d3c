"""The iterative GPR's stochastic log evidence and gradient on the MI355X through the C ABI: gprc_dev_lowrank_grad (the low-rank-weighted
contraction on the f64 MFMA), gprc_igpr_probes, gprc_igpr_logp_grad, and IterativeGPR.logp_grad / fit.optimize_iterative on top of them.

Every bound is derived in tests/igpr_logp_ref.py (its docstring has the table and the reasoning), whose checks run here on the device's
output and in tests/test_igpr_logp_cpu.py on a numpy model of the same algorithm: the eight paths_ref.CASES at noise 0.1, tolerance 1e-10,
ranks 0 and 32, 63 probes from default_rng(DRAW_SEED).  The contraction alone: n = 1 (exactly 0), 15, 16, 17, 129, 130, 300 and 2117 (34
row tiles = 17 stripes of two, the last ragged; 34 column tiles), R = 1, 3, 4, 5, 64 and 65 (two blocks), d = 1, 3, 17 and 20 (two staging
passes), ARD at d = 17 and 20, all eight kernels, and an input with two identical points off the diagonal.  Every test prints its figures.

Measured on an MI355X, 61 passed in 27 s.  Contraction <= 0.006 of its bound on all thirteen shapes, repeats equal bit for bit; probes <=
0.30 of their bound; q_s <= 2.4e-14 in the bound's units (bound 1e-11, the numpy model 4.1e-14); gradient far inside its bound (the
solve's tolerance term dominates it); |logp - formula| <= 1.0e-13; against gprc_gpr_logp_grad the value within 2.26 and every gradient
entry within 2.61 standard errors (the numpy model's figures to the printed digits); every bitwise comparison equal.  Optimiser on case 7
from -107.0, exact optimum 420.40: rank 0 ends 0.05 nats below it after 58 evaluations, rank 32 0.08 below after 321 (5 - 6 s each).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import igpr_logp_ref as G
import igpr_ref as I
import paths_ref as R
from gprc_amd import GPR, IterativeGPR
from gprc_amd import _native as nat
from gprc_amd.fit import logp_grad, optimize, optimize_iterative
from gpu_calls import kfun, step_time_limit  # noqa: F401  (the autouse fixture)
from kernel_ref import KERNEL_ID

pytestmark = pytest.mark.gpu

CASE_IDS = [R.case_id(i) for i in range(len(R.CASES))]
ALL = range(len(R.CASES))
T = G.T_PROBES


def ctx():
    return nat.default_context().handle


def raw_fit(ref, rank, tol=I.CG_TOL, max_iter=0, y=None):
    _, pp, npar = nat.params_array(ref["par"])
    h = C.c_void_p()
    y = ref["y"] if y is None else y
    rc = nat.lib().gprc_igpr_fit(ctx(), KERNEL_ID[ref["name"]], pp, npar, ref["X"].ctypes.data, ref["d"], ref["n"], y.ctypes.data, I.NOISE, tol,
                                 max_iter, rank, C.byref(h))
    return rc, h


@functools.lru_cache(maxsize=None)
def model(index, rank):
    """the fitted model of (case, rank), shared by the tests and never freed before the process ends"""
    rc, h = raw_fit(I.reference(index), rank)
    nat.check(rc)
    return h


def raw_logp_grad(h, G1, G2, n_par, n, want_se=True, want_terms=True, g1ptr=None, ldg1=None, g2ptr=None, ldg2=None, count=None):
    """gprc_igpr_logp_grad -> (rc, logp, se, grad, terms)"""
    Tn = G2.shape[1] if count is None else count
    lp, se = C.c_double(np.nan), C.c_double(np.nan)
    grad, terms = np.full(n_par + 1, np.nan), np.full(max(Tn, 1), np.nan)
    rc = nat.lib().gprc_igpr_logp_grad(h, g1ptr or (G1.ctypes.data if G1 is not None else None), ldg1 or (G1.shape[0] if G1 is not None else 1),
                                       g2ptr or G2.ctypes.data, ldg2 or n, Tn, C.byref(lp), C.byref(se) if want_se else None, grad.ctypes.data,
                                       terms.ctypes.data if want_terms else None)
    return rc, lp.value, se.value, grad, terms


def raw_alpha(h, n):
    a = np.full(n, np.nan)
    nat.check(nat.lib().gprc_igpr_get_alpha(h, a.ctypes.data))
    return a


@functools.lru_cache(maxsize=None)
def device_L(index, rank):
    """the device's own preconditioner factor (None at rank 0), registered for igpr_logp_ref.dense"""
    if rank == 0:
        return None
    ref = I.reference(index)
    n = ref["n"]
    _, pp, npar = nat.params_array(ref["par"])
    L, piv, reached = np.full((n, rank), np.nan, order="F"), np.full(rank, -7, dtype=np.int64), C.c_int64(-1)
    nat.check(nat.lib().gprc_dev_pivoted_cholesky(ctx(), KERNEL_ID[ref["name"]], pp, npar, ref["X"].ctypes.data, ref["d"], n, rank, L.ctypes.data, n,
                                                  piv.ctypes.data, C.byref(reached)))
    L = L[:, :reached.value]
    L.setflags(write=False)
    G.DEVICE_L[(index, rank)] = L
    return L


def dense(index, rank):
    device_L(index, rank)
    return G.dense(index, rank, None if rank == 0 else (index, rank))


def raw_probes(h, G1, G2, n):
    Z = np.full((n, G2.shape[1]), np.nan, order="F")
    nat.check(nat.lib().gprc_igpr_probes(h, G1.ctypes.data if G1 is not None else None, G1.shape[0] if G1 is not None else 1, G2.ctypes.data, n,
                                         G2.shape[1], Z.ctypes.data, n))
    return Z


@functools.lru_cache(maxsize=None)
def evidence(index, rank):
    """one T = 63 call per (case, rank), shared: (logp, se, grad, terms, Z)"""
    ref = I.reference(index)
    G1, G2 = G.draws(index)
    h = model(index, rank)
    rc, lp, se, grad, terms = raw_logp_grad(h, G1, G2, len(ref["par"]), ref["n"])
    assert rc == 0
    return lp, se, grad, terms, raw_probes(h, G1, G2, ref["n"])


# ---- 1. the contraction alone ---------------------------------------------------------------------------------------------------------------
# (kernel, parameters, d, n, R, two identical points)
CONTRACTIONS = [
    ("sqrexp", [0.7], 3, 1, 1, False),
    ("gammaexp", [1.2, 1.5], 3, 15, 3, False),
    ("rationalquadratic", [0.9, 1.7], 1, 16, 4, False),
    ("sqrexp_ard", [0.5, 1.5, 3.0], 3, 17, 5, False),
    ("matern32", [0.9], 3, 129, 64, False),
    ("matern52", [6.0], 20, 130, 65, False),
    ("matern32_ard", list(np.linspace(3.0, 9.0, 20)), 20, 300, 5, False),
    ("matern52_ard", [0.6, 1.4, 2.5], 3, 2117, 5, False),
    ("sqrexp", [5.0], 17, 300, 64, False),
    ("sqrexp_ard", list(np.linspace(2.0, 6.0, 17)), 17, 129, 1, False),
    ("gammaexp", [1.2, 0.8], 3, 130, 4, True),
    ("rationalquadratic", [0.9, 1.7], 3, 300, 65, True),
    ("matern32_ard", [0.8, 1.1, 2.0], 3, 130, 3, True),
]


def contraction_problem(i):
    name, par, d, n, Rk, twin = CONTRACTIONS[i]
    rng = np.random.default_rng(5300 + i)
    X = rng.uniform(-2, 2, (d, n))
    if twin:
        X[:, n - 3] = X[:, 4]                                         # an s = 0 pair off the diagonal, in different tiles for n > 64
    return np.asfortranarray(X), np.asfortranarray(rng.standard_normal((n, Rk))), np.asfortranarray(rng.standard_normal((n, Rk)))


def raw_lowrank(name, par, X, A, B, lda=None, ldb=None, kid=None):
    d, n = X.shape
    _, pp, npar = nat.params_array(np.asarray(par, dtype=float))
    g = np.full(npar, np.nan)
    rc = nat.lib().gprc_dev_lowrank_grad(ctx(), KERNEL_ID[name] if kid is None else kid, pp, npar, X.ctypes.data, d, n, A.ctypes.data, lda or n, B.ctypes.data, ldb or n,
                                         A.shape[1], g.ctypes.data)
    return rc, g


@pytest.mark.parametrize("i", range(len(CONTRACTIONS)), ids=["%s-d%d-n%d-R%d%s" % (c[0], c[2], c[3], c[4], "-twin" if c[5] else "") for c in CONTRACTIONS])
def test_contraction_against_a_longdouble_sum(i):
    name, par, d, n, Rk, _ = CONTRACTIONS[i]
    X, A, B = contraction_problem(i)
    rc, g = raw_lowrank(name, par, X, A, B)
    assert rc == 0, nat.last_error()
    rc, g2 = raw_lowrank(name, par, X, A, B)
    assert rc == 0 and np.array_equal(g, g2)                          # a repeat: the same bits
    if n == 1:
        assert not g.any()                                            # one point: dk(x, x) / dtheta = 0 exactly
    worst = G.check_contraction(name, par, X, A, B, g)
    print("lowrank_grad %s d = %d, n = %d, R = %d: worst |got - ref| / bound %.2e" % (name, d, n, Rk, worst))


def test_contraction_rejects_bad_arguments():
    X, A, B = contraction_problem(1)
    assert raw_lowrank("gammaexp", [1.2, 1.5], X, A, B, lda=14)[0] == nat.ERR_ARG
    assert raw_lowrank("linear", [1.0], X, A, B, kid=1)[0] == nat.ERR_ARG                 # GPRC_LINEAR: no k(x, x) = 1, no exact gradient


# ---- 2. probes --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", ALL, ids=CASE_IDS)
def test_probes(index):
    ref = I.reference(index)
    G1, G2 = G.draws(index)
    for rank in G.RANKS:
        Z = raw_probes(model(index, rank), G1 if rank else None, G2, ref["n"])
        ratio = G.check_probes(device_L(index, rank), I.NOISE, G1, G2, Z)
        assert np.array_equal(Z, evidence(index, rank)[4])
        print("probes %s rank %d: %.3f of their bound" % (CASE_IDS[index], rank, ratio))


# ---- 3. - 5., 7.: the terms, the gradient, the value, the statistics -----------------------------------------------------------------------
@pytest.mark.parametrize("index", ALL, ids=CASE_IDS)
def test_terms_against_the_dense_value(index):
    for rank in G.RANKS:
        lp, se, grad, terms, Z = evidence(index, rank)
        fig = G.check_terms(dense(index, rank), Z, terms)
        print("q_s %s rank %d: worst %.2e in the bound's units (bound %.0e; the numpy model %.1e)" % (CASE_IDS[index], rank, fig, G.Q_BOUND,
                                                                                                      G.Q_MODEL_WORST))


@pytest.mark.parametrize("index", ALL, ids=CASE_IDS)
def test_gradient_against_longdouble_solves(index):
    ref = I.reference(index)
    for rank in G.RANKS:
        lp, se, grad, terms, Z = evidence(index, rank)
        worst = G.check_gradient(ref, dense(index, rank), Z, grad, I.CG_TOL)
        print("gradient %s rank %d: worst error %.2e of its bound" % (CASE_IDS[index], rank, worst))


@pytest.mark.parametrize("index", ALL, ids=CASE_IDS)
def test_value_and_standard_error_are_the_stated_formulas(index):
    ref = I.reference(index)
    for rank in G.RANKS:
        lp, se, grad, terms, Z = evidence(index, rank)
        dn = dense(index, rank)
        alpha = raw_alpha(model(index, rank), ref["n"])
        # log det P is the device's: from its own L it is within the r x r factor's rounding of numpy's
        err = G.check_value(ref["y"], alpha, dn["logdet_p"], terms, lp, se)
        print("value %s rank %d: logp %.6f, se %.4f, |logp - formula| %.2e" % (CASE_IDS[index], rank, lp, se, err))


@pytest.mark.parametrize("index", ALL, ids=CASE_IDS)
def test_statistics_against_the_exact_evidence(index):
    ref = I.reference(index)
    exact = logp_grad(ref["X"], ref["y"], I.NOISE, ref["name"], ref["par"])
    for rank in G.RANKS:
        lp, se, grad, terms, Z = evidence(index, rank)
        dn = dense(index, rank)
        U = np.asarray(I.solve_ld(ref, Z), dtype=float)
        W = np.linalg.solve(dn["Lp"].T, np.linalg.solve(dn["Lp"], Z))
        zv, zg = G.statistics(ref, dn, lp, se, grad, U, W, exact)
        print("statistics %s rank %d: logp %.3f +- %.3f (exact %.3f, %.2f se), worst gradient entry %.2f se" % (CASE_IDS[index], rank, lp, se, exact[0],
                                                                                                               zv, zg))
        assert zv <= 4.0 and zg <= 4.0


# ---- 6. bitwise ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [0, 3, 6], ids=[CASE_IDS[i] for i in (0, 3, 6)])
def test_bitwise(index):
    torch = pytest.importorskip("torch")
    ref = I.reference(index)
    n, npar = ref["n"], len(ref["par"])
    G1, G2 = G.draws(index)
    B = I.solve_rhs(ref)
    for rank in G.RANKS:
        h = model(index, rank)
        lp, se, grad, terms, Z = evidence(index, rank)
        alpha0 = raw_alpha(h, n)
        X0 = np.full(B.shape, np.nan, order="F")
        nat.check(nat.lib().gprc_igpr_solve(h, B.ctypes.data, n, B.shape[1], X0.ctypes.data, n, None, None))
        # a repeat
        rc, lp2, se2, grad2, terms2 = raw_logp_grad(h, G1, G2, npar, n)
        assert rc == 0 and lp2 == lp and se2 == se and np.array_equal(grad2, grad) and np.array_equal(terms2, terms)
        # without the optional outputs
        rc, lp3, _, grad3, _ = raw_logp_grad(h, G1, G2, npar, n, want_se=False, want_terms=False)
        assert rc == 0 and lp3 == lp and np.array_equal(grad3, grad)
        # device pointers, pitches larger than the extents
        g2d = np.full((T, n + 5), np.nan)
        g2d[:, :n] = G2.T
        g1d = np.full((T, 32 + 3), np.nan)
        g1d[:, :32] = G1.T
        g2dev, g1dev = torch.from_numpy(g2d).cuda(), torch.from_numpy(g1d).cuda()
        torch.cuda.synchronize()
        rc, lp4, se4, grad4, terms4 = raw_logp_grad(h, G1, G2, npar, n, g1ptr=g1dev.data_ptr(), ldg1=35, g2ptr=g2dev.data_ptr(), ldg2=n + 5)
        assert rc == 0 and lp4 == lp and se4 == se and np.array_equal(grad4, grad) and np.array_equal(terms4, terms)
        zdev = torch.full((T, n + 2), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        nat.check(nat.lib().gprc_igpr_probes(h, g1dev.data_ptr(), 35, g2dev.data_ptr(), n + 5, T, zdev.data_ptr(), n + 2))
        torch.cuda.synchronize()
        zgot = zdev.cpu().numpy()
        assert np.array_equal(zgot[:, :n].T, Z) and np.isnan(zgot[:, n:]).all()
        # a probe's term does not depend on the other probes of the call
        rc, _, _, _, terms5 = raw_logp_grad(h, np.asfortranarray(G1[:, :5]), np.asfortranarray(G2[:, :5]), npar, n)
        assert rc == 0 and np.array_equal(terms5, terms[:5])
        # the model is unchanged
        assert np.array_equal(raw_alpha(h, n), alpha0)
        X1 = np.full(B.shape, np.nan, order="F")
        nat.check(nat.lib().gprc_igpr_solve(h, B.ctypes.data, n, B.shape[1], X1.ctypes.data, n, None, None))
        assert np.array_equal(X1, X0)


def test_python_layer_returns_the_abi_bits():
    ref = I.reference(0)
    G1, G2 = G.draws(0)
    with IterativeGPR(ref["X"], ref["y"], I.NOISE, kfun(ref["name"], ref["par"]), tol=I.CG_TOL, precond_rank=32) as m:
        est = m.logp_grad(g1=G1, g2=G2)
        lp, se, grad, terms, Z = evidence(0, 32)
        assert est.value == lp and est.se == se and np.array_equal(est.grad, grad) and np.array_equal(est.terms, terms)
        assert np.array_equal(m.probes(G1, G2), Z)
        drawn = m.logp_grad(T, rng=np.random.default_rng(G.DRAW_SEED))            # g2 first, then g1: the same normals
        assert drawn.value == lp and np.array_equal(drawn.grad, grad)
        one = m.logp_grad(g1=G1[:, :1], g2=G2[:, :1])
        assert np.isnan(one.se) and one.terms[0] == terms[0]


# ---- 8. the optimiser -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_optimum():
    ref = I.reference(7)
    start = logp_grad(ref["X"], ref["y"], I.NOISE, ref["name"], ref["par"])[0]
    return start, optimize(ref["X"], ref["y"], I.NOISE, ref["name"], ref["par"])


@pytest.mark.parametrize("rank", G.RANKS)
def test_optimiser_recovers_the_exact_optimum(rank):
    ref = I.reference(7)                                               # matern52_ard, d = 3, n = 700
    start, best = exact_optimum()
    got = optimize_iterative(ref["X"], ref["y"], I.NOISE, ref["name"], ref["par"], n_probes=T, rng=np.random.default_rng(7), tol=1e-8, precond_rank=rank)
    at = logp_grad(ref["X"], ref["y"], got["noise"], ref["name"], got["par"])[0]
    print("optimiser rank %d: start %.1f, exact optimum %.2f, exact evidence at the stochastic optimum %.2f (%.2f below), estimate %.2f +- %.2f, "
          "%d evaluations, convergence %d" % (rank, start, best["value"], at, best["value"] - at, got["value"], got["se"], got["counts"][0],
                                              got["convergence"]))
    assert at - start >= 0.99 * (best["value"] - start)
    assert got["se"] > 0 and set(got) == set(best) | {"se"}


# ---- 9. errors ------------------------------------------------------------------------------------------------------------------------------------
def test_errors():
    ref = I.reference(0)
    n, npar = ref["n"], len(ref["par"])
    G1, G2 = G.draws(0)
    h = model(0, 32)
    assert raw_logp_grad(h, G1, G2, npar, n, count=0)[0] == nat.ERR_ARG                                   # T < 1
    assert raw_logp_grad(h, G1[:, :1], G2[:, :1], npar, n, want_se=True)[0] == nat.ERR_ARG                # se_out with T = 1
    assert raw_logp_grad(h, G1[:, :1], G2[:, :1], npar, n, want_se=False)[0] == 0
    assert raw_logp_grad(h, G1, G2, npar, n, ldg2=n - 1)[0] == nat.ERR_ARG
    assert raw_logp_grad(h, G1, G2, npar, n, ldg1=31)[0] == nat.ERR_ARG
    exact = GPR(ref["X"], ref["y"], I.NOISE, kfun(ref["name"], ref["par"]))                                # a non-iterative model
    assert raw_logp_grad(exact._model, G1, G2, npar, n)[0] == nat.ERR_ARG
    Z = np.empty((n, T), order="F")
    assert nat.lib().gprc_igpr_probes(exact._model, G1.ctypes.data, 32, G2.ctypes.data, n, T, Z.ctypes.data, n) == nat.ERR_ARG
    assert raw_logp_grad(None, G1, G2, npar, n)[0] == nat.ERR_ARG
    m = IterativeGPR(ref["X"], ref["y"], I.NOISE, kfun(ref["name"], ref["par"]), tol=I.CG_TOL, precond_rank=32)
    m.close()                                                                                             # a closed model
    with pytest.raises(nat.GprcError) as e:
        m.logp_grad(g1=G1, g2=G2)
    assert e.value.status == nat.ERR_ARG
    # the iteration cap: y = 0 is solved in 0 steps, so a model with max_iter = 2 exists; its probes then run into the cap, and every output is
    # written from the last iterates, as gprc_igpr_solve does
    rc, hz = raw_fit(ref, 0, max_iter=2, y=np.zeros(n))
    assert rc == 0
    rc, lp, se, grad, terms = raw_logp_grad(hz, None, G2, npar, n)
    assert rc == nat.ERR_MAXITER and "max_iter" in nat.last_error()
    assert np.isfinite(lp) and np.isfinite(se) and np.isfinite(grad).all() and np.isfinite(terms).all()
    nat.lib().gprc_model_free(hz)
