"""Sparse GPR with inducing points on the MI355X: gprc_sgpr_fit / _elbo / _predict / _get_elbo (SparseGPR, fit.elbo) and the two
building blocks gprc_dev_gram_rows and gprc_dev_col_reduce, against the float64 formulas of tests/sgpr_ref.py (which
tests/test_sgpr_cpu.py ties to their longdouble twin) and against the library's own exact GPR.

Gates: the project's TOL = 1e-10, relative on elbo and t, normwise (conftest.nerr) on mean and var; bitwise equality under every
chunking; elbo <= gprc_gpr_log_marginal; the Gram block and the column reduction componentwise inside the standard dot-product bound
gamma_769 (|C0| + |V|^T |V|), gamma_k = k u / (1 - k u), u = 2^-53, valid for any summation order and for fused multiply-adds (768 products
and the addition to the stored value).

Shapes (sgpr_ref.CASES): n and m off every tile size; m_pad = 512 (one panel) and 1024 (two panels: cross-panel Gram tiles and a
two-panel factor of B); m = 130, barely over one 128-block; a rank-deficient K_uu (linear; its trace term cancels to about 0 and is not
compared); Z = X with jitter 0, where the bound is tight.

Measured on an MI355X (every test prints its figures), 15 passed: against the float64 reference elbo <= 1.6e-13, t <= 1.1e-12,
mean <= 3.4e-13, var <= 1.7e-11 (case 3, linear, taken when the reference still summed its variance plainly and itself stood 1.3e-11
from longdouble there; it now sums exactly, 6.3e-12, and the test passes as before; next 6.0e-12, case 4);
Z = X against the library's exact GPR: elbo 5.2e-14, mean 1.3e-11, var 9.5e-13, |t| <= 7.1e-15 (sqrexp); gaps of the bound 532, 808, 37.9,
1.5e-4 (4.2e-8 relative, case 3), 37.7; the Gram block at 0.035 of its bound, the column reduction below 0.001 of its.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import packed_ref as P
import sgpr_ref as R
from conftest import TOL, nerr
from gprc_amd import GPC, GPR, GprcError, NotPositiveDefinite, SparseGPR, cov_func, linear, select_inducing, sqrexp
from gprc_amd import _native as nat
from gprc_amd.fit import dens, elbo
from gprc_amd.sparse import elbo as elbo_and_trace
from gpu_calls import kfun, same_bits, step_time_limit  # noqa: F401  (the autouse fixture)

pytestmark = pytest.mark.gpu

CASE_IDS = ["%d-%s" % (i, c[0]) for i, c in enumerate(R.CASES)]
LD = np.longdouble


def kernel_of(name, theta):
    return cov_func(linear, sigma=theta[0]) if name == "linear" else kfun(name, theta)


@functools.lru_cache(maxsize=None)
def reference(index):
    """the problem and the float64 reference of case `index`, computed once and shared; the arrays are never written to"""
    name, theta, n, m, d = R.CASES[index]
    X, y, Z, Xs = R.problem(index, n, m, d)
    r = R.sgpr(name, theta, X, y, R.NOISE, Z, R.JITTER, Xs)
    out = dict(X=X, y=y, Z=Z, Xs=Xs, k=kernel_of(name, theta), name=name, theta=theta, elbo=float(r["elbo"]), t=float(r["t"]),
               mean=r["mean"], var=r["var"], c=r["c"])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def raw_fit(ctx, k, X, y, noise, Z, jitter, Xptr=None, yptr=None):
    """gprc_sgpr_fit -> (rc, model handle); Xptr / yptr: device addresses in place of the host arrays"""
    d, n = X.shape
    _, pp, npar = nat.params_array(k.native_params(d))
    h = C.c_void_p()
    rc = nat.lib().gprc_sgpr_fit(ctx.handle, k.gprc_kernel[0], pp, npar, Xptr or X.ctypes.data, d, n, yptr or y.ctypes.data, noise,
                                 Z.ctypes.data if Z is not None else None, Z.shape[1] if Z is not None else 0, jitter, C.byref(h))
    return rc, h


def model_outputs(h, Xs, m):
    """[elbo, t, mean, var, c] of a sparse model"""
    ns = Xs.shape[1]
    e, t = C.c_double(), C.c_double()
    mean, var, c = np.full(ns, np.nan), np.full(ns, np.nan), np.full(m, np.nan)
    nat.check(nat.lib().gprc_sgpr_get_elbo(h, C.byref(e), C.byref(t)))
    nat.check(nat.lib().gprc_sgpr_predict(h, Xs.ctypes.data, ns, mean.ctypes.data, var.ctypes.data))
    nat.check(nat.lib().gprc_sgpr_get_c(h, c.ctypes.data))
    return [e.value, t.value, mean, var, c]


# ---- 1. values ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(R.CASES)), ids=CASE_IDS)
def test_values_against_the_float64_reference(index):
    ref = reference(index)
    s = SparseGPR(ref["X"], ref["y"], R.NOISE, ref["k"], ref["Z"], R.JITTER)
    mean, var = s.predict(ref["Xs"])
    got_elbo, got_t = s.elbo, s.trace
    s.close()
    errs = dict(elbo=abs(got_elbo - ref["elbo"]) / abs(ref["elbo"]), mean=nerr(mean, ref["mean"]), var=nerr(var, ref["var"]))
    if index != 3:
        errs["t"] = abs(got_t - ref["t"]) / abs(ref["t"])
    print("sgpr case %d (%s): %s; elbo %.6f t %.6g" % (index, ref["name"], {k: "%.2e" % v for k, v in errs.items()}, got_elbo, got_t))
    assert max(errs.values()) <= TOL, errs
    assert elbo(ref["X"], ref["y"], R.NOISE, ref["k"], ref["Z"], R.JITTER) == got_elbo     # gprc_sgpr_elbo: the bits of fit + get_elbo
    assert elbo_and_trace(ref["X"], ref["y"], R.NOISE, ref["k"], ref["Z"], R.JITTER, with_trace=True) == (got_elbo, got_t)


# ---- 2. chunk invariance, bitwise -------------------------------------------------------------------------------------------------------
def test_fit_and_predict_are_bitwise_chunk_invariant(monkeypatch):
    ref = reference(2)                                              # n = 2000, m = 600: m_pad = 1024
    m = ref["Z"].shape[1]
    ctx = nat.default_context()
    rc, h = raw_fit(ctx, ref["k"], ref["X"], ref["y"], R.NOISE, ref["Z"], R.JITTER)
    assert rc == 0
    whole = model_outputs(h, ref["Xs"], m)                          # the default budget: one chunk of 2048 rows, one of 384 test rows
    assert same_bits(model_outputs(h, ref["Xs"], m), whole)
    monkeypatch.setenv("GPRC_CHUNK_BYTES", str(256 * 1024 * 8))     # 256 rows per chunk at m_pad = 1024: eight fit chunks, two predict chunks
    ctx2 = nat.Context(0)
    rc, h2 = raw_fit(ctx2, ref["k"], ref["X"], ref["y"], R.NOISE, ref["Z"], R.JITTER)
    assert rc == 0
    parts = model_outputs(h2, ref["Xs"], m)
    assert same_bits(parts, whole)
    assert same_bits(model_outputs(h, ref["Xs"], m)[2:4], model_outputs(h2, ref["Xs"], m)[2:4])
    assert nerr(parts[4], ref["c"]) <= 1e-8                         # c itself is what the formulas say (cond(B) enters: a sanity gate only)
    nat.lib().gprc_model_free(h2)
    ctx2.close()
    nat.lib().gprc_model_free(h)


# ---- 3. tight at Z = X ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index,case", list(enumerate(R.TIGHT_CASES)), ids=[c[0] for c in R.TIGHT_CASES])
def test_inducing_points_equal_to_the_data_give_the_exact_model(index, case):
    name, theta = case
    X, y, _, Xs = R.problem(len(R.CASES) + index, R.TIGHT_N, 1, R.TIGHT_D)
    k = kernel_of(name, theta)
    g = GPR(X, y, R.NOISE, k)
    assert g.noise == R.NOISE
    pred = g.predict(Xs)
    lp = C.c_double()
    nat.check(nat.lib().gprc_gpr_get_logp(g._model, C.byref(lp)))
    g.close()
    s = SparseGPR(X, y, R.NOISE, k, X, 0.0)
    mean, var = s.predict(Xs)
    errs = (abs(s.elbo - lp.value) / abs(lp.value), nerr(mean, pred[:, 0]), nerr(var, pred[:, 1]))
    t = s.trace
    s.close()
    print("Z = X %s: elbo vs logp %.2e mean %.2e var %.2e, t %.2e" % (name, *errs, t))
    assert max(errs) <= TOL, errs
    assert abs(t) <= 1e-9


# ---- 4. the bound -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(R.CASES)), ids=CASE_IDS)
def test_the_bound_is_below_the_log_marginal_likelihood(index):
    ref = reference(index)
    lower = elbo(ref["X"], ref["y"], R.NOISE, ref["k"], ref["Z"], R.JITTER)
    logp = dens(ref["X"], ref["y"], R.NOISE, ref["name"], ref["theta"])
    print("case %d: elbo %.9f logp %.9f gap %.3g (relative %.2e)" % (index, lower, logp, logp - lower, (logp - lower) / abs(logp)))
    assert lower <= logp


# ---- 5. the Gram block and the column reduction on an arbitrary matrix ------------------------------------------------------------------
def test_gram_rows_and_col_reduce_on_an_arbitrary_matrix():
    torch = pytest.importorskip("torch")
    rows, n_pad, ld = 768, 1024, 768 + 128
    g = P.geometry(n_pad)
    assert g.n_pad == n_pad and g.P == 2
    rng = np.random.default_rng(5)
    V = rng.standard_normal((rows, n_pad))
    C0 = rng.standard_normal(g.packed_size)
    w = rng.standard_normal(rows)
    o0 = rng.standard_normal(n_pad)
    Vd = np.zeros((n_pad, ld))                                      # column j of V = row j of the C-ordered host image
    Vd[:, :rows] = V.T
    ctx = nat.Context(0, torch.cuda.current_stream().cuda_stream)
    vt = torch.from_numpy(Vd).cuda()
    wd = torch.from_numpy(w).cuda()

    def run(splits):
        """the packed buffer and the reduced vector after the calls over the row ranges `splits`"""
        pk, out = torch.from_numpy(C0.copy()).cuda(), torch.from_numpy(o0.copy()).cuda()
        torch.cuda.synchronize()
        for r0, r1 in splits:
            nat.check(nat.lib().gprc_dev_gram_rows(ctx.handle, vt.data_ptr() + 8 * r0, ld, r1 - r0, n_pad, pk.data_ptr()))
            nat.check(nat.lib().gprc_dev_col_reduce(ctx.handle, vt.data_ptr() + 8 * r0, ld, r1 - r0, n_pad, wd.data_ptr() + 8 * r0, out.data_ptr()))
        torch.cuda.synchronize()
        return pk.cpu().numpy(), out.cpu().numpy()

    got, red = run([(0, rows)])
    got3, red3 = run([(0, 256), (256, 512), (512, 768)])
    torch.cuda.synchronize()
    ctx.close()
    gam = LD(P.gamma(rows + 1))
    Vl = np.ascontiguousarray(V.T.astype(LD))                       # n_pad x rows, contiguous along the summed index
    worst = 0.0
    for q in range(g.P):
        cols = slice(q * g.NB, (q + 1) * g.NB)
        prod = np.einsum("ik,jk->ij", Vl[q * g.NB:], Vl[cols])      # (V^T V)[q NB:, cols] in longdouble
        mag = np.einsum("ik,jk->ij", np.abs(Vl[q * g.NB:]), np.abs(Vl[cols]))
        c0 = P.panel_view(C0, g, q).astype(LD)
        mask = P.lower_mask(g, q)                                   # the part of the diagonal block above the diagonal is not compared
        err = np.abs(P.panel_view(got, g, q).astype(LD) - (c0 + prod))
        bound = gam * (np.abs(c0) + mag)
        worst = max(worst, float((err[mask] / bound[mask]).max()))
        assert np.all(err[mask] <= bound[mask]), (q, worst)
        upper = ~(np.arange(g.n_pad - q * g.NB)[:, None] // 128 >= np.arange(g.NB)[None, :] // 128)
        assert np.array_equal(P.panel_view(got, g, q)[upper], P.panel_view(C0, g, q)[upper])   # tiles above the block diagonal: untouched
    rerr = np.abs(red.astype(LD) - (o0.astype(LD) + Vl @ w.astype(LD)))
    rbound = gam * (np.abs(o0).astype(LD) + np.abs(Vl) @ np.abs(w).astype(LD))
    print("gram_rows: worst error / bound %.3f; col_reduce: %.3f" % (worst, float((rerr / rbound).max())))
    assert np.all(rerr <= rbound)
    assert np.array_equal(got3, got) and np.array_equal(red3, red)  # three calls of 256 rows: the very bits of one call of 768


# ---- 6. arguments -------------------------------------------------------------------------------------------------------------------------
def test_arguments_model_types_and_pointer_kinds():
    torch = pytest.importorskip("torch")
    ref = reference(4)
    X, y, Z, Xs, k = ref["X"], ref["y"], ref["Z"], ref["Xs"], ref["k"]
    d, n = X.shape
    m, ns = Z.shape[1], Xs.shape[1]
    ctx = nat.default_context()
    L = nat.lib()
    rc, h = raw_fit(ctx, k, X, y, R.NOISE, Z, R.JITTER)
    assert rc == 0
    host = model_outputs(h, Xs, m)
    nn, dd = C.c_int64(), C.c_int64()
    nat.check(L.gprc_model_dims(h, C.byref(nn), C.byref(dd)))
    assert (nn.value, dd.value) == (m, d)
    # a device-pointer X (and y) gives the bits of the host-pointer call
    Xd = torch.from_numpy(np.array(X.T, order="C", copy=True)).cuda()   # d x n column-major = n x d row-major
    yd = torch.from_numpy(y.copy()).cuda()
    torch.cuda.synchronize()
    rc, hd = raw_fit(ctx, k, X, y, R.NOISE, Z, R.JITTER, Xptr=Xd.data_ptr(), yptr=yd.data_ptr())
    assert rc == 0
    assert same_bits(model_outputs(hd, Xs, m), host)
    L.gprc_model_free(hd)
    # one output may be NULL, not both
    mean = np.full(ns, np.nan)
    nat.check(L.gprc_sgpr_predict(h, Xs.ctypes.data, ns, mean.ctypes.data, None))
    var = np.full(ns, np.nan)
    nat.check(L.gprc_sgpr_predict(h, Xs.ctypes.data, ns, None, var.ctypes.data))
    assert np.array_equal(mean, host[2]) and np.array_equal(var, host[3])
    assert L.gprc_sgpr_predict(h, Xs.ctypes.data, ns, None, None) == nat.ERR_ARG
    # the exact-GPR and GPC calls refuse a sparse model
    buf = np.empty(max(n, ns, m * m))
    sc = C.c_double()
    for rc in (L.gprc_gpr_predict(h, Xs.ctypes.data, ns, 1, buf.ctypes.data, buf.ctypes.data),
               L.gprc_gpr_predict_grad(h, Xs.ctypes.data, ns, buf.ctypes.data, None, None, None),
               L.gprc_gpr_loo(h, buf.ctypes.data, None, None, None),
               L.gprc_gpr_extend(h, Xs.ctypes.data, ns, buf.ctypes.data),
               L.gprc_model_get_L(h, buf.ctypes.data, m),
               L.gprc_gpr_get_alpha(h, buf.ctypes.data), L.gprc_gpr_get_logp(h, C.byref(sc)), L.gprc_gpr_get_noise(h, C.byref(sc)),
               L.gprc_gpc_predict_latent(h, Xs.ctypes.data, ns, buf.ctypes.data, buf.ctypes.data),
               L.gprc_gpc_predict_class(h, Xs.ctypes.data, ns, buf.ctypes.data),
               L.gprc_gpc_get_f_hat(h, buf.ctypes.data), L.gprc_gpc_get_logq(h, C.byref(sc))):
        assert rc == nat.ERR_ARG and nat.last_error()
    assert same_bits(model_outputs(h, Xs, m), host)                  # and leave it as it was
    L.gprc_model_free(h)
    # ... and the sparse calls refuse a GPR and a GPC model
    g = GPR(X[:, :200], y[:200], R.NOISE, k)
    rng = np.random.default_rng(3)
    Xc = rng.uniform(-1, 1, (2, 60))
    yc = np.sign(Xc[0] + 0.1 * rng.standard_normal(60))
    yc[yc == 0] = 1.0
    c = GPC(Xc, yc, cov_func(sqrexp, l=0.8))
    for model in (g._model, c._model):
        assert L.gprc_sgpr_predict(model, Xs.ctypes.data, ns, buf.ctypes.data, buf.ctypes.data) == nat.ERR_ARG
        assert "not a sparse GPR model" in nat.last_error()
        assert L.gprc_sgpr_get_elbo(model, C.byref(sc), None) == nat.ERR_ARG
        assert L.gprc_sgpr_get_c(model, buf.ctypes.data) == nat.ERR_ARG
    g.close()
    # refused values
    for noise, jitter, Zbad in ((R.NOISE, -1e-6, Z), (R.NOISE, float("nan"), Z), (0.0, R.JITTER, Z), (-0.05, R.JITTER, Z), (float("inf"), R.JITTER, Z),
                                (R.NOISE, R.JITTER, Z[:, :0]), (R.NOISE, R.JITTER, None)):
        rc, hb = raw_fit(ctx, k, X, y, noise, Zbad, jitter)
        assert rc == nat.ERR_ARG and not hb.value, (noise, jitter)
    with pytest.raises(GprcError):
        SparseGPR(X, y, 0.0, k, Z)
    # duplicated inducing points without jitter: K_uu is singular at the second pivot (k(z,z) = 1 = l_10^2 exactly)
    ks = cov_func(sqrexp, l=0.6)
    Zdup = np.asfortranarray(np.hstack([Z[:, :1], Z[:, :1], Z[:, 1:]]))
    rc, hb = raw_fit(ctx, ks, X, y, R.NOISE, Zdup, 0.0)
    assert rc == 2 and "K_uu" in nat.last_error() and not hb.value
    with pytest.raises(NotPositiveDefinite) as ei:
        SparseGPR(X, y, R.NOISE, ks, Zdup, 0.0)
    assert ei.value.info == 2
    assert np.isfinite(elbo(X, y, R.NOISE, ks, Zdup, R.JITTER))      # with the default jitter the same Z fits (the value is not judged here)
    # m > n is allowed; select_inducing picks distinct columns
    Zsel = select_inducing(X, 64, rng=7)
    assert Zsel.shape == (d, 64) and len({tuple(col) for col in Zsel.T}) == 64 and all(tuple(col) in {tuple(c2) for c2 in X.T} for col in Zsel.T)
    few = SparseGPR(X[:, :50], y[:50], R.NOISE, k, Zsel)
    assert np.isfinite(few.elbo) and few.Z.shape == (d, 64) and few.noise == R.NOISE
    few.close()
