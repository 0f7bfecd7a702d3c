"""Gradients of the posterior sample paths on the MI355X and the Thompson-sampling maximiser over them: gprc_gpr_paths_eval_grad
(SamplePaths.paths_grad), the two gradient products alone (gprc_dev_feature_gemm_grad, gprc_dev_kernel_gemm_grad), SamplePaths.maximize
and GPR.thompson_batch, against the float64 formulas of tests/paths_grad_ref.py (which tests/test_paths_grad_cpu.py ties to their
longdouble twin and to central differences on these very inputs).

Gates: the project's TOL = 1e-10, normwise (conftest.nerr), on the gradients of all eight cases and on the entry at a training point
alone; bitwise equality of the values with gprc_gpr_paths_eval's, and of the gradients under every chunking, for single points, for
host and device pointers and over the model's lifetime; the two products componentwise inside the bounds derived here, against the
longdouble twin; the four conditions of the maximiser against the grid evaluated on the device.

The bound of a gradient product dout_isc = f_c sum_j w_ij e_cij B_js computed in float64 (u = 2^-53, gamma_k = k u / (1 - k u)):
  * as for the value products (tests/test_gpu_paths.py), a sum of `cols` products in any order, fused or not, of the operands formed,
    costs gamma_cols (|G^_c| |B|)_is.  An operand is now a product: the weight w as a correctly formed value (1 rounding), the
    difference a_ic - b_jc of two staged coordinates (1; for ARD both are scaled first, a relative change of the difference's terms
    that the factor t_c of the bound's |G_c| carries), their product (1), and the pair-independent factor applied once by the tail (1):
    gamma_{cols+4}.  The weight also carries the rounding of its squared distance, a sum of d terms, (d + 2) u s |dh/ds| with
    s |dh/ds| <= h for these kernels at these parameters up to a small constant: d more roundings relative to |h|.  Together
    gamma_{cols+d+4} (|G_c| |B|)_is with G_c[i, j] = t_c h_ij (a_ic - b_jc): the kernel product's bound.
  * features: the operand is sin(2 pi t) nu_cj (the sine's rounding and the product's), the tail's factor 2 pi scale one more:
    gamma_{cols+3} 2 pi (|nu_c o sin| |B|)_is.  The phase t = sum_c nu_cj a_ic + u_j is d fused multiply-adds and one addition,
    |t^ - t| <= gamma_{d+1} (sum_c' |nu_c'j a_ic'| + |u_j|); sinpi reduces its argument exactly and |d sin 2 pi t / dt| <= 2 pi, and
    the error is then multiplied by 2 pi |nu_cj|: gamma_{d+1} 4 pi^2 sum_j (sum_c' |nu_c'j a_ic'| + |u_j|) |nu_cj| |B_js|.
tests/test_paths_grad_cpu.py checks that numpy's own float64 products lie inside both against the twin (worst ratio 0.019).

Shapes: paths_ref.CASES with the last test point a training point (n_pad 512 and 1024; n* 1, 130, 300; S 1, 5, 70, 130: under one
16-column MFMA block, under and over the 32-column sample block; d 1, 3, 20: under one coordinate group of four, five groups, and two
staging passes before the weight is known); paths_ref.PRODUCTS (rows 129 .. 257, cols 67 .. 2117 ragged, d 1 / 2 / 3 / 20, S 1 .. 70).

Measured on an MI355X (every test prints its figures), 25 passed in 14 s.  Gradients against the float64 reference per case | at the
training point alone: 5.2e-15 | 6.7e-15, 1.5e-15 | 1.5e-15, 3.2e-14 | 4.3e-14, 5.0e-14 | 2.7e-14, 7.5e-15 | 7.5e-15, 9.1e-15 | 7.3e-15,
4.1e-15 | 4.1e-15, 2.7e-14 | 2.0e-14.  The products, worst |got - longdouble| / bound: features 0.0004 and 0.0173; kernel 0.0006
(matern52_ard), 0.0339 (sqrexp, d = 20), 0.0046 (gammaexp), 0.0062 (rationalquadratic, S = 1).  Bits: the values those of
gprc_gpr_paths_eval with and without `out`; gradients equal for repeat, halves, 130 single points, device pointers with ld = n* + 5 and
n* + 3, after add_data, after close and under a 2 MiB chunk budget.  Maximiser: 10-11 evaluations at d = 1, 51-84 at d = 2, every
candidate converged to 1e-8, worst (grid max - best) / max|F| 0.0 (at or above the grid), worst projected gradient of a best point 9.8e-9.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import paths_grad_ref as G
import paths_ref as R
from conftest import TOL, nerr
from gprc_amd import GPR, cov_func, polynomial
from gprc_amd import _native as nat
from gpu_calls import kfun, step_time_limit  # noqa: F401  (the autouse fixture)
from kernel_ref import KERNEL_ID

pytestmark = pytest.mark.gpu

LD = np.longdouble
CASE_IDS = [R.case_id(i) for i in range(len(R.CASES))]


@functools.lru_cache(maxsize=None)
def reference(index):
    """the problem and the float64 reference of case `index`, computed once and shared; the arrays are never written to"""
    name, par, *_ = R.CASES[index]
    X, y, Xs, nu, phase, W, E = G.problem(index)
    F, dF, U = G.paths_grad(name, par, X, y, R.NOISE, nu, phase, W, E, Xs)
    out = dict(name=name, par=par, X=X, y=y, Xs=Xs, nu=nu, phase=phase, W=W, E=E, F=F, dF=dF, U=U)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def model_of(ref, **kw):
    g = GPR(ref["X"], ref["y"], R.NOISE, kfun(ref["name"], ref["par"]), **kw)
    assert g.noise == R.NOISE                                       # no jitter was added: the reference's K_y is the model's
    return g


def paths_of(g, ref, **over):
    a = dict(nu=ref["nu"], phase=ref["phase"], w=ref["W"], e=ref["E"])
    a.update(over)
    return g.sample_paths(ref["W"].shape[1], ref["W"].shape[0], **a)


def raw_eval_grad(h, Xs, S, want_out=True, xptr=None, optr=None, dptr=None, ld=None, ldd=None, ns=None):
    """gprc_gpr_paths_eval_grad -> (rc, out or None, dout); xptr / optr / dptr: device addresses in place of the host arrays"""
    d = Xs.shape[0]
    ns = Xs.shape[1] if ns is None else ns
    out = np.full((max(ns, 1), S), np.nan, order="F")
    dout = np.full((max(ns, 1), S, d), np.nan, order="F")
    rc = nat.lib().gprc_gpr_paths_eval_grad(h, xptr or Xs.ctypes.data, ns, (optr or out.ctypes.data) if want_out else None, ld or ns,
                                            dptr or dout.ctypes.data, ldd or ns)
    return rc, (out if want_out else None), dout


# ---- 1. gradients ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(R.CASES)), ids=CASE_IDS)
def test_gradients_against_the_float64_reference(index):
    ref = reference(index)
    g = model_of(ref)
    with paths_of(g, ref) as sp:
        F, dF = sp.paths_grad(ref["Xs"])
    g.close()
    name, par, d, n, ns, D, S = R.CASES[index]
    assert F.shape == (ns, S) and dF.shape == (ns, S, d) and F.flags.f_contiguous and dF.flags.f_contiguous
    ef, eg = nerr(F, ref["F"]), nerr(dF, ref["dF"])
    et = nerr(dF[-1], ref["dF"][-1])                                # the training point on its own
    print("paths_grad %s: values %.2e gradients %.2e, at the training point %.2e" % (CASE_IDS[index], ef, eg, et))
    assert max(ef, eg, et) <= TOL


# ---- 2. the values' bits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [3, 5], ids=[CASE_IDS[i] for i in (3, 5)])
def test_values_have_the_bits_of_paths_eval_and_may_be_left_out(index):
    ref = reference(index)
    S = ref["W"].shape[1]
    g = model_of(ref)
    with paths_of(g, ref) as sp:
        values = sp.paths(ref["Xs"])
        rc, out, dout = raw_eval_grad(sp._h, ref["Xs"], S)
        assert rc == 0
        rc, none, dalone = raw_eval_grad(sp._h, ref["Xs"], S, want_out=False)
        assert rc == 0 and none is None
    g.close()
    assert np.array_equal(out, values)
    assert np.isfinite(dout).all() and np.array_equal(dalone, dout)
    print("value bits %s: out == gprc_gpr_paths_eval's; out = NULL leaves dout's bits" % CASE_IDS[index])


# ---- 3. the two products alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(R.PRODUCTS)), ids=["%d-%s" % (i, p[1] or p[0]) for i, p in enumerate(R.PRODUCTS)])
def test_gradient_products_inside_their_componentwise_bounds(index):
    torch = pytest.importorskip("torch")
    what, name, par, rows, cols, d, S = R.PRODUCTS[index]
    A, P, phase, B = R.product_problem(index)
    want, bound = G.product_grad_reference(index, LD)
    ctx = nat.Context(0, torch.cuda.current_stream().cuda_stream)
    ldb, ld = cols + 3, rows + 1
    Bd = np.full((S, ldb), np.nan)                                  # column s of B = row s of the C-ordered host image; NaN in the pitch's padding
    Bd[:, :cols] = B.T
    adev, pdev, phdev, bdev = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (A.T, P.T, phase, Bd))

    def run():
        out = torch.full((d, S, ld), float("nan"), dtype=torch.float64, device="cuda")    # dout[i + ld (s + S c)]
        torch.cuda.synchronize()
        if what == "features":
            nat.check(nat.lib().gprc_dev_feature_gemm_grad(ctx.handle, pdev.data_ptr(), phdev.data_ptr(), cols, adev.data_ptr(), rows, d, bdev.data_ptr(),
                                                           ldb, S, 1.0, out.data_ptr(), ld))
        else:
            _, pp, npar = nat.params_array(np.asarray(par, dtype=float))
            nat.check(nat.lib().gprc_dev_kernel_gemm_grad(ctx.handle, KERNEL_ID[name], pp, npar, adev.data_ptr(), rows, pdev.data_ptr(), cols, d,
                                                          bdev.data_ptr(), ldb, S, out.data_ptr(), ld))
        torch.cuda.synchronize()
        return out.cpu().numpy()

    got, again = run(), run()
    ctx.close()
    assert np.array_equal(got[:, :, :rows], again[:, :, :rows])
    assert np.isnan(got[:, :, rows:]).all()                         # nothing is written past `rows`
    got = got[:, :, :rows].transpose(2, 1, 0)
    assert np.isfinite(got).all()
    ratio = float((np.abs(got.astype(LD) - want) / bound).max())
    print("gradient product %d %s %s %d x %d, d = %d, S = %d: worst |got - longdouble| / bound %.4f" % (index, what, name, rows, cols, d, S, ratio))
    assert ratio <= 1.0


# ---- 4. bits ------------------------------------------------------------------------------------------------------------------------------
def test_same_bits_for_every_split_chunking_and_pointer_kind(monkeypatch):
    torch = pytest.importorskip("torch")
    ref = reference(7)                                              # n = 700, n* = 300, D = 260, S = 70, d = 3
    Xs, S = ref["Xs"], ref["W"].shape[1]
    d, ns = Xs.shape
    g = model_of(ref)
    sp = paths_of(g, ref)
    F, dF = sp.paths_grad(Xs)
    again = sp.paths_grad(Xs)
    assert np.array_equal(again[0], F) and np.array_equal(again[1], dF)
    half = ns // 2
    lo, hi = sp.paths_grad(Xs[:, :half]), sp.paths_grad(Xs[:, half:])
    assert np.array_equal(np.concatenate([lo[1], hi[1]], axis=0), dF) and np.array_equal(np.vstack([lo[0], hi[0]]), F)
    ref1 = reference(0)                                             # n* = 130 single points
    g1 = model_of(ref1)
    with paths_of(g1, ref1) as sp1:
        batch = sp1.paths_grad(ref1["Xs"])[1]
        singles = np.concatenate([sp1.paths_grad(ref1["Xs"][:, i:i + 1])[1] for i in range(ref1["Xs"].shape[1])], axis=0)
    g1.close()
    assert np.array_equal(singles, batch)
    # device pointers, and leading dimensions of the caller's
    xdev = torch.from_numpy(np.array(Xs.T, order="C")).cuda()
    odev = torch.full((S, ns + 5), float("nan"), dtype=torch.float64, device="cuda")
    ddev = torch.full((d, S, ns + 3), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rc, _, _ = raw_eval_grad(sp._h, Xs, S, xptr=xdev.data_ptr(), optr=odev.data_ptr(), dptr=ddev.data_ptr(), ld=ns + 5, ldd=ns + 3)
    assert rc == 0
    torch.cuda.synchronize()
    ohost, dhost = odev.cpu().numpy(), ddev.cpu().numpy()
    assert np.array_equal(ohost[:, :ns].T, F) and np.isnan(ohost[:, ns:]).all()
    assert np.array_equal(dhost[:, :, :ns].transpose(2, 1, 0), dF) and np.isnan(dhost[:, :, ns:]).all()
    # the model's lifetime: the bits of before after add_data and after the model is closed
    rng = np.random.default_rng(3)
    Xn = rng.uniform(-2, 2, (d, 30))
    g.add_data(Xn, np.sin(Xn.sum(0)))
    assert np.array_equal(sp.paths_grad(Xs)[1], dF)
    g.close()
    assert np.array_equal(sp.paths_grad(Xs)[1], dF)
    sp.close()
    # a small chunk budget in a second context: three chunks of 128 test points in both gradient products
    monkeypatch.setenv("GPRC_CHUNK_BYTES", str(256 * 1024 * 8))
    ctx2 = nat.Context(0)
    g2 = model_of(ref, ctx=ctx2)
    with paths_of(g2, ref) as sp2:
        F2, dF2 = sp2.paths_grad(Xs)
    g2.close()
    ctx2.close()
    assert np.array_equal(F2, F) and np.array_equal(dF2, dF)
    print("gradient bits: repeat, halves, %d single points, device pointers with ld = n* + 5 and n* + 3, after add_data, after close, "
          "GPRC_CHUNK_BYTES = 2 MiB: equal" % batch.shape[0])


# ---- 5. errors --------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    ref = reference(4)                                              # matern32, n = 300, n* = 130, S = 5
    Xs, S = ref["Xs"], ref["W"].shape[1]
    ns = Xs.shape[1]
    lib = nat.lib()
    g = model_of(ref)
    sp = paths_of(g, ref)

    def refused(rc):
        return rc == nat.ERR_ARG and nat.last_error().startswith("paths_eval_grad:")

    out, dout = np.empty((ns, S), order="F"), np.empty((ns, S, 3), order="F")
    assert refused(lib.gprc_gpr_paths_eval_grad(None, Xs.ctypes.data, ns, out.ctypes.data, ns, dout.ctypes.data, ns))
    assert refused(lib.gprc_gpr_paths_eval_grad(sp._h, Xs.ctypes.data, ns, out.ctypes.data, ns, None, ns)) and "dout" in nat.last_error()
    assert refused(lib.gprc_gpr_paths_eval_grad(sp._h, Xs.ctypes.data, ns, out.ctypes.data, ns, dout.ctypes.data, ns - 1)) and "ld_dout" in nat.last_error()
    assert refused(lib.gprc_gpr_paths_eval_grad(sp._h, Xs.ctypes.data, ns, out.ctypes.data, ns - 1, dout.ctypes.data, ns)) and "ld_out" in nat.last_error()
    assert refused(lib.gprc_gpr_paths_eval_grad(sp._h, Xs.ctypes.data, 0, out.ctypes.data, ns, dout.ctypes.data, ns))
    assert refused(lib.gprc_gpr_paths_eval_grad(sp._h, None, ns, out.ctypes.data, ns, dout.ctypes.data, ns))
    F, dF = sp.paths_grad(Xs)                                       # the paths are as usable as before
    assert nerr(dF, ref["dF"]) <= TOL and nerr(F, ref["F"]) <= TOL
    with pytest.raises(ValueError):
        sp.paths_grad(np.zeros((2, 4)))                             # d = 3
    sp.close()
    with pytest.raises(nat.GprcError):
        sp.paths_grad(Xs)
    # after its context is destroyed a paths object refuses, as for eval
    ctx2 = nat.Context(0)
    g2 = model_of(ref, ctx=ctx2)
    sp2 = paths_of(g2, ref)
    g2.close()
    ctx2.close()
    assert refused(raw_eval_grad(sp2._h, Xs, S)[0])
    sp2.close()
    g.close()


# ---- 6. the maximiser on the device ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", G.MAXIMA_SEEDS)
@pytest.mark.parametrize("which", range(len(G.MAXIMA)), ids=["d1-sqrexp", "d2-matern52_ard"])
def test_maximize_reaches_the_grid_maximum_of_every_path(which, seed):
    m = G.MAXIMA[which]
    X, y, nu, phase, W, E = G.maxima_problem(which, seed)
    lower, upper = np.full(m["d"], m["box"][0]), np.full(m["d"], m["box"][1])
    g = GPR(X, y, m["noise"], kfun(m["name"], m["par"]))
    assert g.noise == m["noise"]
    with g.sample_paths(m["S"], m["D"], nu=nu, phase=phase, w=W, e=E) as sp:
        Fg = sp.paths(G.maxima_grid(which))
        res = sp.maximize(lower, upper, n_starts=m["starts"], rng=np.random.default_rng(seed))
        again = sp.maximize(lower, upper, n_starts=m["starts"], rng=np.random.default_rng(seed))
        at_best = sp.paths(res.x_best)
    g.close()
    short, pg, inside = G.check_maxima(res, Fg.max(axis=0), float(np.abs(Fg).max()), lower, upper)
    print("maximize %s seed %d: %d evaluations; worst (grid max - best) / max|F| %.2e; worst projected gradient of a best point %.2e; "
          "candidates converged %d of %d" % (m["name"], seed, res.n_evals, short, pg, int((res.pg <= 1e-8).sum()), res.pg.size))
    assert res.x_best.shape == (m["d"], m["S"]) and res.f_best.shape == (m["S"],)
    assert short <= 1e-10
    assert pg <= 1e-6
    assert inside
    assert all(np.array_equal(a, b) for a, b in zip(res, again))
    assert np.array_equal(res.f_best, at_best[np.arange(m["S"]), np.arange(m["S"])])   # the bits of sp.paths at each best point alone or in a batch


# ---- 7. a Thompson batch ------------------------------------------------------------------------------------------------------------------
def test_thompson_batch():
    m = G.MAXIMA[1]
    X, y, *_ = G.maxima_problem(1, 0)
    lower, upper = np.full(2, m["box"][0]), np.full(2, m["box"][1])
    q, D, starts = 4, 256, 8
    g = GPR(X, y, m["noise"], kfun(m["name"], m["par"]))
    batch = g.thompson_batch(q, lower, upper, n_features=D, n_starts=starts, rng=np.random.default_rng(5))
    assert batch.shape == (2, q) and ((batch >= lower[:, None]) & (batch <= upper[:, None])).all()
    assert np.array_equal(g.thompson_batch(q, lower, upper, n_features=D, n_starts=starts, rng=np.random.default_rng(5)), batch)
    rng = np.random.default_rng(5)
    with g.sample_paths(q, D, rng=rng) as sp:                       # the same draws by hand
        res = sp.maximize(lower, upper, n_starts=starts, rng=rng)
    assert np.array_equal(res.x_best, batch)
    g.add_data(batch, np.sin(3.0 * batch[0]) * np.cos(batch[1]))
    second = g.thompson_batch(q, lower, upper, n_features=D, n_starts=starts, rng=np.random.default_rng(6))
    assert second.shape == (2, q) and ((second >= lower[:, None]) & (second <= upper[:, None])).all()
    g.close()
    gm = GPR(X, y, m["noise"], kfun(m["name"], m["par"]), devices=[0, 0])
    with pytest.raises(ValueError, match="refit"):
        gm.thompson_batch(q, lower, upper)
    gm.close()
    gp = GPR(X, y, m["noise"], cov_func(polynomial, sigma=0.5, p=2.0))
    with pytest.raises(ValueError):
        gp.thompson_batch(q, lower, upper)
    gp.close()
    print("thompson_batch: %d x %d inside the box, the same for a seed, the points of sample_paths + maximize; a second batch after add_data" % batch.shape)
