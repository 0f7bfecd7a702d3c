"""Posterior sample paths on the MI355X: gprc_gpr_paths_create / _eval / _get_weights / _dims / _free (GPR.sample_paths) and the two
generated-operand products alone (gprc_dev_feature_gemm, gprc_dev_kernel_gemm), against the float64 formulas of tests/paths_ref.py
(which tests/test_paths_cpu.py ties to their longdouble twin on these very inputs) and against the library's own predict.

Gates: the project's TOL = 1e-10, normwise (conftest.nerr), on the paths, on U, on the training identity and on the mean identity;
bitwise equality under every chunking, for single points, for host and device pointers and over the model's lifetime; 5 standard errors
on the statistics.  The two products alone are held componentwise to the bounds derived here, against the longdouble twin.

The bound of a product out_is = sum_j g_ij B_js computed in float64 (u = 2^-53, gamma_k = k u / (1 - k u)):
  * a sum of `cols` products, in any order and with fused multiply-adds or not, of operands g^ and B: |fl(sum) - sum_j g^_ij B_js| <=
    gamma_cols (|G^| |B|)_is (Higham, Accuracy and Stability, section 3.1; the MFMA's groups of four, the stripes and their tail are one
    such order).  One more rounding, that of g^ itself as a correctly formed value, makes it gamma_{cols+1} (|G| |B|)_is: the kernel product's
    bound.  (A kernel value also carries the rounding of its squared distance s, about (d + 2) u s |dk/ds|; s |dk/ds| stays below 1
    for these kernels at these parameters and vanishes where k is near 1, so against (|G| |B|)_is of a row with 67 or more columns
    it stays a small part of gamma_{cols+1}: the bound is not widened for it, and the figures show the room.)
  * features: g = cos 2 pi t with t = sum_c nu_cj a_ic + u_j computed as d fused multiply-adds and one addition, |t^ - t| <=
    gamma_{d+1} (sum_c |nu_cj a_ic| + |u_j|); cospi reduces its argument exactly and |d cos 2 pi t / dt| <= 2 pi, so
    |g^ - g| <= 2 pi gamma_{d+1} (sum_c |nu_cj a_ic| + |u_j|) beside its own rounding, and the product's bound gains the phase term
    2 pi gamma_{d+1} sum_j (sum_c |nu_cj a_ic| + |u_j|) |B_js|.
tests/test_paths_cpu.py checks that numpy's own float64 product lies inside both against the twin.

Shapes (paths_ref.CASES, paths_ref.PRODUCTS): n = 300 and 700 (n_pad 512 and 1024: a two-panel forward and reversed solve); n* = 1, 130,
300; D = 1, 6, 260; S = 1, 5, 70, 130 (off 16, over one 64 block, over the 128-row solve block); d = 1, 3, 20 (two staging passes);
products with rows 129 .. 257 and cols 67 .. 2117 (17 stripes of two column tiles, the last tile ragged).

Measured on an MI355X (every test prints its figures), 23 passed in 14 s.  Against the float64 reference, paths | U per case:
5.7e-15 | 1.1e-14, 1.2e-15 | 1.2e-14, 7.8e-14 | 3.8e-14, 8.4e-14 | 6.1e-14, 6.2e-15 | 9.6e-15, 2.5e-14 | 1.8e-14, 7.5e-15 | 7.4e-15,
4.0e-14 | 4.3e-14.  The products, worst |got - longdouble| / bound: features 0.0003 (130 x 2117, d = 3, S = 70) and 0.0089 (129 x 67,
d = 20, S = 5); kernel 0.0003 (matern52_ard 130 x 2117), 0.0247 (sqrexp 129 x 67, d = 20), 0.0040 (gammaexp 131 x 301), 0.0047
(rationalquadratic 257 x 130, S = 1).  Training identity 1.4e-14, 1.5e-13 (n = 700, S = 130), 3.2e-14; mean identity 8.8e-15, 9.8e-15.
Bits: repeat, halves, 130 single points, device pointers with ld = n* + 5 and a 2 MiB chunk budget all equal; the bits of before after
add_data and after the model is freed.  Statistics through GPR.sample_paths: worst z of the mean 1.77, of the covariance 2.66 (the
reference's own figures for that seed), the paths 6.2e-15 from the float64 reference.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import paths_ref as R
from conftest import TOL, nerr
from gprc_amd import GPC, GPR, SparseGPR, cov_func, linear, polynomial, sqrexp
from gprc_amd import _native as nat
from gpu_calls import kfun, same_bits, step_time_limit  # noqa: F401  (the autouse fixture)
from kernel_ref import KERNEL_ID

pytestmark = pytest.mark.gpu

LD = np.longdouble
CASE_IDS = [R.case_id(i) for i in range(len(R.CASES))]


@functools.lru_cache(maxsize=None)
def reference(index, noise=R.NOISE):
    """the problem and the float64 reference of case `index`, computed once and shared; the arrays are never written to"""
    name, par, *_ = R.CASES[index]
    X, y, Xs, nu, phase, W, E = R.problem(index)
    F, U = R.paths(name, par, X, y, noise, nu, phase, W, E, Xs)
    out = dict(name=name, par=par, X=X, y=y, Xs=Xs, nu=nu, phase=phase, W=W, E=E, F=F, U=U)
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


def raw_eval(h, Xs, S, xptr=None, optr=None, ld=None):
    """gprc_gpr_paths_eval -> (rc, out); xptr / optr: device addresses in place of the host arrays"""
    ns = Xs.shape[1]
    out = np.full((ns, S), np.nan, order="F")
    rc = nat.lib().gprc_gpr_paths_eval(h, xptr or Xs.ctypes.data, ns, optr or out.ctypes.data, ld or ns)
    return rc, out


# ---- 1. values ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(R.CASES)), ids=CASE_IDS)
def test_values_against_the_float64_reference(index):
    ref = reference(index)
    g = model_of(ref)
    with paths_of(g, ref) as sp:
        F, U = sp.paths(ref["Xs"]), sp.weights
        dims = [C.c_int64() for _ in range(4)]
        nat.check(nat.lib().gprc_gpr_paths_dims(sp._h, *[C.byref(v) for v in dims]))
    g.close()
    name, par, d, n, ns, D, S = R.CASES[index]
    assert [v.value for v in dims] == [n, d, D, S] and F.shape == (ns, S) and U.shape == (n, S)
    ef, eu = nerr(F, ref["F"]), nerr(U, ref["U"])
    print("paths %s: paths %.2e U %.2e" % (CASE_IDS[index], ef, eu))
    assert max(ef, eu) <= TOL


# ---- 2. the two products alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(R.PRODUCTS)), ids=["%d-%s" % (i, p[1] or p[0]) for i, p in enumerate(R.PRODUCTS)])
def test_products_inside_their_componentwise_bounds(index):
    torch = pytest.importorskip("torch")
    what, name, par, rows, cols, d, S = R.PRODUCTS[index]
    A, P, phase, B = R.product_problem(index)
    want, bound = R.product_reference(index, LD)
    ctx = nat.Context(0, torch.cuda.current_stream().cuda_stream)
    ldb, ld = cols + 3, rows + 1
    Bd = np.full((S, ldb), np.nan)                                  # column s of B = row s of the C-ordered host image; NaN in the pitch's padding
    Bd[:, :cols] = B.T
    adev, pdev, phdev, bdev = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (A.T, P.T, phase, Bd))

    def run():
        out = torch.full((S, ld), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        if what == "features":
            nat.check(nat.lib().gprc_dev_feature_gemm(ctx.handle, pdev.data_ptr(), phdev.data_ptr(), cols, adev.data_ptr(), rows, d, bdev.data_ptr(), ldb, S,
                                                      1.0, out.data_ptr(), ld))
        else:
            _, pp, npar = nat.params_array(np.asarray(par, dtype=float))
            nat.check(nat.lib().gprc_dev_kernel_gemm(ctx.handle, KERNEL_ID[name], pp, npar, adev.data_ptr(), rows, pdev.data_ptr(), cols, d, bdev.data_ptr(),
                                                     ldb, S, out.data_ptr(), ld))
        torch.cuda.synchronize()
        return out.cpu().numpy()

    got, again = run(), run()
    ctx.close()
    assert np.array_equal(got[:, :rows], again[:, :rows])
    assert np.isnan(got[:, rows:]).all()                            # nothing is written past `rows`
    got = got[:, :rows].T
    assert np.isfinite(got).all()
    ratio = float((np.abs(got.astype(LD) - want) / bound).max())
    print("product %d %s %s %d x %d, d = %d, S = %d: worst |got - longdouble| / bound %.4f" % (index, what, name, rows, cols, d, S, ratio))
    assert ratio <= 1.0


# ---- 3. the training identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [0, 3, 5], ids=[CASE_IDS[i] for i in (0, 3, 5)])
def test_paths_at_the_training_points_close_the_linear_system(index):
    """eval(X) + sqrt(noise) E + noise U = y 1^T: (K + noise I) U = y - prior - sqrt(noise) E with the update kernel's K, no reference"""
    ref = reference(index)
    g = model_of(ref)
    with paths_of(g, ref) as sp:
        FX, U = sp.paths(ref["X"]), sp.weights
    g.close()
    S = U.shape[1]
    err = nerr(FX + np.sqrt(R.NOISE) * ref["E"] + R.NOISE * U, np.repeat(ref["y"][:, None], S, axis=1))
    print("training identity %s: %.2e" % (CASE_IDS[index], err))
    assert err <= TOL


# ---- 4. the mean identity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [2, 7], ids=[CASE_IDS[i] for i in (2, 7)])
def test_paths_without_randomness_are_the_posterior_mean(index):
    ref = reference(index)
    g = model_of(ref)
    mean = g.predict(ref["Xs"])[:, 0]
    with paths_of(g, ref, w=np.zeros_like(ref["W"]), e=np.zeros_like(ref["E"])) as sp:
        F = sp.paths(ref["Xs"])
    g.close()
    err = nerr(F, np.repeat(mean[:, None], F.shape[1], axis=1))
    print("mean identity %s: %.2e" % (CASE_IDS[index], err))
    assert err <= TOL


# ---- 5. bits ------------------------------------------------------------------------------------------------------------------------------
def test_same_bits_for_every_split_chunking_and_pointer_kind(monkeypatch):
    torch = pytest.importorskip("torch")
    ref = reference(7)                                              # n = 700, n* = 300, D = 260, S = 70
    Xs, S = ref["Xs"], ref["W"].shape[1]
    ns = Xs.shape[1]
    g = model_of(ref)
    sp = paths_of(g, ref)
    whole, U = sp.paths(Xs), sp.weights
    assert np.array_equal(sp.paths(Xs), whole)
    half = ns // 2
    assert np.array_equal(np.vstack([sp.paths(Xs[:, :half]), sp.paths(Xs[:, half:])]), whole)
    ref1 = reference(0)                                             # n* = 130 single points
    g1 = model_of(ref1)
    with paths_of(g1, ref1) as sp1:
        batch = sp1.paths(ref1["Xs"])
        singles = np.vstack([sp1.paths(ref1["Xs"][:, i:i + 1]) for i in range(ref1["Xs"].shape[1])])
    g1.close()
    assert np.array_equal(singles, batch)
    # device pointers, and a leading dimension of the caller's
    xdev = torch.from_numpy(np.array(Xs.T, order="C")).cuda()
    odev = torch.full((S, ns + 5), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rc, _ = raw_eval(sp._h, Xs, S, xptr=xdev.data_ptr(), optr=odev.data_ptr(), ld=ns + 5)
    assert rc == 0
    torch.cuda.synchronize()
    dev = odev.cpu().numpy()
    assert np.array_equal(dev[:, :ns].T, whole) and np.isnan(dev[:, ns:]).all()
    sp.close()
    g.close()
    # a small chunk budget in a second context: two chunks of test points, two of training points in create
    monkeypatch.setenv("GPRC_CHUNK_BYTES", str(256 * 1024 * 8))
    ctx2 = nat.Context(0)
    g2 = model_of(ref, ctx=ctx2)
    with paths_of(g2, ref) as sp2:
        assert np.array_equal(sp2.weights, U)
        assert np.array_equal(sp2.paths(Xs), whole)
    g2.close()
    ctx2.close()
    print("bits: repeat, halves, %d single points, device pointers with ld = n* + 5, GPRC_CHUNK_BYTES = 2 MiB: equal" % batch.shape[0])


# ---- 6. lifetime ----------------------------------------------------------------------------------------------------------------------------
def test_paths_outlive_the_model_and_its_extension():
    ref = reference(4)
    g = model_of(ref)
    sp = paths_of(g, ref)
    before, U = sp.paths(ref["Xs"]), sp.weights
    rng = np.random.default_rng(3)
    Xn = rng.uniform(-2, 2, (3, 30))
    g.add_data(Xn, np.sin(Xn.sum(0)))
    assert np.array_equal(sp.paths(ref["Xs"]), before) and np.array_equal(sp.weights, U)
    with paths_of(g, dict(ref, E=np.vstack([ref["E"], rng.standard_normal((30, U.shape[1]))]))) as sp_new:    # the extended model gives other paths
        assert sp_new.weights.shape[0] == U.shape[0] + 30
        assert nerr(sp_new.paths(ref["Xs"]), before) > 1e-6
    g.close()
    assert np.array_equal(sp.paths(ref["Xs"]), before)
    sp.close()
    with pytest.raises(nat.GprcError):
        sp.paths(ref["Xs"])
    print("lifetime: the bits of before after add_data and after the model is freed")


# ---- 7. errors --------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    ref = reference(1)                                              # gammaexp, n = 300, D = 6, S = 1
    lib = nat.lib()
    X, y, Xs, nu, phase, W, E = (ref[k] for k in ("X", "y", "Xs", "nu", "phase", "W", "E"))
    D, S = W.shape

    def refused_create(model, nu_=nu, phase_=phase, D_=D, W_=W, E_=E, S_=S, out=True):
        h = C.c_void_p()
        rc = lib.gprc_gpr_paths_create(model, nu_.ctypes.data if nu_ is not None else None, phase_.ctypes.data if phase_ is not None else None, D_,
                                       W_.ctypes.data if W_ is not None else None, E_.ctypes.data if E_ is not None else None, S_,
                                       C.byref(h) if out else None)
        return rc == nat.ERR_ARG and nat.last_error().startswith("paths_create:") and not h

    g = model_of(ref)
    assert refused_create(None)
    assert refused_create(g._model, D_=0) and refused_create(g._model, S_=0)
    assert refused_create(g._model, nu_=None) and refused_create(g._model, phase_=None) and refused_create(g._model, W_=None)
    assert refused_create(g._model, E_=None) and refused_create(g._model, out=False)
    Xc = np.linspace(-1, 1, 21).reshape(1, -1)
    gc = GPC(Xc, 2.0 * (Xc[0] > 0) - 1, cov_func(sqrexp, l=0.4), 1e-5)
    assert refused_create(gc._model)                                # a GPC model
    sg = SparseGPR(X, y, R.NOISE, kfun(ref["name"], ref["par"]), X[:, :40])
    assert refused_create(sg._model)                                # a sparse model
    sg.close()
    gm = GPR(X, y, R.NOISE, kfun(ref["name"], ref["par"]), devices=[0, 0])   # two virtual ranks on one GPU: rank 0's model is borrowed
    assert refused_create(gm._model)
    with pytest.raises(ValueError, match="refit"):
        gm.sample_paths(2, 8)
    gm.close()
    for k in (cov_func(polynomial, sigma=0.5, p=2.0), cov_func(linear, sigma=1.3)):   # kernels outside the eight
        gp = GPR(X, y, R.NOISE, k)
        assert refused_create(gp._model)
        with pytest.raises(ValueError):
            gp.sample_paths(2, 8)
        with pytest.raises(ValueError):
            gp.sample_paths(S, D, nu=nu, phase=phase, w=W, e=E)
        gp.close()
    with pytest.raises(ValueError):                                 # gammaexp has no frequency sampler: nu must be given
        g.sample_paths(2, 8)
    sp = paths_of(g, ref)

    def refused_eval(h, **kw):
        rc, _ = raw_eval(h, Xs, S, **kw)
        return rc == nat.ERR_ARG and nat.last_error().startswith("paths_eval:")

    assert refused_eval(None)
    out = np.empty((3, S), order="F")
    assert lib.gprc_gpr_paths_eval(sp._h, Xs.ctypes.data, 0, out.ctypes.data, 3) == nat.ERR_ARG and nat.last_error()
    assert lib.gprc_gpr_paths_eval(sp._h, None, 1, out.ctypes.data, 3) == nat.ERR_ARG and nat.last_error()
    assert lib.gprc_gpr_paths_eval(sp._h, Xs.ctypes.data, 1, None, 3) == nat.ERR_ARG and nat.last_error()
    X2 = np.asfortranarray(np.hstack([Xs, Xs]))
    assert lib.gprc_gpr_paths_eval(sp._h, X2.ctypes.data, 2, out.ctypes.data, 1) == nat.ERR_ARG and nat.last_error().startswith("paths_eval: ld_out")
    assert lib.gprc_gpr_paths_get_weights(sp._h, None) == nat.ERR_ARG and nat.last_error()
    assert lib.gprc_gpr_paths_get_weights(None, out.ctypes.data) == nat.ERR_ARG and nat.last_error()
    assert lib.gprc_gpr_paths_dims(None, None, None, None, None) == nat.ERR_ARG and nat.last_error()
    assert lib.gprc_gpr_paths_free(None) == 0
    assert nerr(sp.paths(Xs), ref["F"]) <= TOL                      # the paths are as usable as before
    sp.close()
    # after its context is destroyed a paths object refuses, as models do
    ctx2 = nat.Context(0)
    g2 = model_of(ref, ctx=ctx2)
    sp2 = paths_of(g2, ref)
    g2.close()
    ctx2.close()
    assert refused_eval(sp2._h)
    assert lib.gprc_gpr_paths_get_weights(sp2._h, out.ctypes.data) == nat.ERR_ARG and nat.last_error()
    sp2.close()
    gc.close()
    g.close()


# ---- 8. statistics through the Python API -----------------------------------------------------------------------------------------------
def test_statistics_of_the_paths_through_the_python_api():
    s = R.STAT
    X, y, Xs = R.stat_problem()
    nu, phase, W, E = R.stat_draws(0)
    g = GPR(X, y, s["noise"], kfun(s["name"], s["par"]))
    assert g.noise == s["noise"]
    with g.sample_paths(s["S"], s["D"], rng=np.random.default_rng(1234)) as sp:   # the draws of paths_ref.stat_draws(0), made by the library's host
        F = sp.paths(Xs)
    with g.sample_paths(s["S"], s["D"], nu=nu, phase=phase, w=W, e=E) as sp:
        assert np.array_equal(sp.paths(Xs), F)                      # the documented order of the draws
    g.close()
    mean, CD, _ = R.feature_covariance(s["name"], s["par"], X, y, s["noise"], nu, phase, Xs)
    zm, zc = R.stat_z_scores(F, mean, CD)
    ref = R.paths(s["name"], s["par"], X, y, s["noise"], nu, phase, W, E, Xs)[0]
    print("statistics: worst z of the mean %.2f, of the covariance %.2f; against the float64 reference %.2e" % (zm, zc, nerr(F, ref)))
    assert zm <= 5.0 and zc <= 5.0
