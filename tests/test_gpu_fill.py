"""Elementwise accuracy of every kernel-value form on the device against the longdouble reference and the derived bounds of
tests/fill_ref.py (whose docstring counts them rounding by rounding; tests/test_fill_cpu.py proves reference, bounds and inputs on the CPU):

    |got - ref| <= (cond (d + A) + E + C) u max(|ref|, 1e-290)        per element

on points whose pair distances span 20 decades, with exact duplicates, at l = 1 and at a length scale that takes the far tail below 1e-290.
Shapes: nA = 257, nB = 130 -- a 3 x 3 grid of 128 x 64 tiles with one interior tile, ragged last tiles both ways and an odd leading
dimension (fill_kernel<.., VEC2 = false, ..>) -- and nA = 256 with an even one (VEC2 = true and its interior fast path).

Entry points:  1 gprc_kernel_matrix (PAD_NONE)   2 gprc_kernel_colwise   3 gprc_dev_fill_panel (PAD_IDENTITY)   4 gprc_dev_fill_cross (PAD_ZERO)
               5 kernel_value<KID> through gprc_dev_kernel_gemm and 6 pair_weight<KID> through gprc_dev_kernel_gemm_grad, both with U = I.

Every switch case and early return, and the parameters that reach it (fill_ref.cases(), fill_ref.gemm_cases()):

    finish<KID> (kernels_fill.hip)                      parameters
    constant        return p[0]                         c = 3.7
    linear          return s                            sigma = 0.3;  17 and 33 per-coordinate sigmas
    polynomial      table case 3 / 4 / 5 / 6 / 7        p = 3 / 4 / 5 / 6 / 7, each at sigma = -0.25 (70 % of the bases negative) and 2000 (none)
                    table default                       p = 8
                    r_pow: y == 2, x * x                p = 2
                    r_pow: pow                          p = 1, 9, 2.5 (2.5: NaN where the base is negative, as R's `^`)
    sqrexp          quotient, exp                       l = 1 and 0.05, at every d of 1, 3, 16, 17, 33
    sqrexp_ard      exp(-0.5 s)                         d = 3, 17, 33, scales over two decades, times 1 and times a small factor
    matern32 / 52   isotropic: quotient, sqrt, exp      l = 1 and sqrt(3) / 230, sqrt(5) / 230
    matern32 / 52_ard   u = 3 s (5 s)                   d = 16 (3/2), 33 (5/2)
    gammaexp        g == 2: sqrt(s) / l, r_pow x * x    gamma = 2
                    root form h = 1 / 2 / 3             gamma = 0.5 / 1 / 1.5
                    exp(g/2 log u)                      gamma = 0.1, 1.3, 1.999          (s = 0: log = -Inf, value exactly 1: the duplicates)
    rationalquadratic   al == 2: 1 / (q q)              alpha = 2
                    rsqrt table case 1 / 2 / 3 / 5 / 6 / 7 / default     alpha = 0.5 / 1 / 1.5 / 2.5 / 3 / 3.5 / 4
                    rsqrt table case 4                  unreachable: alpha = 2 has returned at `al == 2.0`
                    exp(-al log q)                      alpha = 4.5, 0.7, 1e-3, 1e3
    kernel_value<KID>, pair_weight<KID> (pair_tile.h)   each of the eight kernels at d = 1, 3, 17, 20, unit and small scale alternating
    gammaexp        !(s > 0): return 1 (value), 0 (weight)     the duplicates;   s > 0: gamma = 0.5, 1.3, 2, 1
    rationalquadratic, sqrexp, sqrexp_ard, matern (ARD or not: one expression each)     alpha = 0.7, 1e3, 2, 1.5

With GPRC_FILL_PROFILE=<path> in the environment the worst observed fraction of the bound per (entry point, branch) is written to <path>,
with what the device returns where a Matern reference lies between 2^-1022 and 1e-290 (recorded, not asserted: profiles/fill_accuracy.txt).
"""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import gprc_amd  # noqa: E402,F401
from gprc_amd import _native as nat  # noqa: E402
from gpu_calls import step_time_limit  # noqa: E402,F401  (autouse fixture)
import fill_ref as R  # noqa: E402
import packed_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = R.cases()
IDS = [R.case_id(c) for c in CASES]
_WORST = {}                                              # (entry point, branch) -> worst fraction of the bound
_BAND = {}                                               # Matern kernel -> (entries, worst |got - ref| / (u |ref|)) for 2^-1022 < ref < F


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("GPRC_FILL_PROFILE")
    if path and _WORST:
        with open(path, "w") as f:
            f.write("%-24s %-48s %s\n" % ("entry point", "branch", "worst |got - ref| / bound"))
            for (entry, br), w in sorted(_WORST.items()):
                f.write("%-24s %-48s %.4f\n" % (entry, br, w))
            f.write("constant under kernel_matrix, kernel_colwise, dev_fill_cross: 0 of a bound of 0 -- the parameter comes back as it went in, the check there is "
                    "equality (dev_fill_panel: the rounding of value + noise on the diagonal)\n")
            f.write("\nMatern references between 2^-1022 and 1e-290 (gprc_kernel_matrix; recorded, not asserted: the check there is absolute)\n")
            for kind, (cnt, w) in sorted(_BAND.items()):
                f.write("%-24s %6d entries, worst |got - ref| / (u |ref|) %.3g\n" % (kind, cnt, w))


def note(entry, kind, par, fr):
    worst = float(np.max(fr)) if np.size(fr) else 0.0
    key = (entry, R.branch(kind, par))
    _WORST[key] = max(_WORST.get(key, 0.0), worst)
    return worst


@pytest.fixture
def ctx():
    c = nat.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c
    torch.cuda.synchronize()
    c.close()


def dev(a):
    """a host array on the device, complete before the library's stream can touch it"""
    t = torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda()   # a copy: fill_ref's cached points are read-only
    torch.cuda.synchronize()
    return t


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def ref_and_bound(index):
    """(values, bound) of case `index` at nA = 257, shared by the matrix and the colwise test; longdouble, not to be written to"""
    kind, par, d, _ = CASES[index]
    A, B = R.points(d)
    ref = R.reference(kind, par, A, B)
    return ref.k, R.fill_bound(kind, par, d, ref)


def kernel_matrix(ctx, kind, par, A, B, pitch_extra=3):
    """gprc_kernel_matrix into a host array whose pitch exceeds nA: (nA x nB result, the rows past nA)"""
    nA, nB, d = A.shape[0], B.shape[0], A.shape[1]
    _, pp, npar = nat.params_array(par)
    out = np.full((nB, nA + pitch_extra), np.nan)
    A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)
    nat.check(nat.lib().gprc_kernel_matrix(ctx.handle, R.KERNEL_ID[kind], pp, npar, A.ctypes.data, d, nA, B.ctypes.data, nB, out.ctypes.data, nA + pitch_extra))
    return out[:, :nA].T, out[:, nA:]


# ---- 1. gprc_kernel_matrix ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nA", [R.NA, R.NA_EVEN], ids=["odd-ld", "even-ld"])
@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_kernel_matrix_elementwise(ctx, index, nA):
    kind, par, d, scale = CASES[index]
    A, B = R.points(d, nA)
    if nA == R.NA:
        k, bound = ref_and_bound(index)
    else:
        ref = R.reference(kind, par, A, B)
        k, bound = ref.k, R.fill_bound(kind, par, d, ref)
    got, past = kernel_matrix(ctx, kind, par, A, B)
    assert np.isnan(past).all()                                # the host rows past nA are not touched
    fr = R.fractions(got, k, bound)                            # asserts that the NaN mask is the reference's
    worst = note("kernel_matrix", kind, par, fr)
    print("kernel_matrix %s nA = %d: worst fraction of the bound %.3f" % (IDS[index], nA, worst))
    if kind.startswith("matern"):
        kf = np.abs(k.astype(np.float64))
        band = (kf > 2.0 ** -1022) & (kf < R.F)
        if band.any():
            rel = float((np.abs(got.astype(R.LD) - k)[band] / (R.U * np.abs(k)[band])).max())
            cnt, w = _BAND.get(kind, (0, 0.0))
            _BAND[kind] = (cnt + int(band.sum()), max(w, rel))
    assert worst <= 1.0
    if kind in R.STATIONARY:
        for i, j in R.DUPLICATES:
            assert got[i, j] == 1.0
    if nA == R.NA:                                             # K(A, A): the same bits on both sides of the diagonal, the exact value on it
        sym, _ = kernel_matrix(ctx, kind, par, A, A)
        assert np.array_equal(sym, sym.T, equal_nan=True)
        i, j = R.DUPLICATE_IN_A
        if kind in R.STATIONARY:
            assert (np.diag(sym) == 1.0).all() and sym[i, j] == 1.0 and sym[j, i] == 1.0
        elif kind == "constant":
            assert (sym == par[0]).all()
        else:
            assert sym[i, j] == sym[i, i] or np.isnan(sym[i, i])


# ---- 2. gprc_kernel_colwise --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_kernel_colwise_elementwise(ctx, index):
    """out[c] = k(x_c, y_c) on the pairs (A[i], B[i mod 130]), i < 257: two blocks of the kernel, the second ragged"""
    kind, par, d, scale = CASES[index]
    A, B = R.points(d)
    k, bound = ref_and_bound(index)
    ii, jj = np.arange(R.NA), np.arange(R.NA) % R.NB
    x, y = np.ascontiguousarray(A[ii]), np.ascontiguousarray(B[jj])
    _, pp, npar = nat.params_array(par)
    out = np.full(R.NA + 2, np.nan)
    nat.check(nat.lib().gprc_kernel_colwise(ctx.handle, R.KERNEL_ID[kind], pp, npar, x.ctypes.data, y.ctypes.data, d, R.NA, out.ctypes.data))
    assert np.isnan(out[R.NA:]).all()
    worst = note("kernel_colwise", kind, par, R.fractions(out[:R.NA], k[ii, jj], bound[ii, jj]))
    print("kernel_colwise %s: worst fraction of the bound %.3f" % (IDS[index], worst))
    assert worst <= 1.0


# ---- 3. gprc_dev_fill_panel ----------------------------------------------------------------------------------------------------------------
FAMILY_IDS = ["%s-%s-d%d" % (k, "_".join("%.3g" % v for v in p[:2]), d) for k, p, d in R.FAMILY_CASES]


@pytest.mark.parametrize("case", R.FAMILY_CASES, ids=FAMILY_IDS)
def test_fill_panel_elementwise(ctx, case):
    """n = 600: two panels, 424 padded rows.  Inside the data the bound (the diagonal: value + noise, one more rounding); the exact identity in
    the padding; nothing outside the panel."""
    kind, par, d = case
    n, noise = 600, 0.1
    g = P.geometry(n)
    assert g.P == 2 and g.n_pad - n == 424
    X, _ = R.points(d, n)
    ref = R.reference(kind, par, X, X)
    k, bound = ref.k.copy(), R.fill_bound(kind, par, d, ref)
    di = np.diag_indices(n)
    k[di] = k[di] + R.LD(noise)
    bound[di] = bound[di] + R.U * np.abs(k[di])
    Xd = dev(X)
    _, pp, npar = nat.params_array(par)
    guard = 1024
    worst = 0.0
    for p in range(g.P):
        buf = dev(np.full(g.packed_size + guard, np.nan))
        nat.check(nat.lib().gprc_dev_fill_panel(ctx.handle, R.KERNEL_ID[kind], pp, npar, Xd.data_ptr(), d, n, g.n_pad, noise, buf.data_ptr(), p))
        flat = host(buf)
        sl = g.panel_slice(p)
        outside = np.ones(flat.size, dtype=bool)
        outside[sl] = False
        assert np.isnan(flat[outside]).all()                   # the other panel and the guard behind the buffer
        panel = P.panel_view(flat[:g.packed_size], g, p)       # rows [p NB, n_pad) x columns [p NB, (p + 1) NB)
        r0, c0 = p * g.NB, p * g.NB
        rows, cols = np.arange(r0, g.n_pad), np.arange(c0, c0 + g.NB)
        rin, cin = rows < n, cols < n
        data = panel[np.ix_(rin, cin)]
        want_k, want_b = k[np.ix_(rows[rin], cols[cin])], bound[np.ix_(rows[rin], cols[cin])]
        worst = max(worst, note("dev_fill_panel", kind, par, R.fractions(data, want_k, want_b)))
        eye = (rows[:, None] == cols[None, :]).astype(np.float64)
        pad = ~(rin[:, None] & cin[None, :])
        assert np.array_equal(panel[pad], eye[pad])            # exactly 1 on the diagonal of the padding, exactly 0 elsewhere in it
    print("dev_fill_panel %s: worst fraction of the bound %.3f" % (case[0], worst))
    assert worst <= 1.0


# ---- 4. gprc_dev_fill_cross ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.FAMILY_CASES, ids=FAMILY_IDS)
def test_fill_cross_elementwise(ctx, case):
    """m = 129 in m_pad = 256, n = 513 in n_pad = 1024: the bound inside, exact zeros in the padding, the ld gap untouched"""
    kind, par, d = case
    m, m_pad, n = 129, 256, 513
    n_pad = P.geometry(n).n_pad
    ld = m_pad + 128
    X, Xs = R.points(d, n, m)
    ref = R.reference(kind, par, Xs, X)                        # m x n
    bound = R.fill_bound(kind, par, d, ref)
    buf = np.random.default_rng(d).normal(size=(n_pad, ld))
    Xd, Xsd, vt = dev(X), dev(Xs), dev(buf)
    _, pp, npar = nat.params_array(par)
    nat.check(nat.lib().gprc_dev_fill_cross(ctx.handle, R.KERNEL_ID[kind], pp, npar, Xsd.data_ptr(), d, m, m_pad, Xd.data_ptr(), n, n_pad, vt.data_ptr(), ld))
    out = host(vt).reshape(n_pad, ld)
    worst = note("dev_fill_cross", kind, par, R.fractions(out[:n, :m].T, ref.k, bound))
    print("dev_fill_cross %s: worst fraction of the bound %.3f" % (case[0], worst))
    assert worst <= 1.0
    assert not out[:n, m:m_pad].any() and not out[n:, :m_pad].any()
    assert np.array_equal(out[:, m_pad:], buf[:, m_pad:])


# ---- 5, 6. kernel_value and pair_weight through the generated-operand products ---------------------------------------------------------------
GEMM_CASES = R.gemm_cases()
GEMM_IDS = ["%s-%s-d%d" % (k, "_".join("%.3g" % v for v in p[:2]), d) for k, p, d in GEMM_CASES]


def identity_operand(cols):
    """U = I as the C-ordered host image of a cols x cols column-major matrix of pitch cols + 3, NaN in the pitch's padding"""
    Bd = np.full((cols, cols + 3), np.nan)
    Bd[:, :cols] = np.eye(cols)
    return Bd, cols + 3


@pytest.mark.parametrize("case", GEMM_CASES, ids=GEMM_IDS)
def test_kernel_value_through_an_identity_product(ctx, case):
    """out = K(A, B) I on the f64 matrix cores: every term but one of a sum is an exact zero, so out[i, j] is kernel_value's k(a_i, b_j)
    itself; rows = 257, cols = S = 130.  Duplicates give exactly 1."""
    kind, par, d = case
    A, B = R.points(d)
    rows, cols = R.NA, R.NB
    ref = R.reference(kind, par, A, B)
    bound = R.value_bound(kind, par, d, ref, A, B)
    Bd, ldb = identity_operand(cols)
    adev, pdev, bdev = dev(A), dev(B), dev(Bd)
    ld = rows + 1
    out = dev(np.full((cols, ld), np.nan))
    _, pp, npar = nat.params_array(par)
    nat.check(nat.lib().gprc_dev_kernel_gemm(ctx.handle, R.KERNEL_ID[kind], pp, npar, adev.data_ptr(), rows, pdev.data_ptr(), cols, d, bdev.data_ptr(), ldb,
                                             cols, out.data_ptr(), ld))
    got = host(out)
    assert np.isnan(got[:, rows:]).all()
    got = got[:, :rows].T
    worst = note("kernel_value (gemm)", kind, par, R.fractions(got, ref.k, bound))
    print("kernel_value %s: worst fraction of the bound %.3f" % (GEMM_IDS[GEMM_CASES.index(case)], worst))
    assert worst <= 1.0
    for i, j in R.DUPLICATES:
        assert got[i, j] == 1.0


@pytest.mark.parametrize("case", GEMM_CASES, ids=GEMM_IDS)
def test_pair_weight_through_an_identity_product(ctx, case):
    """dout[i, j, c] = -t_c h(a_i, b_j) (a_ic - b_jc) with U = I, against the longdouble h and t of tests/kernel_ref.py's table; a coinciding
    pair contributes an exact 0 for every kernel, gammaexp with gamma < 1 included"""
    kind, par, d = case
    A, B = R.points(d)
    rows, cols = R.NA, R.NB
    want, bound = R.weight_reference(kind, par, A, B)          # d x rows x cols
    Bd, ldb = identity_operand(cols)
    adev, pdev, bdev = dev(A), dev(B), dev(Bd)
    ld = rows + 1
    out = dev(np.full((d, cols, ld), np.nan))
    _, pp, npar = nat.params_array(par)
    nat.check(nat.lib().gprc_dev_kernel_gemm_grad(ctx.handle, R.KERNEL_ID[kind], pp, npar, adev.data_ptr(), rows, pdev.data_ptr(), cols, d, bdev.data_ptr(),
                                                  ldb, cols, out.data_ptr(), ld))
    got = host(out)
    assert np.isnan(got[:, :, rows:]).all()
    got = got[:, :, :rows].transpose(0, 2, 1)                  # c, i, j
    worst = note("pair_weight (gemm_grad)", kind, par, R.fractions(got, want, bound))
    print("pair_weight %s: worst fraction of the bound %.3f" % (GEMM_IDS[GEMM_CASES.index(case)], worst))
    assert worst <= 1.0
    for i, j in R.DUPLICATES:
        assert not got[:, i, j].any()
