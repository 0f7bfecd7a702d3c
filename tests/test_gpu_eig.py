"""Accuracy of the sampling layer on the device -- sym_absmax, sym_copy, the three jacobi_* kernels, jacobi_offnorm, gather_scale_cols,
affine_lz and pack_dense of kernels_eig.hip with their host driver sym_eigen_dev / mvn_factor_dev -- through gprc_sym_eigen,
gprc_mvn_factor and gprc_mvn_sample, against the float64 model, the long-double checks and the counted bounds of tests/eig_ref.py
(whose docstring derives them; tests/test_eig_cpu.py proves model, checks and bounds on the CPU and shows every assertion here failing
for a deliberately wrong model).

Decomposition.  Every family of eig_ref.FAMILIES at m = 129, and dense PSD / indefinite at m = 1, 2, 3, 5, 64, 255, 256, 257, 511, 513 (the
second block of jacobi_angles), 1025 (the blockIdx.y stride loop of jacobi_rows) and 2051 (more than 1024 pairs: the stride loop of
jacobi_cols; the smallest odd size that runs both).  Asserted: resid, orth and -- where the spectrum is known -- the eigenvalues inside the
analytic bounds, values non-increasing, sweeps < 40; and up to m = 257, against the model on the same matrix,
    resid_dev <= rel(m) + 4 resid_model,      orth_dev <= 4 max(orth_model, m u),      sweeps_dev <= sweeps_model + 1.
The factor 4 is reasoned, not measured: fused multiply-adds and another summation order change which roundings occur, not how many, and
one sweep more adds under 20 %.  The measured fractions are in profiles/eig_accuracy.txt (GPRC_EIG_PROFILE=<path> writes the file).

Exact cases, scale (2^s A0 for s = +-300 bit for bit, s = -1000, -560, -520, 520, 1000 inside the same bounds), the ABI's inputs (non-finite
entries, the unread upper triangle, lda > m, device pointers, vectors_out = NULL), the eigen and the Cholesky branch of gprc_mvn_factor and
the product of gprc_mvn_sample are stated at each test.  A 1 x 1 covariance cannot reach the eigen branch: it factors or it is refused.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import gprc_amd  # noqa: E402,F401
from gprc_amd import _native as nat  # noqa: E402
from gpu_calls import step_time_limit  # noqa: E402,F401  (autouse fixture)
import eig_ref as R  # noqa: E402
import packed_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 5, 64, 255, 256, 257, 511, 513, 1025, 2051]
CASES = [(f, 129) for f in R.FAMILIES] + [(f, m) for m in SIZES for f in ("psd", "indefinite")]
MODEL_MAX = 257
_RECORD = []                                             # lines of profiles/eig_accuracy.txt


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("GPRC_EIG_PROFILE")
    if path and _RECORD:
        with open(path, "w") as f:
            f.write("\n".join(_RECORD) + "\n")


@pytest.fixture
def ctx():
    c = nat.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c
    torch.cuda.synchronize()
    c.close()


def padded(A, extra=0, fill=np.nan):
    """A as a column-major host array of pitch m + extra, the rows past m filled with `fill`"""
    m = A.shape[0]
    buf = np.full((m + extra, m), fill, order="F")
    buf[:m, :] = A
    return buf


def sym_eigen(ctx, A, lda=None, vectors=True, device=False):
    """gprc_sym_eigen on the column-major (lda x m) host array A: (values, vectors or None, sweeps); device=True passes device pointers for
    the matrix and both outputs"""
    A = np.asfortranarray(A)
    lda = A.shape[0] if lda is None else lda
    m = A.shape[1]
    assert A.shape[0] == lda
    sweeps = C.c_int(-1)
    if device:
        a = torch.from_numpy(np.ascontiguousarray(A.T)).cuda()
        val = torch.full((m,), float("nan"), dtype=torch.float64, device="cuda")
        vec = torch.full((m, m), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rc = nat.lib().gprc_sym_eigen(ctx.handle, a.data_ptr(), lda, m, val.data_ptr(), vec.data_ptr() if vectors else None, C.byref(sweeps))
        torch.cuda.synchronize()
        nat.check(rc)
        return val.cpu().numpy(), (vec.cpu().numpy().T.copy() if vectors else None), sweeps.value
    val = np.full(m, np.nan)
    vec = np.full((m, m), np.nan, order="F")
    nat.check(nat.lib().gprc_sym_eigen(ctx.handle, A.ctypes.data, lda, m, val.ctypes.data, vec.ctypes.data if vectors else None, C.byref(sweeps)))
    return val, (vec if vectors else None), sweeps.value


def mvn_factor_rc(ctx, cov, tol=1e-6):
    """(rc, L, method) of gprc_mvn_factor on the column-major (ld x m) host array cov"""
    cov = np.asfortranarray(cov)
    ld, m = cov.shape
    L = np.full((m, m), np.nan, order="F")
    method = C.c_int(0)
    rc = nat.lib().gprc_mvn_factor(ctx.handle, cov.ctypes.data, ld, m, float(tol), L.ctypes.data, C.byref(method))
    return rc, L, method.value


def mvn_sample(ctx, cov, mean, Z, tol=1e-6):
    cov, Z = np.asfortranarray(cov), np.asfortranarray(Z)
    ld, m = cov.shape
    nd = Z.shape[1]
    out = np.full((m, nd), np.nan, order="F")
    method = C.c_int(0)
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    nat.check(nat.lib().gprc_mvn_sample(ctx.handle, cov.ctypes.data, ld, m, mean.ctypes.data, float(tol), Z.ctypes.data, nd, out.ctypes.data, C.byref(method)))
    return out, method.value


@functools.lru_cache(maxsize=None)
def model_figures(name, m):
    A, lam = R.family(name, m)
    val, V, sweeps = R.jacobi(A)
    return R.check_decomposition(A, lam, val, V, sweeps)


def record(tag, m, c, cm=None):
    line = "%-22s m %5d  sweeps %2d  resid %.3e = %.4f of its bound  orth %.3e = %.4f" % (tag, m, c["sweeps"], c["resid"], c["resid"] / c["b"]["resid"],
                                                                                          c["orth"], c["orth"] / c["b"]["orth"] if c["b"]["orth"] else 0.0)
    if c["eig"] is not None:
        line += "  eig %.3e = %.4f" % (c["eig"], c["eig"] / c["b"]["eig"])
    if cm is not None:
        fr = R.model_fractions(c, cm, m)
        line += "  | model: sweeps %2d  resid / (rel + 4 resid_model) %.4f  orth / (4 max(orth_model, m u)) %.4f" % (cm["sweeps"], fr["resid"], fr["orth"])
    print(line)
    _RECORD.append(line)


# ---- decomposition -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,m", CASES, ids=["%s-%d" % c for c in CASES])
def test_decomposition_inside_the_bounds_and_beside_the_model(ctx, name, m):
    A, lam = R.family(name, m)
    val, V, sweeps = sym_eigen(ctx, A)
    assert np.isfinite(val).all() and np.isfinite(V).all()
    c = R.check_decomposition(A, lam, val, V, sweeps)
    cm = model_figures(name, m) if m <= MODEL_MAX else None
    record(name, m, c, cm)
    assert R.analytic_failures(c, val) == []
    if cm is not None:
        assert R.model_failures(c, cm, m) == []


# ---- exact cases -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,m", [("diagonal", 129), ("zero", 129), ("nearly-diagonal", 2)])
def test_inputs_without_off_diagonal_weight_come_back_exactly(ctx, name, m):
    """0 sweeps, the sorted diagonal bit for bit, the vectors exact permutation columns with ties in index order; nearly diagonal is
    [[1, .], [1e-160, 2]], whose off-diagonal square is 0 in float64"""
    A, _ = R.family(name, m)
    val, V, sweeps = sym_eigen(ctx, A)
    assert R.exact_failures(A, val, V, sweeps) == []


# ---- scale -----------------------------------------------------------------------------------------------------------------------------
def test_powers_of_two_change_no_bit_of_the_vectors_and_scale_the_values(ctx):
    """A = 2^s A0, A0 64 x 64 symmetric normal.  s = +-300: the values are 2^s times those of A0 bit for bit and the vectors are identical.
    s = -1000, -560, -520 (the squares of the entries underflow to zero or to subnormals), +520, +1000 (they overflow): no call is refused and
    the analytic bounds and the model comparison hold as at s = 0."""
    A0 = R.scale_base()
    cm = model_figures("indefinite", 64)
    val0, V0, s0 = sym_eigen(ctx, A0)
    for s in (300, -300):
        val, V, sw = sym_eigen(ctx, np.ldexp(A0, s))
        assert sw == s0 and np.array_equal(val, np.ldexp(val0, s)) and np.array_equal(V, V0)
    for s in (0, -1000, -560, -520, 520, 1000):
        A = np.ldexp(A0, s)
        val, V, sw = sym_eigen(ctx, A)
        assert np.isfinite(val).all() and np.isfinite(V).all()
        c = R.check_decomposition(A, None, val, V, sw)
        record("2^%d A0" % s, 64, c, cm)
        assert R.analytic_failures(c, val) == [] and R.model_failures(c, cm, 64) == []


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def test_what_is_read_and_what_is_refused(ctx):
    m = 129
    A = np.array(R.family("indefinite", m)[0])
    val, V, sweeps = sym_eigen(ctx, A)
    for bad in (np.nan, np.inf, -np.inf):                    # in the lower triangle, the diagonal included: the argument error
        for i, j in ((m - 1, 0), (77, 77), (128, 127)):
            B = np.asfortranarray(A.copy())
            B[i, j] = bad
            out = np.empty(m)
            rc = nat.lib().gprc_sym_eigen(ctx.handle, B.ctypes.data, m, m, out.ctypes.data, None, None)
            assert rc == nat.ERR_ARG and "non-finite" in nat.last_error()
    B = A.copy()
    B[np.triu_indices(m, 1)] = np.nan                        # the strict upper triangle is not read
    v2, V2, s2 = sym_eigen(ctx, B)
    assert s2 == sweeps and np.array_equal(v2, val) and np.array_equal(V2, V)
    v3, V3, s3 = sym_eigen(ctx, padded(B, 3), lda=m + 3)     # nor are the rows m .. lda - 1
    assert s3 == sweeps and np.array_equal(v3, val) and np.array_equal(V3, V)
    v4, V4, s4 = sym_eigen(ctx, padded(B, 3), lda=m + 3, device=True)   # device pointers in and out: the bits of host pointers
    assert s4 == sweeps and np.array_equal(v4, val) and np.array_equal(V4, V)
    v5, V5, s5 = sym_eigen(ctx, A, vectors=False)            # vectors_out = NULL
    assert V5 is None and s5 == sweeps and np.array_equal(v5, val)
    v6, _, s6 = sym_eigen(ctx, A, vectors=False, device=True)
    assert s6 == sweeps and np.array_equal(v6, val)


# ---- gprc_mvn_factor, eigen branch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [129, 257])
def test_factor_eigen_branch_on_a_known_spectrum(ctx, m):
    """lambda = 1 .. 1e-3 and four eigenvalues of -1e-9 lambda_1: clipped, so ||L L^T - A||_F <= 2 resid_bound ||A||_F + ||lambda_-||_2 and the squared
    column norms are max(lambda_k, 0) within (resid_bound + u) ||A||_F (eig_ref.factor_eigen_figures); a tail of -2e-6 lambda_1 is refused at
    tol = 1e-6; with lambda_min = +1e-13 lambda_1 either branch may answer and L L^T holds the bound of its branch"""
    lam = R.mvn_spectrum(m, -1e-9)
    A = R.from_spectrum(lam, 96000 + m)
    sweeps = sym_eigen(ctx, A, vectors=False)[2]
    rc, L, method = mvn_factor_rc(ctx, A)
    assert rc == 0 and method == 2 and np.isfinite(L).all()
    f = R.factor_eigen_figures(A, lam, L, sweeps)
    line = "mvn_factor eigen        m %5d  sweeps %2d  |L L^T - A|_F %.3e = %.4f of its bound  columns %.3e = %.4f" % (
        m, sweeps, f["llt"], f["llt"] / f["llt_bound"], f["cols"], f["cols"] / f["cols_bound"])
    print(line)
    _RECORD.append(line)
    assert sweeps < R.MAX_SWEEPS and f["llt"] <= f["llt_bound"] and f["cols"] <= f["cols_bound"]

    rc, _, _ = mvn_factor_rc(ctx, R.from_spectrum(R.mvn_spectrum(m, -2e-6), 97000 + m))
    assert rc == nat.ERR_NOT_PD

    lam = R.mvn_spectrum(m, 1e-13)
    A = R.from_spectrum(lam, 98000 + m)
    rc, L, method = mvn_factor_rc(ctx, A)
    assert rc == 0 and method in (1, 2) and np.isfinite(L).all()
    if method == 1:
        assert not np.triu(L, 1).any() and P.omega_chol(A, L) <= R.gamma(m + 1)
    else:
        f = R.factor_eigen_figures(A, lam, L, sym_eigen(ctx, A, vectors=False)[2])
        assert f["llt"] <= f["llt_bound"] and f["cols"] <= f["cols_bound"]
    print("lambda_min = 1e-13 lambda_1, m = %d: method %d" % (m, method))


@pytest.mark.parametrize("s", [-560, 520])
def test_factor_eigen_branch_far_from_one(ctx, s):
    """2^s times the rank-6 family at m = 129.  A = B B^T in float64 is within 6 u sqrt(6) ||A||_F < 15 u ||A||_F of a positive semi-definite
    matrix, which bounds its negative eigenvalues; compared after the exact division by 2^s (L by 2^(s/2))."""
    m = 129
    A0 = np.array(R.family("rank6", m)[0])
    A = np.ldexp(A0, s)
    sweeps = sym_eigen(ctx, A, vectors=False)[2]
    rc, L, method = mvn_factor_rc(ctx, A)
    assert rc == 0 and method == 2 and np.isfinite(L).all() and sweeps < R.MAX_SWEEPS
    f = R.factor_eigen_figures(A0, np.zeros(m), np.ldexp(L, -s // 2), sweeps)
    bound = f["llt_bound"] + 15 * R.U * float(R.fro(A0))
    print("rank 6 at 2^%d: |L L^T - A|_F %.3e = %.4f of its bound, %d sweeps" % (s, f["llt"], f["llt"] / bound, sweeps))
    assert f["llt"] <= bound


# ---- gprc_mvn_factor, Cholesky branch through pack_dense -------------------------------------------------------------------------------
def spd(m):
    B = np.random.default_rng(99000 + m).normal(size=(m, m))
    return R.sym_lower(B @ B.T + m * np.eye(m))


@pytest.mark.parametrize("m", [1, 127, 128, 129, 257])
def test_factor_cholesky_branch_reads_the_lower_triangle_at_any_pitch(ctx, m):
    """the upper triangle and the rows m .. ld - 1 of the input are NaN, ld = m + 3: |A - L L^T| <= gamma_{m+1} |L| |L|^T componentwise in
    longdouble, and the strict upper triangle of L is exactly 0"""
    A = spd(m)
    cov = A.copy()
    cov[np.triu_indices(m, 1)] = np.nan
    rc, L, method = mvn_factor_rc(ctx, padded(cov, 3))
    assert rc == 0 and method == 1 and np.isfinite(L).all()
    assert not np.triu(L, 1).any()
    w = P.omega_chol(A, L)
    line = "mvn_factor cholesky     m %5d  omega %.3f u = %.4f of gamma_{m+1}" % (m, w / R.U, w / R.gamma(m + 1))
    print(line)
    _RECORD.append(line)
    assert w <= R.gamma(m + 1)


# ---- affine_lz through gprc_mvn_sample ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 255, 257])
@pytest.mark.parametrize("branch", ["cholesky", "eigen"])
def test_draws_are_mean_plus_factor_times_z(ctx, branch, m):
    """|out - ref| <= gamma_{k+1} (|mean| + |L| |Z|) componentwise, ref in longdouble from the L that gprc_mvn_factor returned for the same
    covariance; k = i + 1 terms in row i on the Cholesky branch, m on the eigen branch; 1, 8, 9 and 17 draws: the 8-draw kernel alone, the
    1-draw kernel alone, and both"""
    rng = np.random.default_rng(99500 + m)
    if branch == "eigen" and m == 1:                         # a 1 x 1 covariance factors or is refused: there is no eigen branch to multiply with
        assert mvn_factor_rc(ctx, np.array([[0.0]]))[0] == nat.ERR_NOT_PD
        assert mvn_factor_rc(ctx, np.array([[2.0]]))[2] == 1
        return
    cov = spd(m) if branch == "cholesky" else np.array(R.family("rank6", m)[0])
    rc, L, method = mvn_factor_rc(ctx, cov)
    assert rc == 0 and method == (1 if branch == "cholesky" else 2)
    mean = rng.normal(size=m)
    for nd in (1, 8, 9, 17):
        Z = rng.normal(size=(m, nd))
        out, meth = mvn_sample(ctx, cov, mean, Z)
        assert meth == method and np.isfinite(out).all()
        fr = R.affine_fraction(out, mean, L, Z, lower=(method == 1))
        line = "affine_lz %-8s      m %5d  draws %2d  worst |out - ref| / bound %.4f" % (branch, m, nd, fr)
        print(line)
        _RECORD.append(line)
        assert fr <= 1.0
