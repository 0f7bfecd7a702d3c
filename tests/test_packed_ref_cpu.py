"""The yardstick of tests/test_gpu_blocks.py, checked without a GPU: the packed layout of tests/packed_ref.py round-trips, its
longdouble Cholesky holds its own bound against 50-digit mpmath, and EVERY matrix and bound the GPU tests use is run here with
LAPACK / BLAS in the device's place -- numpy.linalg.cholesky, scipy's solve_triangular and dpotrf, float64 matmul.  LAPACK
substitutes (no explicit inverses: kappa_blk = 1), so it must stay inside the plain gamma ceilings, and the generators must hit
every info index.  Measured at n = 1100 (seed 1): omega_chol of LAPACK = 7.9 / 19.5 / 22.4 / 29.1 u at cond 1e2 / 1e6 / 1e10 / 1e13,
17.4 u at cond 1e6 with grade 6: under 3 % of gamma_1101."""
import numpy as np
import pytest
import scipy.linalg as sl
from scipy.linalg import lapack

import packed_ref as R

U, gamma = R.U, R.gamma


@pytest.mark.parametrize("n", [1, 129, 512, 513, 1100])
def test_pack_unpack_round_trip(n):
    from gprc_amd import _native as nat
    lib = nat.lib()
    g = R.geometry(n)
    rng = np.random.default_rng(n)
    M = rng.normal(size=(n, n))
    M = M + M.T
    packed = R.pack(M, n)
    assert packed.size == g.packed_size == lib.gprc_packed_size(g.n_pad)
    Mp = np.eye(g.n_pad)
    Mp[:n, :n] = M
    for p in range(g.P):
        off, ld = lib.gprc_panel_offset(g.n_pad, p), g.n_pad - p * g.NB
        assert off == g.offsets[p] and lib.gprc_panel_elems(g.n_pad, p) == ld * g.NB
        for (i, c) in [(0, 0), (ld - 1, g.NB - 1), (ld // 2, 7), (3, 200)]:        # element (i, c) of panel p sits at off + i + c ld
            assert packed[off + i + c * ld] == Mp[p * g.NB + i, p * g.NB + c]
        assert np.array_equal(R.panel_view(packed, g, p), Mp[p * g.NB:, p * g.NB:(p + 1) * g.NB])
    Lo = R.unpack_lower(packed, g.n_pad)
    assert np.array_equal(Lo, np.tril(Mp))
    assert np.array_equal(Lo[n:, n:], np.eye(g.n_pad - n)) and not Lo[n:, :n].any()     # the padding is the identity


def test_winv_and_inv_block_layout():
    w = np.arange(2 * 16384, dtype=np.float64)
    assert R.winv_block(w, 1)[5, 7] == 16384 + 5 + 7 * 128                        # column-major 128 x 128 blocks
    inv = np.arange(2 * 512 * 512, dtype=np.float64)
    T, written = R.inv_block(inv, 1)
    assert T[300, 20] == 512 * 512 + 20 + 300 * 512                               # inv(L_pp)[r, c] at c + r NB
    assert written[300, 20] and written[130, 255] and not written[127, 128] and written.sum() == 10 * 128 * 128


def test_longdouble_cholesky_against_mpmath():
    """n = 24, cond 1e10: omega_chol of the longdouble column Cholesky, evaluated in 50-digit arithmetic, is <= gamma_25 at u = 2^-64."""
    import mpmath as mp
    mp.mp.dps = 50
    n = 24
    K = R.spd(n, 1e10, R.SEED)
    L, info = R.chol_ld(K)
    assert info == 0

    def exact(x):                                    # a longdouble as the exact sum of two doubles
        hi = float(x)
        return mp.mpf(hi) + mp.mpf(float(x - R.LD(hi)))

    Lm = [[exact(L[i, j]) for j in range(n)] for i in range(n)]
    w = mp.mpf(0)
    for i in range(n):
        for j in range(i + 1):
            s = sum(Lm[i][k] * Lm[j][k] for k in range(j + 1))
            den = sum(abs(Lm[i][k] * Lm[j][k]) for k in range(j + 1))
            w = max(w, abs(mp.mpf(float(K[i, j])) - s) / den)
    assert w <= gamma(n + 1, R.U_LD), float(w) / R.U_LD
    # and it agrees with LAPACK's float64 factor to float64 accuracy times the condition
    assert np.abs(np.asarray(L, dtype=float) - np.linalg.cholesky(K)).max() <= 1e10 * 64 * U


# ---- a. factor: LAPACK under the ceilings of the GPU test ----------------------------------------------------------------------
@pytest.mark.parametrize("case", R.FACTOR_CASES, ids=R.case_id)
def test_lapack_cholesky_is_inside_the_factor_ceiling(case):
    n, cond, grade = case
    K = R.spd(n, cond, R.SEED, grade)
    L = np.linalg.cholesky(K)
    n_pad = R.geometry(n).n_pad
    w = R.omega_chol(K, L)
    print("omega_chol(LAPACK) %s = %.2f u" % (R.case_id(case), w / U))
    assert w <= gamma(n_pad + 1)                     # kappa_blk = 1: LAPACK substitutes
    assert R.kappa_blk(R.pad_identity(L, n_pad), 128) >= 1.0


@pytest.mark.parametrize("scale", R.PIVOT_SCALES)
def test_lapack_cholesky_at_the_pivot_extremes(scale):
    K = scale * R.spd(513, 1e2, R.SEED)
    L = np.linalg.cholesky(K)
    assert np.isfinite(L).all()
    assert R.omega_chol(K, L) <= gamma(1024 + 1)


# ---- d, e. solves -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cond", R.SOLVE_CONDS)
def test_lapack_triangular_solves_are_inside_the_solve_ceiling(cond):
    n = 1100
    L = np.linalg.cholesky(R.spd(n, cond, R.SEED))
    rng = np.random.default_rng(R.SEED + 1)
    for b in (rng.normal(size=n), L @ np.ones(n)):
        for transpose in (False, True):
            x = sl.solve_triangular(L, b, lower=True, trans=1 if transpose else 0)
            assert R.omega_tri(L, x, b, transpose) <= gamma(1536 + 1), (cond, transpose)
    m_pad = 256                                      # the largest right-hand-side block of the solve_rows cases
    vt = rng.normal(size=(m_pad, n))
    V = sl.solve_triangular(L, vt.T, lower=True).T   # V L^T = vt
    assert R.omega_tri(L, V.T, vt.T) <= gamma(1536 + 1), cond


# ---- c. trailing updates ---------------------------------------------------------------------------------------------------------
SAMPLE = 48      # rows per target panel that the int64 / longdouble products (no BLAS: slow) cover


@pytest.mark.parametrize("call", R.UPDATE_CALLS, ids=[c[0] for c in R.UPDATE_CALLS])
def test_update_cases_exact_precondition_and_blas_inside_the_bound(call):
    name, n_pad, sources, targets = call
    g = R.geometry(n_pad)
    K = g.NB * (sources[1] - sources[0])
    # exact case: every partial sum of C - A B^T is an integer below 2^53, so ANY summation order gives the same float64
    packed = R.small_ints(g.packed_size, R.UPDATE_BITS, R.SEED)
    assert np.abs(packed).max() + K * 2.0 ** (2 * R.UPDATE_BITS) < 2.0 ** 53
    got, _ = R.update_expected(packed, g, sources, targets)
    pi = packed.astype(np.int64)
    want, _ = R.update_expected(pi, g, sources, targets, sample=SAMPLE)
    for q in got:
        assert np.array_equal(got[q][R.sample_rows(got[q].shape[0], SAMPLE)], want[q].astype(np.float64)), (name, q)
    # rounded case: the float64 BLAS product against longdouble, one-sided bound (the GPU test compares two rounded results: factor 2)
    packed = np.random.default_rng(R.SEED).normal(size=g.packed_size)
    got, mag = R.update_expected(packed, g, sources, targets)
    ref, _ = R.update_expected(packed.astype(R.LD), g, sources, targets, sample=SAMPLE)
    for q in got:
        rows = R.sample_rows(got[q].shape[0], SAMPLE)
        assert np.all(np.abs(got[q][rows] - ref[q]) <= gamma(K + 1) * mag[q][rows]), (name, q)


# ---- f, g. reductions -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", R.REDUCE_COLS)
def test_reduce_cases_exact_precondition_and_numpy_inside_the_bound(cols):
    rows = max(R.REDUCE_ROWS)
    v, w = R.small_ints((rows, cols), R.REDUCE_BITS, cols), R.small_ints(cols, R.REDUCE_BITS, cols + 1)
    assert cols * 2.0 ** (2 * R.REDUCE_BITS) < 2.0 ** 53
    vi, wi = v.astype(np.int64), w.astype(np.int64)
    assert np.array_equal(v @ w, (vi @ wi).astype(np.float64)) and np.array_equal((v * v).sum(1), (vi * vi).sum(1).astype(np.float64))
    rng = np.random.default_rng(cols)
    v, w = rng.normal(size=(rows, cols)), rng.normal(size=cols)
    assert np.all(np.abs(v @ w - R.rows_dot_ld(v, w)) <= gamma(cols) * (np.abs(v) @ np.abs(w)))
    assert np.all(np.abs((v * v).sum(1) - R.rows_dot_ld(v)) <= gamma(cols) * (v * v).sum(1))


def test_logp_in_float64_is_inside_the_bound():
    n, cond, grade = R.FACTOR_CASES[-1]
    L = np.linalg.cholesky(R.spd(n, cond, R.SEED, grade))
    d = np.diag(L)
    assert np.log10(d.max() / d.min()) > 8           # the graded factor's diagonal spans many decades
    rng = np.random.default_rng(R.SEED + 2)
    y, alpha = rng.normal(size=n), rng.normal(size=n)
    got = -0.5 * (y @ alpha) - np.log(d).sum() - n / 2 * np.log(2 * np.pi)
    ref, mag = R.logp_ld(L, n, y, alpha)
    assert abs(got - ref) <= gamma(n + 2) * mag


# ---- i. info ------------------------------------------------------------------------------------------------------------------------
def test_dpotrf_reports_every_k_of_the_list():
    for k in R.INFO_KS:
        M = R.not_pd_at(R.INFO_N, k, R.SEED)
        if k > 1:
            np.linalg.cholesky(M[:k - 1, :k - 1])    # leading minors 1 .. k-1 are positive definite
        _, info = lapack.dpotrf(M, lower=1)
        assert info == k, (k, info)


def test_rank_one_matrix_fails_at_the_second_minor():
    M = R.rank_one(600, R.SEED)
    _, info = lapack.dpotrf(M, lower=1)
    assert info == 2
