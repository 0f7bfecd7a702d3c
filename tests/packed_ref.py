"""Helpers of tests/test_gpu_blocks.py and tests/test_packed_ref_cpu.py: the packed block-column layout on the host, an
extended-precision (numpy.longdouble, 64-bit significand) reference for Cholesky factors, triangular solves and reductions,
componentwise backward-error measures, seeded matrix generators, and the cases both test files run.  No GPU and no torch.

Layout (include/gprc_native.h): n_pad = gprc_pad(n); panel p holds rows [p NB, n_pad) x columns [p NB, (p+1) NB), column-major
with leading dimension n_pad - p NB, at element offset gprc_panel_offset(n_pad, p).  winv: one column-major 128 x 128 block per 128
columns.  inv: per panel the NB x NB inverse of the diagonal block, stored transposed with leading dimension NB.

Measures, u = 2^-53, gamma_k = k u / (1 - k u)  (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.):
    omega_chol = max_{i >= j} |K - L L^T|_ij / (|L| |L^T|)_ij        a backward-stable Cholesky: <= gamma_{n+1}     (Thm 10.3)
    omega_tri  = max_i |b - T x|_i / (|T| |x|)_i, T = L or L^T      substitution: <= gamma_n                      (Thm 8.5)
Residuals are evaluated in longdouble (their own rounding, 2^-64 relative, is 2^-11 of u per term), denominators in float64.
"""
import math
import os
import sys

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, (
    "tests/packed_ref.py needs an extended-precision numpy.longdouble (x87 80-bit or wider: eps <= 2^-63); this platform's has eps = %g, "
    "so the reference would be no more accurate than the float64 results it judges" % float(np.finfo(LD).eps))

U = 2.0 ** -53
U_LD = 2.0 ** -64


def gamma(k, u=U):
    return k * u / (1.0 - k * u)


# ---- the cases of the accuracy tests (tests/test_gpu_blocks.py; tests/test_packed_ref_cpu.py runs them through LAPACK) -------------
FACTOR_CASES = [(1, 1.0, 0), (129, 1e2, 0), (512, 1e6, 0), (513, 1e6, 0), (1100, 1e2, 0), (1100, 1e6, 0), (1100, 1e10, 0), (1100, 1e13, 0),
                (1100, 1e6, 6)]                       # (n, cond, grade) of spd(); the seed is SEED
PIVOT_SCALES = [1e-280, 1e280]                        # times spd(513, 1e2)
SOLVE_CONDS = [1e2, 1e6, 1e10]                        # the n = 1100 rungs the solves run on
SOLVE_ROWS_SHAPES = [(128, 128), (128, 256), (256, 384)]   # (m_pad, ld)
REDUCE_ROWS = [128, 256]
REDUCE_COLS = [1, 3, 4, 5, 511, 512, 513, 1027]
INFO_N = 1300
INFO_KS = [1, 2, 16, 17, 128, 129, 511, 512, 513, 640, 1024, 1025, 1300]
SEED = 1
UPDATE_BITS, REDUCE_BITS = 10, 20


def case_id(case):
    n, cond, grade = case
    return "n%d-cond%.0e-grade%d" % (n, cond, grade)


# ---- generators ----------------------------------------------------------------------------------------------------------------
def spd(n, cond, seed, grade=0):
    """Q diag(logspace(0, -log10 cond)) Q^T, symmetrised; grade = g then scales rows and columns by 10^U(-g, g)."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    ev = np.logspace(0, -np.log10(cond), n)
    A = (Q * ev) @ Q.T
    A = (A + A.T) / 2
    if grade:
        s = 10.0 ** rng.uniform(-grade, grade, n)
        A = A * s[:, None] * s[None, :]
    return A


def not_pd_at(n, k, seed):
    """Symmetric, leading minors 1 .. k-1 positive definite (those of L0 L0^T, untouched), pivot k about -0.25."""
    rng = np.random.default_rng(seed)
    L0 = np.tril(rng.normal(size=(n, n))) / np.sqrt(n)
    L0[np.diag_indices(n)] = rng.uniform(0.5, 1.5, n)
    M = L0 @ L0.T
    M[k - 1, k - 1] -= L0[k - 1, k - 1] ** 2 + 0.25
    return M


def rank_one(n, seed):
    """v v^T, exactly singular from the second leading minor on IN FLOATING POINT too: v holds non-zero integers of at most 3 bits and
    v_0 = 2, so pivot 1 is 4, 1 / sqrt(4) and column 1 (= v) are exact in any arithmetic, and pivot 2 is v_1^2 - v_1^2 = 0."""
    rng = np.random.default_rng(seed)
    v = rng.integers(1, 8, size=n, endpoint=True) * rng.choice([-1, 1], size=n)
    v[0] = 2
    v = v.astype(np.float64)
    return np.outer(v, v)


def small_ints(shape, bits, seed):
    """integers in [-2^bits, 2^bits] as float64"""
    return np.random.default_rng(seed).integers(-2 ** bits, 2 ** bits, size=shape, endpoint=True).astype(np.float64)


# ---- packed layout -------------------------------------------------------------------------------------------------------------
def geometry(n):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import gprc_amd  # noqa: F401  (alias loader)
    from gprc_amd.distributed import Geometry
    return Geometry(n)


def panel_view(packed, g, p):
    """panel p as an (n_pad - p NB) x NB array in matrix orientation: a view into packed"""
    ld = g.n_pad - p * g.NB
    return packed[g.panel_slice(p)].reshape(g.NB, ld).T


def pack(M, n):
    """Packed block-column buffer of M (n x n) padded with the identity; the diagonal blocks carry both triangles of M, as fill_panel
    writes them."""
    g = geometry(n)
    Mp = np.eye(g.n_pad)
    Mp[:n, :n] = M
    packed = np.zeros(g.packed_size)
    for p in range(g.P):
        panel_view(packed, g, p)[:, :] = Mp[p * g.NB:, p * g.NB:(p + 1) * g.NB]
    return packed


def unpack_lower(packed, n_pad):
    """n_pad x n_pad lower factor, the upper part zero"""
    g = geometry(n_pad)
    assert g.n_pad == n_pad
    L = np.zeros((n_pad, n_pad))
    for p in range(g.P):
        L[p * g.NB:, p * g.NB:(p + 1) * g.NB] = panel_view(packed, g, p)
    return np.tril(L)


def winv_block(winv, j):
    """128 x 128 inverse of the j-th 128 x 128 diagonal block of L"""
    return winv[j * 16384:(j + 1) * 16384].reshape(128, 128).T


def inv_block(inv, p, NB=512):
    """(T, written): T[r, c] = inv(L_pp)[r, c] of panel p (stored transposed, leading dimension NB) and the mask of the entries the
    kernels write: 128-block row >= 128-block column (the rest of the buffer is never touched)."""
    T = inv[p * NB * NB:(p + 1) * NB * NB].reshape(NB, NB)
    blk = np.arange(NB) // 128
    return T, blk[None, :] <= blk[:, None]


# ---- extended-precision reference ------------------------------------------------------------------------------------------------
def chol_ld(A):
    """column Cholesky in longdouble: (L, info), info = 0 or LAPACK's (first non-positive pivot, 1-based)"""
    A = np.asarray(A, dtype=LD)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            return L, j + 1
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return L, 0


def chol_residual_columns(K, L):
    """generator of (j, |K - L L^T|[j:, j]) in longdouble, column by column (n^3 / 3; a full L @ L.T costs six times that)"""
    Kl, Ll = np.asarray(K, dtype=LD), np.asarray(L, dtype=LD)
    for j in range(Kl.shape[0]):
        yield j, np.abs(Kl[j:, j] - Ll[j:, :j + 1] @ Ll[j, :j + 1])


def _ratio_max(r, den):
    """max r / den with 0 / 0 = 0 and r / 0 = inf; r longdouble, den float64"""
    r, den = np.asarray(r), np.asarray(den)
    if r.size == 0:
        return 0.0
    zero = den == 0
    if np.any(zero & (r != 0)):
        return math.inf
    q = r / np.where(zero, 1.0, den)
    return float(q.max())


def omega_chol(K, L):
    """max over the lower triangle of |K - L L^T| / (|L| |L^T|); L float64 lower-triangular"""
    L = np.asarray(L, dtype=np.float64)
    den = np.abs(L) @ np.abs(L).T
    w = 0.0
    for j, r in chol_residual_columns(K, L):
        w = max(w, _ratio_max(r, den[j:, j]))
    return w


def tri_times(L, X, transpose=False):
    """L X (or L^T X) in longdouble; X a vector or a matrix of columns"""
    Ll = np.asarray(L, dtype=LD)
    return (Ll.T if transpose else Ll) @ np.asarray(X, dtype=LD)


def omega_tri(L, X, B, transpose=False):
    """max over all entries of |B - T X| / (|T| |X|), T = L or L^T.  (For V L^T = B with rows as right-hand sides: X = V^T, B = B^T.)"""
    L = np.asarray(L, dtype=np.float64)
    T = L.T if transpose else L
    r = np.abs(np.asarray(B, dtype=LD) - tri_times(L, X, transpose))
    return _ratio_max(r, np.abs(T) @ np.abs(np.asarray(X, dtype=np.float64)))


def kappa_inf_lower(T):
    """kappa_inf of a lower-triangular block, through its explicit inverse (scipy, float64)"""
    import scipy.linalg as sl
    Ti = sl.solve_triangular(T, np.eye(T.shape[0]), lower=True)
    return float(np.abs(T).sum(1).max() * np.abs(Ti).sum(1).max())


def kappa_blk(L, size):
    """largest kappa_inf among the size x size diagonal blocks of the lower factor L (its dimension a multiple of size)"""
    return max(kappa_inf_lower(L[c:c + size, c:c + size]) for c in range(0, L.shape[0], size))


def pad_identity(L, n_pad):
    Lp = np.eye(n_pad)
    n = L.shape[0]
    Lp[:n, :n] = L
    return Lp


def rows_dot_ld(V, w=None):
    """out[i] = sum_j V[i, j] w[j]  (w None: sum_j V[i, j]^2) in longdouble, returned as longdouble"""
    Vl = np.asarray(V, dtype=LD)
    return (Vl * Vl).sum(1) if w is None else Vl @ np.asarray(w, dtype=LD)


def logp_ld(L, n, y, alpha):
    """(-1/2 y.alpha - sum log L_ii - n/2 log 2 pi, the bound's magnitude 1/2 sum|y alpha| + sum|log L_ii| + n/2 log 2 pi), longdouble"""
    d = np.asarray(np.diag(L)[:n], dtype=LD)
    yl, al = np.asarray(y[:n], dtype=LD), np.asarray(alpha[:n], dtype=LD)
    c = LD(n) / 2 * np.log(2 * np.pi * LD(1))
    ld = np.log(d)
    return -(yl * al).sum() / 2 - ld.sum() - c, float(np.abs(yl * al).sum() / 2 + np.abs(ld).sum() + c)


# ---- trailing updates on a packed buffer that is not a factor ---------------------------------------------------------------------
UPDATE_CALLS = [                                       # (name, n_pad, source panels [p0, p1), targets (q_begin, q_end, q_stride))
    ("trailing-all", 1536, (0, 1), (1, 3, 1)),
    ("range-3-sources", 2048, (0, 3), (3, 4, 1)),
    ("trailing-stride-2", 2048, (0, 1), (1, 4, 2)),
]


def sample_rows(ld, sample):
    """`sample` row indices of a panel, evenly spread, first and last included (None: all)"""
    return np.arange(ld) if sample is None else np.unique(np.linspace(0, ld - 1, sample).astype(np.int64))


def update_expected(packed, g, sources, targets, sample=None):
    """({q: C - A B^T}, {q: |C| + |A| |B^T|}) for the target panels q, from the packed buffer BEFORE the call and in its dtype (float64:
    BLAS; int64 and longdouble: the exact / extended reference -- numpy has no fast product for those, hence `sample`: only the rows
    sample_rows() names).  A = rows [q NB, n_pad) of the source panels' columns, B = rows [q NB, (q+1) NB) of them."""
    NB = g.NB
    out, mag = {}, {}
    for q in range(*targets):
        A = np.hstack([panel_view(packed, g, p)[(q - p) * NB:, :] for p in range(*sources)])
        B = A[:NB, :]
        rows = sample_rows(A.shape[0], sample)
        A, C = A[rows], panel_view(packed, g, q)[rows]
        out[q] = C - A @ B.T
        mag[q] = np.abs(C) + np.abs(A) @ np.abs(B).T
    return out, mag


def lower_mask(g, q):
    """entries of panel q on or below the matrix diagonal"""
    ld = g.n_pad - q * g.NB
    return np.arange(ld)[:, None] >= np.arange(g.NB)[None, :]
