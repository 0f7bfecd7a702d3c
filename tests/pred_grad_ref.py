"""Reference of gprc_gpr_predict_grad for the tests (tests/test_pred_grad_cpu.py, tests/test_gpu_predict_grad.py): posterior mean,
pointwise variance and their gradients with respect to the test points, written from the formulas and nothing else.  No GPU, no torch.

    K_y = K + noise I = L L^T,  alpha = K_y^-1 y,  k*_j = k(x*, x_j),  v = L^-1 k*,  w = L^-T v
    mu = k* . alpha                      d mu / d x*_c      =      sum_j alpha_j dk(x*, x_j) / d x*_c
    sigma^2 = k(x*, x*) - v . v          d sigma^2 / d x*_c = -2 sum_j w_j     dk(x*, x_j) / d x*_c
    dk / d x*_c = -h_j (x*_c - x_jc) t_c:  k, h and t of every kernel are tests/kernel_ref.py's `pairwise` (the formula table is there)

predict_grad(..., dtype): everything in `dtype` -- numpy.float64 (Cholesky and triangular solves of LAPACK) or numpy.longdouble (the
column Cholesky and substitutions below).  X: d x n, X_star: d x m, one point per column, as the library takes them.
"""
import numpy as np

from kernel_ref import pairwise

LD = np.longdouble


def chol(A):
    """lower Cholesky factor in A's dtype (longdouble: column by column; float64: LAPACK)"""
    if A.dtype == np.float64:
        return np.linalg.cholesky(A)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        assert v[0] > 0
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return L


def solve_lower(L, B, transpose=False):
    """L^-1 B (or L^-T B), B a matrix of columns, in L's dtype"""
    if L.dtype == np.float64:
        import scipy.linalg as sl
        return sl.solve_triangular(L, B, lower=True, trans=1 if transpose else 0)
    n = L.shape[0]
    X = np.array(B, dtype=L.dtype, copy=True)
    if not transpose:
        for i in range(n):
            X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    else:
        for i in range(n - 1, -1, -1):
            X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def fit(name, par, X, y, noise, dtype=np.float64):
    """(L, alpha) of K + noise I in dtype"""
    X = np.asarray(X, dtype=dtype)
    K = pairwise(name, par, X, X, dtype)[0] + dtype(noise) * np.eye(X.shape[1], dtype=dtype)
    L = chol(K)
    yv = np.asarray(y, dtype=dtype).reshape(-1, 1)
    alpha = solve_lower(L, solve_lower(L, yv), transpose=True)[:, 0]
    return L, alpha


def mean_var(name, par, X, L, alpha, Xs, dtype=np.float64):
    """(mean, var) at the test points alone (what the central differences difference)"""
    ks = pairwise(name, par, Xs, X, dtype)[0]        # m x n
    v = solve_lower(L, ks.T)                               # n x m
    kss = np.ones(ks.shape[0], dtype=dtype)                # k(x*, x*) = 1 for the eight stationary kernels
    return ks @ alpha, kss - (v * v).sum(0)


def predict_cov(name, par, X, L, alpha, Xs, dtype=np.float64):
    """(mean, full posterior covariance) at the test points"""
    ks = pairwise(name, par, Xs, X, dtype)[0]
    v = solve_lower(L, ks.T)
    return ks @ alpha, pairwise(name, par, Xs, Xs, dtype)[0] - v.T @ v


def predict_grad(name, par, X, y, noise, Xs, dtype=np.float64, factor=None):
    """(mean[m], var[m], dmean[d, m], dvar[d, m]) in dtype; factor: (L, alpha) of fit() to reuse"""
    X, Xs = np.asarray(X, dtype=dtype), np.asarray(Xs, dtype=dtype)
    L, alpha = factor if factor is not None else fit(name, par, X, y, noise, dtype)
    ks, h, t = pairwise(name, par, Xs, X, dtype)      # m x n
    v = solve_lower(L, ks.T)                               # n x m
    w = solve_lower(L, v, transpose=True)                  # n x m: K_y^-1 k*
    mean = ks @ alpha
    var = np.ones(ks.shape[0], dtype=dtype) - (v * v).sum(0)
    diff = Xs[:, :, None] - X[:, None, :]                  # d x m x n
    dk = -h[None, :, :] * diff * t[:, None, None]          # dk(x*_i, x_j) / d x*_ic
    dmean = (dk * alpha[None, None, :]).sum(2)
    dvar = -dtype(2) * (dk * w.T[None, :, :]).sum(2)
    return mean, var, dmean, dvar


def make_case(case, n, m=40, seed=0, at_training_point=5):
    """(X d x n, y, Xs d x m): uniform on [-2, 2]; test point 0 equals training point `at_training_point` (None: none does)"""
    name, par, d = case
    rng = np.random.default_rng(seed + 1000 * d + n)
    X = rng.uniform(-2, 2, (d, n))
    y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
    Xs = rng.uniform(-2, 2, (d, m))
    if at_training_point is not None:
        Xs[:, 0] = X[:, at_training_point]
    return np.asfortranarray(X), y, np.asfortranarray(Xs)


def nerr(got, ref):
    """normwise max |got - ref| / max |ref| (conftest.nerr's definition), any dtype"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(float(np.abs(ref).max()), 1e-300))


# ---- the reversed factor (gprc_dev_reverse_factor) on the host -------------------------------------------------------------------
def reverse_packed(packed, winv, n_pad):
    """(packed_rev, winv_rev) as the device builds them, from the raw buffers: M = J tril(L) ^T J packed in L's layout (zero above the
    diagonal, whatever `packed` holds there), block b of winv_rev = J winv_block(B - 1 - b)^T J (all of the block).  Copies only: exact."""
    import packed_ref as R
    g = R.geometry(n_pad)
    assert g.n_pad == n_pad
    M = R.unpack_lower(packed, n_pad)[::-1, ::-1].T
    packed_rev = np.zeros_like(packed)
    for p in range(g.P):
        R.panel_view(packed_rev, g, p)[:, :] = M[p * g.NB:, p * g.NB:(p + 1) * g.NB]
    B = n_pad // 128
    winv_rev = np.empty_like(winv)
    for b in range(B):
        winv_rev[b * 16384:(b + 1) * 16384] = R.winv_block(winv, B - 1 - b)[::-1, ::-1].ravel()   # (J W^T J)^T row by row = the block column by column
    return packed_rev, winv_rev
