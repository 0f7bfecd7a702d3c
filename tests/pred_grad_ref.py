"""Reference of gprc_gpr_predict_grad for the tests (tests/test_pred_grad_cpu.py, tests/test_gpu_predict_grad.py): posterior mean,
pointwise variance and their gradients with respect to the test points, written from the formulas and nothing else.  No GPU, no torch.

    K_y = K + noise I = L L^T,  alpha = K_y^-1 y,  k*_j = k(x*, x_j),  v = L^-1 k*,  w = L^-T v
    mu = k* . alpha                      d mu / d x*_c      =      sum_j alpha_j dk(x*, x_j) / d x*_c
    sigma^2 = k(x*, x*) - v . v          d sigma^2 / d x*_c = -2 sum_j w_j     dk(x*, x_j) / d x*_c
    dk / d x*_c = -h_j (x*_c - x_jc) t_c,  s = |x* - x_j|^2, r = sqrt(s):
        sqrexp (l)                 h = k / l^2
        sqrexp_ard (l_1 .. l_d)    h = k, t_c = 1 / l_c^2
        gammaexp (l, gamma)        h = k gamma (r / l)^gamma / s;   h = 0 at r = 0
        rationalquadratic (l, a)   q = 1 + s / (2 a l^2),  h = k / (q l^2)

predict_grad(..., dtype): everything in `dtype` -- numpy.float64 (Cholesky and triangular solves of LAPACK) or numpy.longdouble (the
column Cholesky and substitutions below).  X: d x n, X_star: d x m, one point per column, as the library takes them.
"""
import numpy as np

LD = np.longdouble

# (kernel name, parameters in the ABI's order, d): the cases of the CPU and the GPU tests
CASES = [
    ("sqrexp", [0.7], 3),
    ("sqrexp", [1.5], 8),
    ("sqrexp_ard", [0.5, 1.5, 3.0], 3),
    ("gammaexp", [1.2, 1.5], 3),
    ("gammaexp", [1.2, 1.0], 2),
    ("rationalquadratic", [0.9, 1.7], 3),
]
SIZES = [(300, 0.1), (600, 0.01)]      # (n, noise)
KERNEL_ID = {"sqrexp": 3, "gammaexp": 4, "rationalquadratic": 5, "sqrexp_ard": 6}   # include/gprc_native.h


def case_id(case):
    name, par, d = case
    return "%s-%s-d%d" % (name, "_".join("%g" % p for p in par), d)


def kernel_and_h(name, par, A, B, dtype):
    """(k, h, t): k[i, j] = k(A[:, i], B[:, j]), h as above, t the d per-coordinate factors; everything in dtype"""
    A, B = np.asarray(A, dtype=dtype), np.asarray(B, dtype=dtype)
    par = [dtype(p) for p in par]
    d = A.shape[0]
    diff = A[:, :, None] - B[:, None, :]                  # d x m x n
    one, two = dtype(1), dtype(2)
    if name == "sqrexp_ard":
        l = np.asarray(par, dtype=dtype)
        s = ((diff / l[:, None, None]) ** 2).sum(0)
        k = np.exp(-s / two)
        return k, k, one / (l * l)
    s = (diff * diff).sum(0)
    t = np.ones(d, dtype=dtype)
    if name == "sqrexp":
        l = par[0]
        k = np.exp(-s / (two * l * l))
        return k, k / (l * l), t
    if name == "gammaexp":
        l, g = par
        r = np.sqrt(s)
        u = (r / l) ** g
        k = np.exp(-u)
        zero = s == 0
        h = np.where(zero, dtype(0), k * g * u / np.where(zero, one, s))
        return k, h, t
    if name == "rationalquadratic":
        l, al = par
        q = one + s / (two * al * l * l)
        k = q ** (-al)
        return k, k / (q * l * l), t
    raise ValueError(name)


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
    K = kernel_and_h(name, par, X, X, dtype)[0] + dtype(noise) * np.eye(X.shape[1], dtype=dtype)
    L = chol(K)
    yv = np.asarray(y, dtype=dtype).reshape(-1, 1)
    alpha = solve_lower(L, solve_lower(L, yv), transpose=True)[:, 0]
    return L, alpha


def mean_var(name, par, X, L, alpha, Xs, dtype=np.float64):
    """(mean, var) at the test points alone (what the central differences difference)"""
    ks = kernel_and_h(name, par, Xs, X, dtype)[0]        # m x n
    v = solve_lower(L, ks.T)                               # n x m
    kss = np.ones(ks.shape[0], dtype=dtype)                # k(x*, x*) = 1 for the four stationary kernels
    return ks @ alpha, kss - (v * v).sum(0)


def predict_grad(name, par, X, y, noise, Xs, dtype=np.float64, factor=None):
    """(mean[m], var[m], dmean[d, m], dvar[d, m]) in dtype; factor: (L, alpha) of fit() to reuse"""
    X, Xs = np.asarray(X, dtype=dtype), np.asarray(Xs, dtype=dtype)
    L, alpha = factor if factor is not None else fit(name, par, X, y, noise, dtype)
    ks, h, t = kernel_and_h(name, par, Xs, X, dtype)      # m x n
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
