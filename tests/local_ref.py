"""What tests/test_local_cpu.py, tests/test_gpu_knn.py and tests/test_gpu_local.py share: the numpy references of the nearest-neighbour
search and of the local GPR, the data sets of the GPU tests (so that the references and the validity of the inputs are judged here, on
the very inputs the device sees), and the raw C-ABI calls.  A plain module: importing it needs no GPU.

    dist2(j, i) = sum_c ((xs_jc - x_ic) s_c)^2, c ascending;   neighbours of j: the m smallest keys (dist2, i), ascending
    local prediction of x*_j: the float64 closed form (batch_predict_ref.closed_form) on its reference neighbours, in reference order
"""
import ctypes as C

import numpy as np

import batch_predict_ref as P
from case_checks import logp_case
from gprc_amd import _native as nat
from gprc_amd.fit import grad_dict

N_MASTER, NS_MASTER = 4099, 300
KNN_DIMS = (1, 3, 8)
KNN_MS = (1, 2, 63, 64, 65, 127, 128)
KNN_NS = (1, 63, 64, 65, 300)
PREDICT_CASES = ("sqrexp", "gammaexp1.5", "ratquad", "ard3", "matern52_ard8")
PREDICT_MS = (1, 17, 64, 128)
PREDICT_N, PREDICT_NS, PREDICT_NOISE = 1000, 37, 0.1
ORDER_MS = (16, 32, 64)


# ---- references -----------------------------------------------------------------------------------------------------------------------
def dist2_matrix(X, Xs, scale=None):
    """ns x n: the formula above, the difference first, then the scale, the terms added with c ascending"""
    X, Xs = np.asarray(X, dtype=np.float64), np.asarray(Xs, dtype=np.float64)
    out = np.zeros((Xs.shape[1], X.shape[1]))
    for c in range(X.shape[0]):
        t = Xs[c][:, None] - X[c][None, :]
        if scale is not None:
            t = t * float(scale[c])
        out += t * t
    return out


def knn_order(X, Xs, scale=None):
    """(order[ns, n], dist2[ns, n]): per test point every training index by ascending key (dist2, index)"""
    D = dist2_matrix(X, Xs, scale)
    index = np.broadcast_to(np.arange(D.shape[1]), D.shape)
    order = np.lexsort((index, D), axis=1)
    return order, np.take_along_axis(D, order, axis=1)


def knn_ref(X, Xs, m, scale=None):
    """(idx[ns, m], dist2[ns, m])"""
    order, dist = knn_order(X, Xs, scale)
    return order[:, :m], dist[:, :m]


def smallest_gaps(sorted_dist, m):
    """per test point the smallest relative gap (b - a) / b between consecutive sorted distances a <= b among ranks 0 .. m (the first
    m + 1 distances, or all of them when there are no more); a pair with b = 0 counts as a gap of 0, a single distance as 1"""
    S = np.asarray(sorted_dist)[:, :m + 1]
    if S.shape[1] < 2:
        return np.ones(S.shape[0])
    a, b = S[:, :-1], S[:, 1:]
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(b > 0, (b - a) / b, 0.0)
    return g.min(axis=1)


def metric_of(name, theta):
    """the search metric of a model: 1 / l_c for the ARD kernels, None (Euclidean) for the others"""
    return 1.0 / np.asarray(theta, dtype=np.float64) if grad_dict[name].kernel_id in nat.ARD_KERNELS else None


def local_predict_ref(name, theta, X, y, noise, Xs, m):
    """(mean[ns], var[ns], idx[ns, m]): per test point the float64 closed form on its reference neighbours, in reference order"""
    X, y, Xs = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(Xs, dtype=np.float64)
    idx, _ = knn_ref(X, Xs, min(m, X.shape[1]), metric_of(name, theta))
    mean, var = np.empty(Xs.shape[1]), np.empty(Xs.shape[1])
    for j, nb in enumerate(idx):
        mj, vj = P.closed_form(name, theta, X[:, nb], y[nb], noise, Xs[:, j:j + 1])
        mean[j], var[j] = mj[0], vj[0]
    return mean, var, idx


def exact_ref(name, theta, X, y, noise, Xs):
    """(mean, var) of the exact GP on all of X: the float64 closed form"""
    return P.closed_form(name, theta, X, y, noise, Xs)


# ---- the data sets of the GPU tests -----------------------------------------------------------------------------------------------------
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def knn_scale(d):
    return np.linspace(0.5, 2.0, d) if d > 1 else np.array([1.7])


def knn_data(d, n):
    """(X d x n, Xs d x 300): uniform in [-1, 1]^d, X the first n columns of one master set per d; the first min(5, n) test points are
    the first training points themselves"""
    def make():
        rng = np.random.default_rng(31_000 + d)
        return rng.uniform(-1, 1, (d, N_MASTER)), rng.uniform(-1, 1, (d, NS_MASTER))
    Xm, Xsm = _cached(("master", d), make)
    X, Xs = np.asfortranarray(Xm[:, :n]), Xsm.copy(order="F")
    k = min(5, n)
    Xs[:, :k] = X[:, :k]
    return X, Xs


def knn_sizes(m):
    return (m, m + 1, 1000, N_MASTER)


def knn_reference(d, n, scaled):
    """knn_order of knn_data(d, n), computed once"""
    def make():
        X, Xs = knn_data(d, n)
        return knn_order(X, Xs, knn_scale(d) if scaled else None)
    return _cached(("knn", d, n, scaled), make)


def lattice_data():
    """(X 3 x 600, Xs 3 x 80, scale): integer coordinates in {0, ..., 5}, scales powers of two: every distance is exact in any order of
    evaluation and most are tied.  Training points 10, 200 and 411, and no others, are the corner (5, 5, 5), which is also test point 0."""
    rng = np.random.default_rng(77)
    X = rng.integers(0, 6, (3, 600)).astype(np.float64)
    X[0, (X == 5.0).all(0)] = 4.0          # the corner (5, 5, 5) belongs to the three points below alone
    X[:, [10, 200, 411]] = 5.0
    Xs = rng.integers(0, 6, (3, 80)).astype(np.float64)
    Xs[:, 0] = X[:, 10]
    return np.asfortranarray(X), np.asfortranarray(Xs), np.array([0.5, 2.0, 4.0])


def predict_points(X, ns=PREDICT_NS, seed=0):
    """d x ns test points: ns - 5 uniform in the data's bounding box, then the first five training points themselves"""
    d, n = X.shape
    lo, hi = X.min(1), X.max(1)
    rng = np.random.default_rng(61_000 + 100 * d + seed)
    inside = lo[:, None] + (hi - lo)[:, None] * rng.uniform(0, 1, (d, ns - 5))
    return np.asfortranarray(np.concatenate([inside, X[:, :5]], axis=1))


def predict_case(case, n=PREDICT_N):
    """(name, theta, X, y, noise, Xs) of a case of the batched grid at size n"""
    def make():
        name, theta, X, y, _ = logp_case(case, n)
        X = np.asfortranarray(X)
        return name, np.asarray(theta, dtype=np.float64), X, np.ascontiguousarray(y), PREDICT_NOISE, predict_points(X)
    return _cached(("case", case, n), make)


def predict_reference(case, m, n=PREDICT_N):
    def make():
        name, theta, X, y, noise, Xs = predict_case(case, n)
        return local_predict_ref(name, theta, X, y, noise, Xs, m)
    return _cached(("lref", case, m, n), make)


def exact_reference(case, n=PREDICT_N):
    def make():
        name, theta, X, y, noise, Xs = predict_case(case, n)
        return exact_ref(name, theta, X, y, noise, Xs)
    return _cached(("exact", case, n), make)


def flagged_data():
    """(name, theta, X 2 x 500, Xdup 2 x 502, y, ydup, Xs 2 x 22, m): Xdup = X with its points 7 and 11 appended again; the first two test
    points are those two points, the others the first 20 of 60 uniform draws in [-1, 1]^2 that have neither of them among their m neighbours.  With noise 0 the local models of the first two test points have one
    point twice, in ranks 0 and 1: the second pivot is exactly 0."""
    rng = np.random.default_rng(99)
    X = rng.uniform(-1, 1, (2, 500))
    y = np.sin(3 * X[0]) * np.cos(2 * X[1])
    Xdup, ydup = np.concatenate([X, X[:, [7, 11]]], axis=1), np.concatenate([y, y[[7, 11]]])
    m = 16
    other = rng.uniform(-1, 1, (2, 60))
    clear = ~np.isin(knn_ref(X, other, m)[0], [7, 11]).any(axis=1)       # neither duplicated point among its neighbours
    Xs = np.concatenate([X[:, [7, 11]], other[:, clear][:, :20]], axis=1)
    return "matern32", np.array([0.4]), np.asfortranarray(X), np.asfortranarray(Xdup), y, ydup, np.asfortranarray(Xs), m


# ---- the raw calls --------------------------------------------------------------------------------------------------------------------
def _addr(a):
    return a if isinstance(a, int) or a is None else nat.ptr(a)


def flat(A):
    """a d x n array as the library reads it: point-major, contiguous"""
    return np.ascontiguousarray(np.asarray(A, dtype=np.float64).ravel(order="F"))


def call_knn(X, d, n, Xs, ns, m, scale=None, ld=None, idx=None, dist=None, want_dist=True, ctx=None):
    """the raw gprc_dev_knn: (rc, idx, dist).  X, Xs: numpy arrays (point-major), torch tensors or addresses; idx, dist: the caller's
    arrays or tensors, else host arrays ns x ld that start as -7; nothing raises"""
    ld = m if ld is None else ld
    if idx is None:
        idx = np.full((max(ns, 1), max(ld, 1)), -7, dtype=np.intc)
    if dist is None and want_dist:
        dist = np.full((max(ns, 1), max(ld, 1)), -7.0)
    sc = None if scale is None else np.ascontiguousarray(np.asarray(scale, dtype=np.float64))
    ctx = ctx or nat.default_context()
    rc = nat.lib().gprc_dev_knn(ctx.handle, _addr(X), d, n, _addr(Xs), ns, _addr(sc), m, _addr(idx), _addr(dist), ld)
    return rc, idx, dist


def lgpr_create(name, theta, X, y, noise, m, ctx=None):
    """the raw gprc_lgpr_create: (rc, handle)"""
    kid = name if isinstance(name, int) else grad_dict[name].kernel_id
    _, pp, npar = nat.params_array(theta)
    X = np.asfortranarray(X)
    d, n = X.shape
    h = C.c_void_p()
    ctx = ctx or nat.default_context()
    rc = nat.lib().gprc_lgpr_create(ctx.handle, kid, pp, npar, X.ctypes.data, d, n, np.ascontiguousarray(y).ctypes.data, float(noise), m, C.byref(h))
    return rc, h


def lgpr_predict(h, Xs, var=True, info=True):
    """the raw gprc_lgpr_predict with host arrays: (rc, mean, var, info)"""
    Xs = np.asfortranarray(Xs)
    ns = Xs.shape[1]
    mean = np.full(ns, -7.0)
    v = np.full(ns, -7.0) if var else None
    inf = np.full(ns, -7, dtype=np.intc) if info else None
    rc = nat.lib().gprc_lgpr_predict(h, Xs.ctypes.data, ns, mean.ctypes.data, _addr(v), _addr(inf))
    return rc, mean, v, inf


def lgpr_free(h):
    nat.lib().gprc_lgpr_free(h)
