"""LocalGPR: nearest-neighbour Gaussian-process regression (gprc_dev_knn and gprc_lgpr_* of include/gprc_native.h; DESIGN.md section 7,
"Local GPR"; no reference counterpart).  Every test point is predicted from the exact GP of its own m <= 128 nearest training points
(local kriging, the prediction half of a nearest-neighbour GP): an exact neighbour search on the device, then one batched small model
per test point.  The cost depends on n only through the search; nothing of size n x n is formed.

    N(x*) = the m training points with the smallest (dist2, index),  dist2 = sum_c ((x*_c - x_c) s_c)^2
    mean(x*) = k_N*^T (K_NN + noise I)^-1 y_N,      var(x*) = k(x*, x*) - k_N*^T (K_NN + noise I)^-1 k_N*

s_c = 1 / l_c for the ARD kernels (the neighbours are the points of largest prior correlation), 1 for the others.  Kernels: those with
a batched small-model path -- sqrexp, sqrexp_ard, gammaexp, rationalquadratic and the four Matern kernels.

The parameters are learnt on the local model itself, through Vecchia's approximation of the likelihood (the likelihood of a
nearest-neighbour GP; DESIGN.md section 7, "Vecchia likelihood"): with the order of conditioning the column order of X,

    log p_V(y) = sum_i log p(y_i | y_N(i)),    N(i) = the min(m, i) points j < i with the smallest (dist2, j)

LocalGPR.vecchia_prepare searches the conditioning sets once (gprc_dev_knn_before) and freezes them, LocalGPR.vecchia_logp_grad is the
sum and its exact gradient in one native call (gprc_lgpr_vecchia_logp_grad), fit.optimize_local the optimiser over it.  The order
matters: vecchia_order gives a random permutation to apply to (X, y) first.
LocalGPC is the classifier on the same search (gprc_lgpc_*; DESIGN.md section 7, "Batched and local GPC"): every test point gets the
Laplace GP classifier of its own m nearest training points, fitted in batches on the device.
Out of scope here: max-min ordering, grouped conditioning sets, Vecchia prediction, gradients at x*.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as nat
from .covfunc import as_points, as_test_points, require_tagged

__all__ = ["LocalGPR", "LocalGPC", "knn", "knn_before", "vecchia_order", "MAX_NEIGHBOURS", "MAX_CONDITIONING", "BATCHED_KERNELS"]

MAX_NEIGHBOURS = 128   # a local model is one batched small model (include/gprc_native.h GPRC_BATCH_MAX_N)
MAX_CONDITIONING = 127   # a conditional is the model of the conditioning set and the point itself
BATCHED_KERNELS = (nat.SQREXP, nat.GAMMAEXP, nat.RATQUAD, nat.SQREXP_ARD, nat.MATERN32, nat.MATERN52, nat.MATERN32_ARD, nat.MATERN52_ARD)


def _check_m(m, who):
    if int(m) != m or not 1 <= int(m) <= MAX_NEIGHBOURS:
        raise ValueError(f"{who}: m must be an integer in 1 .. {MAX_NEIGHBOURS}")
    return int(m)


def knn(X, X_star, m, scale=None, ctx=None):
    """(idx[n*, m], dist2[n*, m]): for every column of X_star (d x n*) the m nearest columns of X (d x n) by
    dist2 = sum_c ((x*_c - x_c) scale_c)^2, ascending, the lower index first among equal distances (gprc_dev_knn; exact, float64).
    scale: d positive values or None; 1 <= m <= min(n, 128)."""
    m = _check_m(m, "knn")
    Xm, Xs = np.asfortranarray(as_points(X, what="X")), as_points(X_star, what="X_star")
    d, n = Xm.shape
    if Xs.shape[0] != d:
        raise ValueError("knn: X_star must have nrow(X) rows")
    if m > n:
        raise ValueError("knn: m <= ncol(X) is not TRUE")
    sc = _checked_scale(scale, d, "knn")
    Xs = np.asfortranarray(Xs)
    ns = Xs.shape[1]
    idx, dist = np.empty((ns, m), dtype=np.intc), np.empty((ns, m))
    ctx = ctx or nat.default_context()
    nat.check(nat.lib().gprc_dev_knn(ctx.handle, Xm.ctypes.data, d, n, Xs.ctypes.data, ns, None if sc is None else sc.ctypes.data, m,
                                     idx.ctypes.data, dist.ctypes.data, m))
    return idx, dist


def _checked_scale(scale, d, who):
    if scale is None:
        return None
    sc = np.ascontiguousarray(np.asarray(scale, dtype=np.float64).ravel())
    if sc.size != d or not (np.all(np.isfinite(sc)) and np.all(sc > 0)):
        raise ValueError(who + ": scale must be nrow(X) finite values > 0")
    return sc


def knn_before(X, m, scale=None, first=0, count=None, ctx=None):
    """(idx[count, m], dist2[count, m]): for every column i in [first, first + count) of X (d x n) the m nearest columns j < i by knn's
    key, ascending (gprc_dev_knn_before): the conditioning sets of the Vecchia likelihood.  Ranks that no predecessor fills (i < m) are
    -1 and +inf.  1 <= m <= 128; count=None: up to the last column."""
    m = _check_m(m, "knn_before")
    Xm = np.asfortranarray(as_points(X, what="X"))
    d, n = Xm.shape
    first = int(first)
    count = n - first if count is None else int(count)
    if first < 0 or count < 0 or first + count > n:
        raise ValueError("knn_before: the window [first, first + count) must lie in 0 .. ncol(X)")
    sc = _checked_scale(scale, d, "knn_before")
    idx, dist = np.empty((count, m), dtype=np.intc), np.empty((count, m))
    ctx = ctx or nat.default_context()
    nat.check(nat.lib().gprc_dev_knn_before(ctx.handle, Xm.ctypes.data, d, n, first, count, None if sc is None else sc.ctypes.data, m,
                                            idx.ctypes.data, dist.ctypes.data, m))
    return idx, dist


def vecchia_order(X, kind="random", seed=0):
    """A permutation of the columns of X (d x n) to condition in: "random" (np.random.default_rng(seed).permutation) or "given" (the
    identity).  The Vecchia likelihood conditions every point on its nearest EARLIER points, so the order matters: in the order a
    regular grid or a time series is stored in, the predecessors all lie to one side; a random order gives every point neighbours
    at every scale around it.  (A max-min ordering does better still; it is out of scope here.)"""
    n = as_points(X, what="X").shape[1]
    if kind == "given":
        return np.arange(n)
    if kind == "random":
        return np.random.default_rng(seed).permutation(n)
    raise ValueError('vecchia_order: kind must be "random" or "given"')


class LocalGPR(nat.Handle):
    """LocalGPR(X, y, noise, k, m=64): X d x n (one point per column), y of length n, noise >= 0 the variance, k a cov_func() of a kernel
    with a batched small-model path, m the number of neighbours a test point is conditioned on (1 .. 128; clamped to n).  The object
    holds X and y on the device until .close() (or its collection); nothing is factorised before predict."""
    _free = "gprc_lgpr_free"

    def __init__(self, X, y, noise, k, m=64, ctx=None):
        m = _check_m(m, "LocalGPR")
        Xm = np.asfortranarray(as_points(X))
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
        if y.ndim != 1 or y.size != Xm.shape[1]:
            raise ValueError("length(y) == ncol(X) is not TRUE")
        if Xm.shape[1] < 1:
            raise ValueError("ncol(X) >= 1 is not TRUE")
        k = self._checked_kernel(k, Xm.shape[0])
        d, n = Xm.shape
        self._X, self._y, self._k, self._noise, self._m = Xm, y, k, float(noise), min(m, n)
        self._info = None
        self._vecchia_m = self._vecchia_flagged = None
        self._model = C.c_void_p()
        self._ctx = ctx or nat.default_context()
        _, pp, npar = nat.params_array(k.native_params(d))
        nat.check(nat.lib().gprc_lgpr_create(self._ctx.handle, k.gprc_kernel[0], pp, npar, Xm.ctypes.data, d, n, y.ctypes.data, self._noise, m,
                                             C.byref(self._model)))

    @staticmethod
    def _checked_kernel(k, d):
        k = require_tagged(k, "LocalGPR")
        if k.gprc_kernel[0] not in BATCHED_KERNELS:
            raise ValueError("LocalGPR: the kernel has no batched small-model path (sqrexp, gammaexp, rationalquadratic, sqrexp_ard and the "
                             "Matern kernels have)")
        k.native_params(d)   # the parameter count against d
        return k

    def _points(self, X_star):
        return np.asfortranarray(as_test_points(X_star, self._X.shape[0]))

    def predict(self, X_star, pointwise_var=True):
        """The n* x 2 array cbind(mean, variance) as GPR.predict returns it (the latent variance); pointwise_var=False: the mean alone, of
        length n*.  A test point whose local model is not positive definite is NaN and has .info > 0; the call does not raise for it."""
        handle = self.handle
        Xs = self._points(X_star)
        ns = Xs.shape[1]
        mean = np.empty(ns)
        var = np.empty(ns) if pointwise_var else None
        info = np.zeros(ns, dtype=np.intc)
        nat.check(nat.lib().gprc_lgpr_predict(handle, Xs.ctypes.data, ns, mean.ctypes.data, var.ctypes.data if pointwise_var else None,
                                              info.ctypes.data))
        self._info = info
        return np.column_stack([mean, var]) if pointwise_var else mean

    def neighbours(self, X_star):
        """(idx[n*, m], dist2[n*, m]) of the test points in the model's metric, the order the local models take their points in"""
        handle = self.handle
        Xs = self._points(X_star)
        ns, m = Xs.shape[1], self._m
        idx, dist = np.empty((ns, m), dtype=np.intc), np.empty((ns, m))
        nat.check(nat.lib().gprc_lgpr_neighbours(handle, Xs.ctypes.data, ns, idx.ctypes.data, dist.ctypes.data, m))
        return idx, dist

    def set_params(self, k, noise):
        """another kernel object of the same kernel family and size, another noise; X and y stay on the device"""
        k = self._checked_kernel(k, self._X.shape[0])
        if k.gprc_kernel[0] != self._k.gprc_kernel[0]:
            raise ValueError("LocalGPR.set_params: the kernel cannot change, only its parameters")
        _, pp, npar = nat.params_array(k.native_params(self._X.shape[0]))
        nat.check(nat.lib().gprc_lgpr_set_params(self.handle, pp, npar, float(noise)))
        self._k, self._noise = k, float(noise)

    def vecchia_prepare(self, m=None):
        """Search and keep the conditioning sets of the Vecchia likelihood: for every point its min(m, i) nearest EARLIER points in the
        model's current metric (1 / l_c of the ARD kernels, Euclidean otherwise), n x m indices on the device.  m: 1 .. 127, default
        min(self.m, 127), clamped to n - 1.  The sets stay as they are -- through set_params too -- until the next vecchia_prepare, so
        vecchia_logp_grad is a smooth function of the parameters.  Returns the m in use."""
        m = min(self._m, MAX_CONDITIONING) if m is None else m
        if int(m) != m or not 1 <= int(m) <= MAX_CONDITIONING:
            raise ValueError(f"LocalGPR.vecchia_prepare: m must be an integer in 1 .. {MAX_CONDITIONING}")
        nat.check(nat.lib().gprc_lgpr_vecchia_prepare(self.handle, int(m)))
        self._vecchia_m = min(int(m), self._X.shape[1] - 1)
        return self._vecchia_m

    def vecchia_logp_grad(self, theta=None, noise=None, grad=True, cond=False):
        """(logp_V, grad[, cond]) at the parameter vector theta (the ABI's order; default: the model's own) and the noise (default: the
        model's own): the Vecchia log likelihood over the prepared conditioning sets and its exact gradient, len(theta) + 1 entries,
        d / d noise last (None when not grad: the value has the same bits); cond=True appends the n conditionals log p(y_i | y_N(i)).
        The model's own parameters are not changed.  A point whose model is not positive definite makes logp_V and grad NaN and its
        conditional NaN; .vecchia_flagged counts them; the call does not raise for it."""
        handle = self.handle
        if self._vecchia_m is None:
            raise ValueError("LocalGPR.vecchia_logp_grad: call vecchia_prepare first")
        d, n = self._X.shape
        p, pp, npar = nat.params_array(self._k.native_params(d) if theta is None else np.atleast_1d(np.asarray(theta, dtype=np.float64)))
        g = np.empty(npar + 1) if grad else None
        c = np.empty(n) if cond else None
        out, flagged = C.c_double(), C.c_int64()
        nat.check(nat.lib().gprc_lgpr_vecchia_logp_grad(handle, pp, npar, float(self._noise if noise is None else noise), C.byref(out),
                                                        g.ctypes.data if grad else None, c.ctypes.data if cond else None, C.byref(flagged)))
        self._vecchia_flagged = int(flagged.value)
        return (out.value, g, c) if cond else (out.value, g)

    @property
    def vecchia_neighbours(self):
        """idx[n, m] of the last vecchia_prepare: row i the conditioning set of point i, nearest first, -1 at the ranks >= i"""
        handle = self.handle
        if self._vecchia_m is None:
            raise ValueError("LocalGPR.vecchia_neighbours: call vecchia_prepare first")
        n, m = self._X.shape[1], self._vecchia_m
        idx = np.empty((n, m), dtype=np.intc)
        if m > 0:
            nat.check(nat.lib().gprc_lgpr_vecchia_neighbours(handle, idx.ctypes.data, m))
        return idx

    vecchia_flagged = property(lambda self: self._vecchia_flagged,
                               doc="points of the last vecchia_logp_grad whose model was not positive definite (None before the first)")
    X = property(lambda self: self._X)
    y = property(lambda self: self._y)
    k = property(lambda self: self._k)
    noise = property(lambda self: self._noise)
    m = property(lambda self: self._m, doc="neighbours per test point, min(m, n)")
    info = property(lambda self: self._info, doc="per test point of the last predict: 0, or the minor of its local model that is not positive definite")


class LocalGPC(nat.Handle):
    """LocalGPC(X, y, k, m=64, epsilon=1e-10, max_iter=0): X d x n, y in {-1, +1} of length n, k a cov_func() of a kernel with a batched
    small-model path, m the neighbours a test point's classifier is fitted on (1 .. 128; clamped to n); epsilon and max_iter: the mode
    search's stop threshold and cap (0 selects 100, at most 1000).  The object holds X and y on the device until .close(); nothing is
    fitted before a predict."""
    _free = "gprc_lgpr_free"

    def __init__(self, X, y, k, m=64, epsilon=1e-10, max_iter=0, ctx=None):
        m = _check_m(m, "LocalGPC")
        Xm = np.asfortranarray(as_points(X))
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
        if y.ndim != 1 or y.size != Xm.shape[1]:
            raise ValueError("length(y) == ncol(X) is not TRUE")
        if Xm.shape[1] < 1:
            raise ValueError("ncol(X) >= 1 is not TRUE")
        if not np.all(np.abs(y) == 1.0):
            raise ValueError("LocalGPC: the labels must be -1 or +1")
        k = self._checked_kernel(k, Xm.shape[0])
        d, n = Xm.shape
        self._X, self._y, self._k, self._m = Xm, y, k, min(m, n)
        self._info = self._iters = None
        self._model = C.c_void_p()
        self._ctx = ctx or nat.default_context()
        _, pp, npar = nat.params_array(k.native_params(d))
        nat.check(nat.lib().gprc_lgpc_create(self._ctx.handle, k.gprc_kernel[0], pp, npar, Xm.ctypes.data, d, n, y.ctypes.data, m, float(epsilon),
                                             int(max_iter), C.byref(self._model)))

    @staticmethod
    def _checked_kernel(k, d):
        k = require_tagged(k, "LocalGPC")
        if k.gprc_kernel[0] not in BATCHED_KERNELS:
            raise ValueError("LocalGPC: the kernel has no batched small-model path (sqrexp, gammaexp, rationalquadratic, sqrexp_ard and the "
                             "Matern kernels have)")
        k.native_params(d)
        return k

    def _points(self, X_star):
        return np.asfortranarray(as_test_points(X_star, self._X.shape[0]))

    def _predict(self, X_star, latent, prob):
        handle = self.handle
        Xs = self._points(X_star)
        ns = Xs.shape[1]
        fs, vf = (np.empty(ns), np.empty(ns)) if latent else (None, None)
        pr = np.empty(ns) if prob else None
        iters, info = np.zeros(ns, dtype=np.intc), np.zeros(ns, dtype=np.intc)
        nat.check(nat.lib().gprc_lgpc_predict(handle, Xs.ctypes.data, ns, nat.ptr(fs), nat.ptr(vf), nat.ptr(pr), iters.ctypes.data, info.ctypes.data))
        self._iters, self._info = iters, info
        return fs, vf, pr

    def predict_latent(self, X_star):
        """(fs_bar[n*], Vfs[n*]): the latent mean and variance of every test point's own classifier; NaN where .info != 0"""
        return self._predict(X_star, True, False)[:2]

    def predict_class(self, X_star):
        """P(y* = +1) of every test point, `GPC.predict_class`'s integral on its own classifier; NaN where .info != 0"""
        return self._predict(X_star, False, True)[2]

    def neighbours(self, X_star):
        """(idx[n*, m], dist2[n*, m]) of the test points in the model's metric, the order the local models take their points in"""
        handle = self.handle
        Xs = self._points(X_star)
        ns, m = Xs.shape[1], self._m
        idx, dist = np.empty((ns, m), dtype=np.intc), np.empty((ns, m))
        nat.check(nat.lib().gprc_lgpr_neighbours(handle, Xs.ctypes.data, ns, idx.ctypes.data, dist.ctypes.data, m))
        return idx, dist

    def set_params(self, k):
        """another kernel object of the same kernel family and size; X and y stay on the device"""
        k = self._checked_kernel(k, self._X.shape[0])
        if k.gprc_kernel[0] != self._k.gprc_kernel[0]:
            raise ValueError("LocalGPC.set_params: the kernel cannot change, only its parameters")
        _, pp, npar = nat.params_array(k.native_params(self._X.shape[0]))
        nat.check(nat.lib().gprc_lgpc_set_params(self.handle, pp, npar))
        self._k = k

    X = property(lambda self: self._X)
    y = property(lambda self: self._y)
    k = property(lambda self: self._k)
    m = property(lambda self: self._m, doc="neighbours per test point, min(m, n)")
    info = property(lambda self: self._info, doc="per test point of the last predict: gprc_gpc_batch_fit's info of its local classifier")
    iters = property(lambda self: self._iters, doc="per test point of the last predict: the Newton iterations of its local classifier")
