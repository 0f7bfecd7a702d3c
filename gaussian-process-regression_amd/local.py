"""LocalGPR: nearest-neighbour Gaussian-process regression (gprc_dev_knn and gprc_lgpr_* of include/gprc_native.h; DESIGN.md section 7,
"Local GPR"; no reference counterpart).  Every test point is predicted from the exact GP of its own m <= 128 nearest training points
(local kriging, the prediction half of a nearest-neighbour GP): an exact neighbour search on the device, then one batched small model
per test point.  The cost depends on n only through the search; nothing of size n x n is formed.

    N(x*) = the m training points with the smallest (dist2, index),  dist2 = sum_c ((x*_c - x_c) s_c)^2
    mean(x*) = k_N*^T (K_NN + noise I)^-1 y_N,      var(x*) = k(x*, x*) - k_N*^T (K_NN + noise I)^-1 k_N*

s_c = 1 / l_c for the ARD kernels (the neighbours are the points of largest prior correlation), 1 for the others.  Kernels: those with
a batched small-model path -- sqrexp, sqrexp_ard, gammaexp, rationalquadratic and the four Matern kernels.
Out of scope here: learning the parameters on the local model (take them from fit.optimize* on a subsample), gradients at x*.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as nat
from .covfunc import as_points, as_test_points, require_tagged

__all__ = ["LocalGPR", "knn", "MAX_NEIGHBOURS", "BATCHED_KERNELS"]

MAX_NEIGHBOURS = 128   # a local model is one batched small model (include/gprc_native.h GPRC_BATCH_MAX_N)
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
    sc = None
    if scale is not None:
        sc = np.ascontiguousarray(np.asarray(scale, dtype=np.float64).ravel())
        if sc.size != d or not (np.all(np.isfinite(sc)) and np.all(sc > 0)):
            raise ValueError("knn: scale must be nrow(X) finite values > 0")
    Xs = np.asfortranarray(Xs)
    ns = Xs.shape[1]
    idx, dist = np.empty((ns, m), dtype=np.intc), np.empty((ns, m))
    ctx = ctx or nat.default_context()
    nat.check(nat.lib().gprc_dev_knn(ctx.handle, Xm.ctypes.data, d, n, Xs.ctypes.data, ns, None if sc is None else sc.ctypes.data, m,
                                     idx.ctypes.data, dist.ctypes.data, m))
    return idx, dist


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

    X = property(lambda self: self._X)
    y = property(lambda self: self._y)
    k = property(lambda self: self._k)
    noise = property(lambda self: self._noise)
    m = property(lambda self: self._m, doc="neighbours per test point, min(m, n)")
    info = property(lambda self: self._info, doc="per test point of the last predict: 0, or the minor of its local model that is not positive definite")
