"""SparseGPR: Gaussian-process regression with m << n inducing points (Titsias' variational sparse GP in its collapsed form, also
called SGPR or VFE; no reference counterpart).  The bound `elbo <= log p(y)` replaces the log marginal likelihood, a prediction costs
O(m^2) per test point, the fit 2 n m^2 flop in one pass over the training points, and the device holds two m x m factors and one chunk
of rows -- never the n x n matrix, never X (gprc_sgpr_* of include/gprc_native.h; DESIGN.md section 7, "Sparse GPR").

    K_uu = k(Z,Z) + jitter I = L_u L_u^T          V = K(X,Z) L_u^-T
    B    = I + V^T V / noise = L_B L_B^T          c = L_B^-1 V^T y / noise
    trace = sum_i ( k(x_i,x_i) - |v_i|^2 )
    elbo = -n/2 log(2 pi noise) - sum_j log (L_B)_jj - y^T y / (2 noise) + c^T c / 2 - trace / (2 noise)
    predict: v* = L_u^-1 k(Z,x*),  w* = L_B^-1 v*,  mean = w*^T c,  var = k(x*,x*) - |v*|^2 + |w*|^2   (the latent variance)

The bound's exact gradient (kernel parameters, noise, Z) and the optimiser over it are fit.elbo_grad and fit.optimize_sparse
(gprc_sgpr_elbo_grad; DESIGN.md section 7, "Sparse GPR gradient").  Out of scope here: FITC, the full predictive covariance, several
devices.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as nat
from .covfunc import as_d_points, as_points, require_tagged

__all__ = ["SparseGPR", "select_inducing", "elbo"]


def select_inducing(X, m, rng=None):
    """m distinct columns of X (d x n, one point per column), drawn without replacement, in ascending column order; `rng`: a
    numpy Generator, a seed, or None."""
    Xm = as_points(X)
    n = Xm.shape[1]
    m = int(m)
    if not 1 <= m <= n:
        raise ValueError("1 <= m <= ncol(X) is not TRUE")
    rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
    idx = np.sort(rng.choice(n, size=m, replace=False))
    return np.asfortranarray(Xm[:, idx])


def _checked(X, y, noise, k, Z, jitter, who):
    Xm = np.asfortranarray(as_points(X))
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
    if y.ndim != 1 or y.size != Xm.shape[1]:
        raise ValueError("length(y) == ncol(X) is not TRUE")
    k = require_tagged(k, who)
    return Xm, y, float(noise), k, as_d_points(Z, Xm.shape[0], "Z"), float(jitter)


def elbo(X, y, noise, k, Z, jitter=1e-6, ctx=None, with_trace=False):
    """The collapsed bound of SparseGPR(X, y, noise, k, Z, jitter) without keeping a model (gprc_sgpr_elbo): the bits SparseGPR(...).elbo
    has.  with_trace: (elbo, trace).  Raises NotPositiveDefinite when K_uu + jitter I or B is not positive definite."""
    Xm, y, noise, k, Zm, jitter = _checked(X, y, noise, k, Z, jitter, "elbo")
    d, n = Xm.shape
    ctx = ctx or nat.default_context()
    _, pp, npar = nat.params_array(k.native_params(d))
    e, t = C.c_double(), C.c_double()
    nat.check(nat.lib().gprc_sgpr_elbo(ctx.handle, k.gprc_kernel[0], pp, npar, Xm.ctypes.data, d, n, y.ctypes.data, noise, Zm.ctypes.data,
                                       Zm.shape[1], jitter, C.byref(e), C.byref(t)))
    return (e.value, t.value) if with_trace else e.value


class SparseGPR(nat.Handle):
    """SparseGPR(X, y, noise, k, Z, jitter=1e-6): X d x n (one point per column), y of length n, noise > 0 the variance, k a
    cov_func() of any gprc kernel, Z d x m inducing points (select_inducing picks columns of X).  The model keeps Z, not X or y."""

    def __init__(self, X, y, noise, k, Z, jitter=1e-6, ctx=None):
        Xm, y, noise, k, Zm, jitter = _checked(X, y, noise, k, Z, jitter, "SparseGPR")
        d, n = Xm.shape
        self._ctx = ctx or nat.default_context()
        self._k, self._Z, self._noise, self._jitter, self._n = k, Zm, noise, jitter, n
        self._model = C.c_void_p()
        _, pp, npar = nat.params_array(k.native_params(d))
        nat.check(nat.lib().gprc_sgpr_fit(self._ctx.handle, k.gprc_kernel[0], pp, npar, Xm.ctypes.data, d, n, y.ctypes.data, noise,
                                          Zm.ctypes.data, Zm.shape[1], jitter, C.byref(self._model)))
        e, t = C.c_double(), C.c_double()
        nat.check(nat.lib().gprc_sgpr_get_elbo(self._model, C.byref(e), C.byref(t)))
        self._elbo, self._trace = e.value, t.value

    def predict(self, X_star):
        """(mean, var) at the columns of X_star: two arrays of length n*; var is the latent variance (add `noise` for an observation)."""
        handle = self.handle
        Xs = as_d_points(np.asarray(X_star), self._Z.shape[0], "X_star")
        ns = Xs.shape[1]
        mean, var = np.empty(ns), np.empty(ns)
        nat.check(nat.lib().gprc_sgpr_predict(handle, Xs.ctypes.data, ns, mean.ctypes.data, var.ctypes.data))
        return mean, var

    elbo = property(lambda self: self._elbo, doc="the collapsed bound, <= log p(y)")
    trace = property(lambda self: self._trace, doc="sum_i k(x_i,x_i) - |v_i|^2: what the inducing points do not explain")
    Z = property(lambda self: self._Z, doc="the inducing points, d x m")
    noise = property(lambda self: self._noise)
