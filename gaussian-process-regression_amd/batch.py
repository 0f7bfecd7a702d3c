"""A fitted batch of small GPs (include/gprc_native.h gprc_gpr_batch_fit / gprc_gpr_batch_predict / gprc_gpr_batch_predict_grad /
gprc_gpr_batch_loo; DESIGN.md section 7, "Batched predict" and "Batched prediction gradients and LOO"): B models of at most 128 points
each fitted in one native call and kept on the device; the posterior mean and variance of all of them at their test points in one
more, their gradients with respect to the test points likewise, and the leave-one-out predictions of all of them in one.  The input
conventions are `fit.logp_grad_batch`'s.

BatchGPC (gprc_gpc_batch_fit / gprc_gpc_batch_predict_latent / gprc_gpc_batch_predict_class; DESIGN.md section 7, "Batched and local
GPC") is the classifier's batch: B Laplace GP classifiers of at most 128 points each, the whole Newton mode search of every one of
them in one launch, and the latent prediction and the class probability of all of them in one call each.
"""
from __future__ import annotations

import ctypes as C
import importlib

import numpy as np

from . import _native as nat
from .covfunc import as_points, pad_point_sets

_fit = importlib.import_module(__package__ + ".fit")   # (the package's attribute `fit` is the function)


class _Batch(nat.Handle):
    """what the two batches share: the native object (a gprc_batch_model of either kind) and the layout of the test points"""
    _free, _closed = "gprc_batch_model_free", "the batch has been closed"

    def _test_points(self, X_star, who):
        """(shared, Xsb, ns_max, xs_stride, ns_each) of one shared d x n* set or a list of B sets, padded into one strided array"""
        B, d = self.B, self.d
        shared = not isinstance(X_star, (list, tuple))
        if shared:
            Xs = as_points(X_star, d, "X_star")
            if Xs.shape[0] != d or Xs.shape[1] < 1:
                raise ValueError(who + ": X_star must be d x n* with n* >= 1")
            return True, np.ascontiguousarray(Xs.ravel(order="F")), Xs.shape[1], 0, None
        if len(X_star) != B:
            raise ValueError(who + ": one set of test points per model")
        pts = [as_points(x, d, "X_star") for x in X_star]
        if any(q.shape[0] != d or q.shape[1] < 1 for q in pts):
            raise ValueError(who + ": every set of test points must be d x n* with n* >= 1")
        Xsb, ns_each, ns_max = pad_point_sets(pts)
        return False, Xsb, ns_max, d * ns_max, ns_each


class BatchGPR(_Batch):
    """B small GPR models, one per row of `thetas` (B x p, the order `dens` takes them; a vector is one model), fitted together.
    X, y: one data set shared by every model (d x n, n values), or lists of B data sets, which may differ in n (they are padded into
    one strided array; the padding is never read); noise: a scalar or B values; name: a kernel of `fit.grad_dict`.  At most 128
    points a model (ValueError beyond: `GPR` takes larger ones).

    .logp[B], .info[B]: the log evidence and 0, or the leading minor that is not positive definite -- such a model does not raise,
    its logp, alpha and predictions are NaN; both are bit for bit `logp_grad_batch`'s.  .alpha[B, n_max] (read from the device when
    asked for, zero behind a model's points).  The object holds 128 KiB of device memory a model until .close() (or its collection)."""
    def __init__(self, X, y, noise, name, thetas, ctx=None):
        func = _fit.grad_dict[name]
        thetas = np.ascontiguousarray(np.atleast_2d(np.asarray(thetas, dtype=np.float64)))
        B, p = thetas.shape
        if B < 1:
            raise ValueError("BatchGPR: at least one model")
        noises = np.ascontiguousarray(np.broadcast_to(np.asarray(noise, dtype=np.float64), (B,)))
        Xb, yb, d, n_max, x_stride, y_stride, n_each = _fit.batch_layout(X, y, B, "BatchGPR")
        self.name, self.thetas, self.noise = name, thetas, noises
        self.B, self.d, self.n_max = B, d, n_max
        self.n_each = np.full(B, n_max, dtype=np.int64) if n_each is None else n_each
        self.logp, self.info = np.empty(B), np.zeros(B, dtype=np.intc)
        self._ctx = ctx or nat.default_context()
        self._model = C.c_void_p()
        nat.check(nat.lib().gprc_gpr_batch_fit(self._ctx.handle, func.kernel_id, B, thetas.ctypes.data, p, p, noises.ctypes.data, Xb.ctypes.data, d,
                                               n_max, x_stride, yb.ctypes.data, y_stride, None if n_each is None else n_each.ctypes.data,
                                               C.byref(self._model), self.logp.ctypes.data, self.info.ctypes.data))

    @property
    def alpha(self):
        out = np.empty((self.B, self.n_max))
        nat.check(nat.lib().gprc_gpr_batch_get_alpha(self.handle, out.ctypes.data))
        return out

    def predict(self, X_star, var=True):
        """Posterior mean and latent variance k(x*, x*) - |L^-1 k*|^2 of every model.  X_star: a d x n* array of test points shared by
        every model -> (mean[B, n*], var[B, n*]); or a list of B arrays (d x n*_b, which may differ in n*_b) -> (list of B means,
        list of B variances).  var=False: the variance is not computed and None stands in its place."""
        B = self.B
        shared, Xsb, ns_max, xs_stride, ns_each = self._test_points(X_star, "BatchGPR.predict")
        mean = np.full((B, ns_max), np.nan)
        v = np.full((B, ns_max), np.nan) if var else None
        nat.check(nat.lib().gprc_gpr_batch_predict(self.handle, Xsb.ctypes.data, ns_max, xs_stride, None if ns_each is None else ns_each.ctypes.data,
                                                   mean.ctypes.data, None if v is None else v.ctypes.data, ns_max))
        if shared:
            return mean, v
        return [mean[b, :n] for b, n in enumerate(ns_each)], (None if v is None else [v[b, :n] for b, n in enumerate(ns_each)])

    def predict_grad(self, X_star, var=True):
        """`predict` with the gradients with respect to the test points (gprc_gpr_batch_predict_grad), one launch.  X_star shared
        (d x n*) -> (mean[B, n*], var[B, n*], dmean[B, d, n*], dvar[B, d, n*]); a list of B sets -> four lists, model b's gradients
        d x n*_b, the orientation of `GPR.predict_grad`.  var=False: None stands for var and dvar and the product with L^-T is skipped."""
        B, d = self.B, self.d
        shared, Xsb, ns_max, xs_stride, ns_each = self._test_points(X_star, "BatchGPR.predict_grad")
        mean = np.full((B, ns_max), np.nan)
        dmean = np.full((B, d * ns_max), np.nan)
        v = np.full((B, ns_max), np.nan) if var else None
        dv = np.full((B, d * ns_max), np.nan) if var else None
        nat.check(nat.lib().gprc_gpr_batch_predict_grad(self.handle, Xsb.ctypes.data, ns_max, xs_stride, None if ns_each is None else ns_each.ctypes.data,
                                                        mean.ctypes.data, None if v is None else v.ctypes.data, ns_max, dmean.ctypes.data,
                                                        None if dv is None else dv.ctypes.data, d * ns_max))

        if shared:         # the library's [b][j][c] (X_star's own layout) as B x d x n*
            return mean, v, dmean.reshape(B, ns_max, d).transpose(0, 2, 1).copy(), None if dv is None else dv.reshape(B, ns_max, d).transpose(0, 2, 1).copy()

        def cut(a, width):
            return None if a is None else [a[b, :width * n] for b, n in enumerate(ns_each)]

        def by_coordinate(rows):
            return None if rows is None else [np.ascontiguousarray(r.reshape(-1, d).T) for r in rows]

        return cut(mean, 1), cut(v, 1), by_coordinate(cut(dmean, d)), by_coordinate(cut(dv, d))

    def loo(self):
        """Leave-one-out cross-validation of every model in closed form (gprc_gpr_batch_loo), one launch: (mean, var, logdens), each
        B x n_max; var is the variance of the NOISY observation, as `GPR.loo`; entries behind a model's n_b points are NaN."""
        out = [np.full((self.B, self.n_max), np.nan) for _ in range(3)]
        nat.check(nat.lib().gprc_gpr_batch_loo(self.handle, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, self.n_max, None))
        return tuple(out)

    @property
    def loo_score(self):
        """the B LOO log predictive probabilities sum_i logdens_i (NaN for a flagged model)"""
        score = np.full(self.B, np.nan)
        nat.check(nat.lib().gprc_gpr_batch_loo(self.handle, None, None, None, self.n_max, score.ctypes.data))
        return score


class BatchGPC(_Batch):
    """B small Laplace GP classifiers, one per row of `thetas`, fitted together: X, y, name and thetas as `BatchGPR` takes them, the
    labels in {-1, +1} (ValueError otherwise); epsilon: the mode search stops when |objective - last| < epsilon; max_iter: its cap,
    0 selects 100, at most 1000.

    .logq[B] the Laplace log evidence, .iters[B] the Newton iterations, .info[B]: 0, or k > 0 (a non-positive pivot: non-finite
    input), -1 (the cap was reached), -2 (the objective was not finite) -- such a model does not raise, its logq, f_hat and
    predictions are NaN.  .f_hat[B, n_max]: the modes (read from the device when asked for, zero behind a model's points).  The object
    holds 128 KiB of device memory a model until .close() (or its collection)."""

    def __init__(self, X, y, name, thetas, epsilon=1e-10, max_iter=0, ctx=None):
        func = _fit.grad_dict[name]
        thetas = np.ascontiguousarray(np.atleast_2d(np.asarray(thetas, dtype=np.float64)))
        B, p = thetas.shape
        if B < 1:
            raise ValueError("BatchGPC: at least one model")
        Xb, yb, d, n_max, x_stride, y_stride, n_each = _fit.batch_layout(X, y, B, "BatchGPC")
        labels = [yb] if n_each is None else [yb[b, :n] for b, n in enumerate(n_each)]     # (the padding behind a model's labels is zero)
        if not all(np.all(np.abs(v) == 1.0) for v in labels):
            raise ValueError("BatchGPC: the labels must be -1 or +1")
        self.name, self.thetas, self.epsilon, self.max_iter = name, thetas, float(epsilon), int(max_iter)
        self.B, self.d, self.n_max = B, d, n_max
        self.n_each = np.full(B, n_max, dtype=np.int64) if n_each is None else n_each
        self.logq, self.iters, self.info = np.empty(B), np.zeros(B, dtype=np.intc), np.zeros(B, dtype=np.intc)
        self._ctx = ctx or nat.default_context()
        self._model = C.c_void_p()
        nat.check(nat.lib().gprc_gpc_batch_fit(self._ctx.handle, func.kernel_id, B, thetas.ctypes.data, p, p, Xb.ctypes.data, d, n_max, x_stride,
                                               yb.ctypes.data, y_stride, None if n_each is None else n_each.ctypes.data, self.epsilon, self.max_iter,
                                               C.byref(self._model), self.logq.ctypes.data, self.iters.ctypes.data, self.info.ctypes.data))

    @property
    def f_hat(self):
        out = np.empty((self.B, self.n_max))
        nat.check(nat.lib().gprc_gpc_batch_get_f_hat(self.handle, out.ctypes.data))
        return out

    def predict_latent(self, X_star, var=True):
        """The latent mean k*^T g and variance k(x*, x*) - |L^-1 (sqrt(W) o k*)|^2 of every model, as `GPC.predict_latent`.  X_star:
        shared (d x n*) -> (fs_bar[B, n*], Vfs[B, n*]); a list of B sets -> two lists.  var=False: None stands for the variance."""
        B = self.B
        shared, Xsb, ns_max, xs_stride, ns_each = self._test_points(X_star, "BatchGPC.predict_latent")
        mean = np.full((B, ns_max), np.nan)
        v = np.full((B, ns_max), np.nan) if var else None
        nat.check(nat.lib().gprc_gpc_batch_predict_latent(self.handle, Xsb.ctypes.data, ns_max, xs_stride, None if ns_each is None else ns_each.ctypes.data,
                                                          mean.ctypes.data, None if v is None else v.ctypes.data, ns_max))
        if shared:
            return mean, v
        return [mean[b, :n] for b, n in enumerate(ns_each)], (None if v is None else [v[b, :n] for b, n in enumerate(ns_each)])

    def predict_class(self, X_star):
        """P(y* = +1) of every model at its test points, `GPC.predict_class`'s integral: prob[B, n*] for shared points, a list of B
        vectors for a list of B sets."""
        B = self.B
        shared, Xsb, ns_max, xs_stride, ns_each = self._test_points(X_star, "BatchGPC.predict_class")
        prob = np.full((B, ns_max), np.nan)
        nat.check(nat.lib().gprc_gpc_batch_predict_class(self.handle, Xsb.ctypes.data, ns_max, xs_stride, None if ns_each is None else ns_each.ctypes.data,
                                                         prob.ctypes.data, ns_max))
        return prob if shared else [prob[b, :n] for b, n in enumerate(ns_each)]
