"""IterativeGPR: exact Gaussian-process regression without the n x n factor (gprc_igpr_* of include/gprc_native.h; DESIGN.md section 7,
"Iterative GPR"; no reference counterpart).  Every solve with K_y = K(X, X) + noise I is a preconditioned conjugate-gradient loop on a
matrix-free kernel product, in O(n) memory per right-hand side, so the posterior mean, pointwise variances at a modest n*, and above
all posterior sample paths and Thompson sampling are available at n where no factor fits.

    alpha = K_y^-1 y                        mean(x*) = sum_j k(x*, x_j) alpha_j
    var(x*) = 1 - k*^T K_y^-1 k*            (a full solve per 64 test points)
    preconditioner  P = L L^T + noise I,    L = precond_rank steps of the pivoted Cholesky of K

    logp ~ -1/2 y^T alpha - 1/2 (log det P + mean_s q_s) - n/2 log 2 pi        (logp_grad: stochastic Lanczos quadrature on the
    d logp / d theta ~ sum_ij (1/2 alpha alpha^T - 1/(2T) sum_s u_s w_s^T)_ij dK_ij   loop's own coefficients, Hutchinson probes z ~ N(0, P))

Kernels: the stationary ones with k(x, x) = 1 -- sqrexp, sqrexp_ard, gammaexp, rationalquadratic and the four Matern kernels.
fit.optimize_iterative maximises logp_grad's estimate over the kernel's parameters and the noise.
Out of scope here: add_data, several devices.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _native as nat
from .covfunc import as_points, as_test_points, require_tagged

__all__ = ["IterativeGPR", "SolveStats", "EvidenceEstimate"]


class SolveStats(NamedTuple):
    """what the fit's own solve K_y alpha = y reported"""
    iterations: int
    relres_recurrence: float    # |r| / |y| of the loop's recurrence residual at the stop
    relres_true: float          # |y - K_y alpha| / |y| from one more product: the figure to trust
    rank: int                   # columns of the preconditioner's L (below precond_rank when the pivoted Cholesky ran out of diagonal)


class EvidenceEstimate(NamedTuple):
    """what IterativeGPR.logp_grad returns"""
    value: float                # the estimate of the log marginal likelihood
    se: float                   # its standard error over the probes, 1/2 std(terms, ddof = 1) / sqrt(T); nan for one probe
    grad: np.ndarray            # d value / d (parameters, noise): len(parameters) + 1 entries, the order of fit.logp_grad
    terms: np.ndarray           # the T quadrature terms q_s, E q_s = log det K_y - log det P


class IterativeGPR(nat.Handle):
    """IterativeGPR(X, y, noise, k, tol=1e-8, max_iter=1000, precond_rank=128): X d x n (one point per column), y of length n, noise > 0
    the variance, k a cov_func() of a stationary gprc kernel.  A column of a solve stops at |r| <= tol |b|; a loop that reaches max_iter
    raises GprcError (ERR_MAXITER).  precond_rank = 0 runs without a preconditioner; at most 1024."""

    def __init__(self, X, y, noise, k, tol=1e-8, max_iter=1000, precond_rank=128, ctx=None):
        Xm = np.asfortranarray(as_points(X))
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
        if y.ndim != 1 or y.size != Xm.shape[1]:
            raise ValueError("length(y) == ncol(X) is not TRUE")
        k = require_tagged(k, "IterativeGPR")
        d, n = Xm.shape
        self._ctx = ctx or nat.default_context()
        self._X, self._y, self._k, self._noise = Xm, y, k, float(noise)
        self._model = C.c_void_p()
        _, pp, npar = nat.params_array(k.native_params(d))
        nat.check(nat.lib().gprc_igpr_fit(self._ctx.handle, k.gprc_kernel[0], pp, npar, Xm.ctypes.data, d, n, y.ctypes.data, self._noise,
                                          float(tol), int(max_iter), int(precond_rank), C.byref(self._model)))
        alpha = np.empty(n)
        nat.check(nat.lib().gprc_igpr_get_alpha(self._model, alpha.ctypes.data))
        it, rec, true, rank = C.c_int(), C.c_double(), C.c_double(), C.c_int64()
        nat.check(nat.lib().gprc_igpr_stats(self._model, C.byref(it), C.byref(rec), C.byref(true), C.byref(rank)))
        self._alpha, self._stats = alpha, SolveStats(it.value, rec.value, true.value, rank.value)

    def _points(self, X_star):
        return np.asfortranarray(as_test_points(X_star, self._X.shape[0]))

    def predict(self, X_star, pointwise_var=True):
        """The n* x 2 array cbind(mean, variance) as GPR.predict returns it (the latent variance); pointwise_var=False: the mean alone, of
        length n*.  The variance costs a full conjugate-gradient solve per 64 test points; the full covariance is not offered."""
        Xs = self._points(X_star)
        ns = Xs.shape[1]
        mean = np.empty(ns)
        var = np.empty(ns) if pointwise_var else None
        nat.check(nat.lib().gprc_igpr_predict(self.handle, Xs.ctypes.data, ns, mean.ctypes.data, var.ctypes.data if pointwise_var else None))
        return np.column_stack([mean, var]) if pointwise_var else mean

    def solve(self, B, with_stats=False):
        """K_y^-1 B for B of length n or n x S; with_stats: (X, iterations per column, true relative residual per column)"""
        Bm = np.asarray(B, dtype=np.float64)
        n = self._X.shape[1]
        vector = Bm.ndim == 1
        Bm = np.asfortranarray(Bm.reshape(n, -1))
        S = Bm.shape[1]
        out = np.empty((n, S), order="F")
        iters, res = (C.c_int * S)(), np.empty(S)
        nat.check(nat.lib().gprc_igpr_solve(self.handle, Bm.ctypes.data, n, S, out.ctypes.data, n, iters, res.ctypes.data_as(C.POINTER(C.c_double))))
        out = out[:, 0] if vector else out
        return (out, np.array(iters[:]), res) if with_stats else out

    def _normals(self, g1, g2):
        """(g1 rank x T or empty, g2 n x T, T) as Fortran arrays; g1 is not looked at without a preconditioner"""
        n, r = self._X.shape[1], self._stats.rank
        g2 = np.asfortranarray(np.asarray(g2, dtype=np.float64).reshape(n, -1))
        T = g2.shape[1]
        if T < 1:
            raise ValueError("ncol(g2) >= 1 is not TRUE")
        if r == 0:
            return np.zeros((0, T), order="F"), g2, T
        if g1 is None:
            raise ValueError("g1 (stats.rank x T) is needed: the model has a preconditioner")
        g1 = np.asfortranarray(np.asarray(g1, dtype=np.float64).reshape(-1, T))
        if g1.shape[0] < r:
            raise ValueError("nrow(g1) >= stats.rank is not TRUE")
        return g1, g2, T

    def probes(self, g1, g2):
        """Z = L g1 + sqrt(noise) g2 (n x T), the probe vectors logp_grad draws its estimates from: z ~ N(0, P) for standard normal g1
        (stats.rank x T) and g2 (n x T).  Without a preconditioner (rank 0) Z = g2 and g1 is ignored."""
        g1, g2, T = self._normals(g1, g2)
        n = self._X.shape[1]
        Z = np.empty((n, T), order="F")
        nat.check(nat.lib().gprc_igpr_probes(self.handle, g1.ctypes.data if g1.size else None, max(g1.shape[0], 1), g2.ctypes.data, n, T,
                                             Z.ctypes.data, n))
        return Z

    def logp_grad(self, n_probes=31, *, rng=None, g1=None, g2=None):
        """EvidenceEstimate(value, se, grad, terms): the log marginal likelihood and its gradient with respect to (parameters, noise),
        estimated from n_probes probe vectors through the conjugate-gradient loop (gprc_igpr_logp_grad).  A deterministic function of
        the standard normals g1 (stats.rank x T) and g2 (n x T); drawn from rng (g2 first, then g1) when not given."""
        n = self._X.shape[1]
        if g2 is None:
            if int(n_probes) < 1:
                raise ValueError("n_probes >= 1 is not TRUE")
            rng = rng if rng is not None else np.random.default_rng()
            g2 = rng.standard_normal((n, int(n_probes)))
            g1 = rng.standard_normal((self._stats.rank, int(n_probes)))
        g1, g2, T = self._normals(g1, g2)
        value, se = C.c_double(), C.c_double(float("nan"))
        grad, terms = np.empty(len(self._k.native_params(self._X.shape[0])) + 1), np.empty(T)
        nat.check(nat.lib().gprc_igpr_logp_grad(self.handle, g1.ctypes.data if g1.size else None, max(g1.shape[0], 1), g2.ctypes.data, n, T,
                                                C.byref(value), C.byref(se) if T >= 2 else None, grad.ctypes.data, terms.ctypes.data))
        return EvidenceEstimate(value.value, se.value, grad, terms)

    def sample_paths(self, n_paths, n_features=1024, *, rng=None, nu=None, phase=None, w=None, e=None):
        """GPR.sample_paths with its arguments and its order of draws; the update term's weights come from the conjugate-gradient solve of
        all n_paths right-hand sides.  Returns a sampling.SamplePaths, which survives close() of this model."""
        from .sampling import SamplePaths, spectral_frequencies
        d, n = self._X.shape
        S, D = int(n_paths), int(n_features)
        if S < 1 or D < 1:
            raise ValueError("n_paths >= 1, n_features >= 1 are not all TRUE")
        rng = rng if rng is not None else np.random.default_rng()
        if nu is None:
            nu = spectral_frequencies(self._k, d, D, rng)
        phase = rng.random(D) if phase is None else phase
        w = rng.standard_normal((S, D)).T if w is None else w
        e = rng.standard_normal((S, n)).T if e is None else e
        nu = np.asfortranarray(np.asarray(nu, dtype=np.float64).reshape(d, D))
        phase = np.ascontiguousarray(np.asarray(phase, dtype=np.float64).reshape(D))
        w = np.asfortranarray(np.asarray(w, dtype=np.float64).reshape(D, S))
        e = np.asfortranarray(np.asarray(e, dtype=np.float64).reshape(n, S))
        return SamplePaths(self.handle, d, nu, phase, w, e)

    def thompson_batch(self, q, lower, upper, n_features=1024, n_starts=16, rng=None, **kw):
        """GPR.thompson_batch: the d x q arg-maxima of q posterior sample paths over the box [lower, upper]"""
        rng = rng if rng is not None else np.random.default_rng()
        with self.sample_paths(q, n_features, rng=rng) as sp:
            return sp.maximize(lower, upper, n_starts=n_starts, rng=rng, **kw).x_best

    X = property(lambda self: self._X)
    y = property(lambda self: self._y)
    k = property(lambda self: self._k)
    noise = property(lambda self: self._noise)
    alpha = property(lambda self: self._alpha, doc="K_y^-1 y")
    stats = property(lambda self: self._stats, doc="SolveStats of the fit's solve")
