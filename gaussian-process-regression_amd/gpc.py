"""GPC: host mirror of the reference's R6 class `GPC` (R/GPCclass.R:55-210).

`GPC$new(X, y, k, epsilon)` runs the Laplace/IRLS mode search on the GPU (kernel fill once, then per
iteration B = I + sqrt(W) K sqrt(W), its Cholesky, two triangular solves and two K-matvecs);
`predict_class` gets fs_bar / Vfs from the GPU (R/GPCclass.R:109-115) and evaluates the reference's
per-point 1-D integral (:116-117, stats::integrate there) as one batched device quadrature kernel
(SURVEY 8f rank 3); the reference's own QUADPACK method stays available as `integrator="quadpack"`.
Reference quirks are reproduced: logq uses sum(diag(L)) (:103), the integral passes the *variance* Vfs
as dnorm's sd (:117), and the stop rule of :90-91 (`least_objective + 10 < objective`, which fires when
the maximised objective IMPROVES by more than 10 over iteration 1) raises "Apparently does not converge."
exactly where the reference does.  `reference_stop=False` (keyword-only, not in the reference) switches
that rule off so that larger problems can be fitted.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

from . import _native as nat
from .covfunc import as_points, require_tagged
from .gpr import _ReadOnly, _is_numeric_vector

__all__ = ["GPC", "class_probability_quadpack", "DEFAULT_INTEGRATOR"]

# "native" | "quadpack": what predict_class(X_star) uses when the call does not say (see GPC.predict_class)
DEFAULT_INTEGRATOR = os.environ.get("GPRC_GPC_INTEGRATOR", "native")


def class_probability_quadpack(fs_bar, Vfs):
    """The reference's integral as the reference computes it (R/GPCclass.R:116-117):
    integrate(function(z) sigmoid(z) * dnorm(z, mean = fs_bar[i], sd = Vfs[i]), -Inf, Inf)$value with integrate()'s
    defaults: QUADPACK dqagi, rel.tol = abs.tol = .Machine$double.eps^0.25, subdivisions = 100."""
    from scipy import integrate, stats
    tol = float(np.finfo(np.float64).eps) ** 0.25
    fs, vf = np.atleast_1d(np.asarray(fs_bar, dtype=np.float64)), np.atleast_1d(np.asarray(Vfs, dtype=np.float64))
    out = np.empty(fs.size)
    with np.errstate(over="ignore"):
        for i in range(fs.size):
            mu, sd = fs[i], vf[i]
            out[i] = integrate.quad(lambda z: (1.0 / (1.0 + np.exp(-z))) * stats.norm.pdf(z, loc=mu, scale=sd),
                                    -np.inf, np.inf, epsabs=tol, epsrel=tol, limit=100)[0]
    return out


class GPC(nat.Handle):
    """GPC$new(X, y, k, epsilon = 1e-5)  --  R/GPCclass.R:66."""

    def __init__(self, X, y, k, epsilon=1e-5, *, ctx=None, max_iter=0, reference_stop=True):
        Xa = np.asarray(X)
        if Xa.dtype.kind not in "fiub" or not _is_numeric_vector(y):
            raise TypeError("is.numeric(X), is.vector(y), is.numeric(y) are not all TRUE")        # :67
        if not isinstance(epsilon, (int, float, np.floating, np.integer)) or not epsilon > 0 or not callable(k):
            raise TypeError("is.numeric(epsilon), epsilon > 0, is.function(k) are not all TRUE")  # :68
        Xm = as_points(Xa)                                                                       # :70
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
        if y.size != Xm.shape[1]:
            raise ValueError("length(y) == ncol(X) is not TRUE")                                 # :71
        k = require_tagged(k, "GPC")
        d, n = Xm.shape
        self._ctx = ctx or nat.default_context()
        self._X, self._y, self._k = Xm, y, k
        self._L = None
        self._model = C.c_void_p()
        _, pp, npar = nat.params_array(k.native_params(d))
        iters = C.c_int()
        rc = nat.lib().gprc_gpc_fit(self._ctx.handle, k.gprc_kernel[0], pp, npar, Xm.ctypes.data, d, n, y.ctypes.data,
                                    float(epsilon), int(max_iter), nat.GPC_REFERENCE_STOP if reference_stop else 0,
                                    C.byref(self._model), C.byref(iters))
        if rc == nat.ERR_DIVERGED:
            raise ArithmeticError("Apparently does not converge.")                               # :91
        nat.check(rc)
        self.iterations = iters.value
        sys.stderr.write(f"Convergence after {iters.value} iterations\n")                        # :98 message()
        f_hat = np.empty(n)
        nat.check(nat.lib().gprc_gpc_get_f_hat(self._model, f_hat.ctypes.data))
        lq = C.c_double()
        nat.check(nat.lib().gprc_gpc_get_logq(self._model, C.byref(lq)))
        self._f_hat, self._logq = f_hat, lq.value

    @classmethod
    def new(cls, *args, **kwargs):
        return cls(*args, **kwargs)

    def _points(self, X_star):
        """The reference gives a bare vector the dimensions 1 x length (:109), not GPR$predict's column-by-column fill, so a vector stands
        for test points only when nrow(X) is 1: not covfunc.as_test_points, because the reference's two classes differ here."""
        Xs = as_points(np.asarray(X_star, dtype=np.float64))                                     # :109
        if Xs.shape[0] != self._X.shape[0]:
            raise ValueError("X_star must have nrow(X) rows")
        return Xs

    def predict_latent(self, X_star):
        """fs_bar and Vfs of R/GPCclass.R:109-115 (the GPU part of predict_class)."""
        Xs = self._points(X_star)
        ns = Xs.shape[1]
        fs, vf = np.empty(ns), np.empty(ns)
        nat.check(nat.lib().gprc_gpc_predict_latent(self._model, Xs.ctypes.data, ns, fs.ctypes.data, vf.ctypes.data))
        return fs, vf

    def predict_class(self, X_star, integrator=None):
        """GPC$predict_class(X_star)  --  R/GPCclass.R:108-118: P(y* = +1 | x*) per test point.
        integrator="native" (default): the batched device quadrature (gprc_gpc_predict_class), accurate to ~1e-11;
        integrator="quadpack": the reference's own method on the host -- QUADPACK dqagi through scipy with
        stats::integrate's defaults (rel.tol = abs.tol = .Machine$double.eps^0.25, 100 subdivisions).
        Both reproduce sd = Vfs[i] (sic, :117).

        WHERE THE TWO DIFFER (pinned by tests/test_gpu_parity.py::test_class_probability_divergence_is_pinned): dqagi on
        (-Inf, Inf) never samples a narrow Gaussian peak far from the origin -- e.g. fs_bar = 8, Vfs = 0.05 -- and
        returns ~0 with a tiny error estimate, so the REFERENCE reports P ~ 0 there, where the integral is 0.9997.
        "native" returns the mathematically correct value; a caller who wants the reference's numbers in that
        regime too asks for "quadpack" (per call, or process-wide through gprc_amd.gpc.DEFAULT_INTEGRATOR /
        the environment variable GPRC_GPC_INTEGRATOR).  The R binding keeps integrate() (r/R/native.R)."""
        integrator = integrator or DEFAULT_INTEGRATOR
        if integrator == "native":
            Xs = self._points(X_star)
            ns = Xs.shape[1]
            out = np.empty(ns)
            nat.check(nat.lib().gprc_gpc_predict_class(self._model, Xs.ctypes.data, ns, out.ctypes.data))
            return out
        if integrator != "quadpack":
            raise ValueError("integrator must be 'native' or 'quadpack'")
        fs, vf = self.predict_latent(X_star)
        return class_probability_quadpack(fs, vf)

    def _get_L(self):
        if self._L is None:
            n = self._X.shape[1]
            L = np.empty((n, n), order="F")
            nat.check(nat.lib().gprc_model_get_L(self._model, L.ctypes.data, n))
            self._L = L
        return self._L

    X = _ReadOnly("X", lambda s: s._X)
    k = _ReadOnly("k", lambda s: s._k)
    y = _ReadOnly("y", lambda s: s._y)
    f_hat = _ReadOnly("f_hat", lambda s: s._f_hat)
    L = _ReadOnly("L", _get_L)
    logq = _ReadOnly("logq", lambda s: s._logq)
