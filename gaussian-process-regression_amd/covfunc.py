"""Covariance-function layer: the reference's operator API (R/GPRclass.R:353-357, 378-403, 424-427).

`cov_func(func, ...)` fixes the parameters of one of the six kernel generics (or of `sqrexp_ard`, the squared
exponential with one length scale per input dimension, or of the Matern kernels `matern32`, `matern52`, `matern32_ard`,
`matern52_ard`, none of which the reference has) and returns a callable
`k(x, y)` obeying the reference's closure contract (two d x m matrices -> the m kernel values of their
columns).  The returned closure carries `gprc_kernel = (id, params)`, which is what routes
`covariance_matrix`, `GPR` and `GPC` to the fused HIP fill kernel.  Arbitrary user closures are part of
the reference API but not of this hot path: they stay on the reference's R implementation, and are
rejected here loudly rather than evaluated on the CPU.
"""
from __future__ import annotations

import numpy as np

from . import _native as nat

__all__ = ["cov_func", "covariance_matrix", "constant", "linear", "polynomial", "sqrexp", "gammaexp",
           "rationalquadratic", "sqrexp_ard", "matern32", "matern52", "matern32_ard", "matern52_ard", "CovFunc", "KernelGeneric", "as_points", "as_test_points"]


def as_points(X, d=None, what="X"):
    """Numeric d x m matrix in the reference's layout.  A bare vector becomes 1 x n (R/GPRclass.R:132)
    or, when `d` is given, d x (len/d) filled column by column (R/GPRclass.R:157-159)."""
    X = np.asarray(X)
    if X.dtype.kind not in "fiub":
        raise TypeError(f"is.numeric({what}) is not TRUE")
    X = X.astype(np.float64, copy=False)
    if X.ndim == 0:
        X = X.reshape(1)
    if X.ndim == 1:
        if d is None:
            X = X.reshape(1, -1)
        else:
            if X.size % d:
                raise ValueError(f"length({what}) %% nrow(X) == 0 is not TRUE")
            X = X.reshape(d, -1, order="F")
    elif X.ndim != 2:
        raise ValueError(f"{what} must be a vector or a d x n matrix")
    return np.asfortranarray(X)


def as_d_points(P, d, what):
    """`as_points` for points that must have d rows (test points, inducing points): a matrix with d rows, or a vector filled
    column by column into d rows (R/GPRclass.R:157-159)."""
    P = as_points(P, d=d, what=what) if np.ndim(P) <= 1 else as_points(P, what=what)
    if P.shape[0] != d:
        raise ValueError(f"{what} must have nrow(X) rows")
    return P


def as_test_points(X_star, d, what="X_star"):
    """The d x n* test points of a model on d-dimensional inputs, checked as GPR$predict checks them (R/GPRclass.R:156-159).  Every
    model's predict goes through here (GPR.add_data too, with what="X_new"); the caller applies whatever layout call it needs."""
    Xs = np.asarray(X_star)
    if Xs.dtype.kind not in "fiub" or Xs.size % d:
        raise ValueError(f"is.numeric({what}), length({what}) %% nrow(self$X) == 0 are not all TRUE")  # :156
    return as_d_points(Xs, d, what)


def pad_point_sets(pts):
    """B point sets (d x n_b each, n_b may differ) in one zero-filled strided array: (Pb[B, d * n_max], n_each[B], n_max), set b
    column-major from Pb[b, 0] on; the padding behind it is never read.  What the batched entry points take."""
    n_each = np.array([q.shape[1] for q in pts], dtype=np.int64)
    n_max = int(n_each.max())
    Pb = np.zeros((len(pts), pts[0].shape[0] * n_max))
    for b, q in enumerate(pts):
        Pb[b, :q.size] = q.ravel(order="F")
    return Pb, n_each, n_max


class KernelGeneric:
    """One of the reference's S3 kernel generics (`sqrexp(x, y, l)` ...).  Calling it evaluates the
    column-wise kernel on the GPU; its main use is as the first argument of `cov_func`."""

    def __init__(self, name, kid, arg_names):
        self.__name__ = name
        self.kernel_id = kid
        self.arg_names = tuple(arg_names)

    def bind(self, args, kwargs):
        """-> dict name->value following R's argument matching (named first, then positional)."""
        vals = dict(kwargs)
        for k in vals:
            if k not in self.arg_names:
                raise TypeError(f"unused argument ({k}) for kernel {self.__name__}")
        free = [a for a in self.arg_names if a not in vals]
        if len(args) > len(free):
            raise TypeError(f"too many arguments for kernel {self.__name__}")
        for a, v in zip(free, args):
            vals[a] = v
        missing = [a for a in self.arg_names if a not in vals]
        if missing:
            raise TypeError(f'argument "{missing[0]}" is missing, with no default')
        return vals

    def param_vector(self, vals):
        return np.concatenate([np.atleast_1d(np.asarray(vals[a], dtype=np.float64)).ravel() for a in self.arg_names])

    def __call__(self, x, y, *args, **kwargs):
        return CovFunc(self, self.bind(args, kwargs))(x, y)

    def __repr__(self):
        return f"<gprc kernel {self.__name__}({', '.join(('x', 'y') + self.arg_names)})>"


# argument order = the reference signatures R/GPRclass.R:381,385,389,393,397,401
constant = KernelGeneric("constant", nat.CONSTANT, ("c",))
linear = KernelGeneric("linear", nat.LINEAR, ("sigma",))
polynomial = KernelGeneric("polynomial", nat.POLYNOMIAL, ("sigma", "p"))
sqrexp = KernelGeneric("sqrexp", nat.SQREXP, ("l",))
gammaexp = KernelGeneric("gammaexp", nat.GAMMAEXP, ("l", "gamma"))
rationalquadratic = KernelGeneric("rationalquadratic", nat.RATQUAD, ("l", "alpha"))
# automatic relevance determination: exp(-1/2 sum_k ((x_k - y_k) / l_k)^2), l of length nrow(X) (no reference counterpart)
sqrexp_ard = KernelGeneric("sqrexp_ard", nat.SQREXP_ARD, ("l",))
# Matern: (1 + a) exp(-a), a = sqrt(3) r / l, and (1 + a + a^2 / 3) exp(-a), a = sqrt(5) r / l; ARD: r / l -> sqrt(sum_k ((x_k - y_k) / l_k)^2)
# (no reference counterpart; nu = 1/2 is gammaexp(l, gamma = 1))
matern32 = KernelGeneric("matern32", nat.MATERN32, ("l",))
matern52 = KernelGeneric("matern52", nat.MATERN52, ("l",))
matern32_ard = KernelGeneric("matern32_ard", nat.MATERN32_ARD, ("l",))
matern52_ard = KernelGeneric("matern52_ard", nat.MATERN52_ARD, ("l",))


class CovFunc:
    """The closure `function(x, y) func(x, y, ...)` (R/GPRclass.R:426), tagged for native dispatch."""

    def __init__(self, func: KernelGeneric, values: dict):
        self.func = func
        self.values = dict(values)
        self.params = func.param_vector(values)
        if func.kernel_id in nat.ARD_KERNELS and not (self.params.size >= 1 and np.all(np.isfinite(self.params)) and np.all(self.params > 0)):
            raise ValueError("all(is.finite(l)), all(l > 0) are not all TRUE")
        if func.kernel_id in (nat.MATERN32, nat.MATERN52) and not (self.params.size == 1 and np.isfinite(self.params[0]) and self.params[0] > 0):
            raise ValueError("length(l) == 1, is.finite(l), l > 0 are not all TRUE")
        self.gprc_kernel = (func.kernel_id, self.params)

    def native_params(self, d):
        """Parameter vector checked against the input dimension (linear: sigma of length 1 or d; the ARD kernels: l of length d)."""
        if self.func.kernel_id == nat.LINEAR and self.params.size not in (1, d):
            raise ValueError("length(sigma) == nrow(X) is not TRUE")
        if self.func.kernel_id in nat.ARD_KERNELS and self.params.size != d:
            raise ValueError("length(l) == nrow(X) is not TRUE")
        return self.params

    def __call__(self, x, y, ctx=None):
        x = np.asarray(x, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        scalar = x.ndim <= 1 and y.ndim <= 1  # the .numeric methods: two vectors -> one value
        if scalar:
            x = x.reshape(-1, 1)
            y = y.reshape(-1, 1)
        x, y = np.asfortranarray(x), np.asfortranarray(y)
        if x.shape != y.shape:
            raise ValueError("kernel arguments must have the same shape")
        d, m = x.shape
        out = np.empty(m)
        ctx = ctx or nat.default_context()
        _, pp, npar = nat.params_array(self.native_params(d))
        nat.check(nat.lib().gprc_kernel_colwise(ctx.handle, self.func.kernel_id, pp, npar, x.ctypes.data, y.ctypes.data, d, m,
                                                 out.ctypes.data))
        return float(out[0]) if scalar else out

    def __repr__(self):
        args = ", ".join(f"{k} = {v}" for k, v in self.values.items())
        return f"cov_func({self.func.__name__}, {args})"


def cov_func(func, *args, **kwargs):
    """cov_func(func, ...) (R/GPRclass.R:424-427): a covariance function with fixed parameters."""
    if not isinstance(func, KernelGeneric):
        raise TypeError("cov_func: `func` must be one of constant, linear, polynomial, sqrexp, gammaexp, "
                        "rationalquadratic, sqrexp_ard, matern32, matern52, matern32_ard, matern52_ard on the MI355X path (arbitrary R closures stay on the reference's R path)")
    return CovFunc(func, func.bind(args, kwargs))


def require_tagged(k, who):
    if not callable(k):
        raise TypeError("is.function(k) is not TRUE")
    if not hasattr(k, "gprc_kernel"):
        raise TypeError(f"{who}: covariance function is not a cov_func() of a gprc kernel; untagged closures are "
                        "evaluated by the reference's R code path only -- there is no CPU fallback here")
    return k


def covariance_matrix(A, B, covariance_function, ctx=None):
    """covariance_matrix(A, B, k) (R/GPRclass.R:355-357): ncol(A) x ncol(B), [i,j] = k(A[,i], B[,j])."""
    k = require_tagged(covariance_function, "covariance_matrix")
    A, B = as_points(A, what="A"), as_points(B, what="B")
    if A.shape[0] != B.shape[0]:
        raise ValueError("A and B must have the same number of rows")
    d, nA = A.shape
    nB = B.shape[1]
    out = np.empty((nA, nB), order="F")
    if nA == 0 or nB == 0:
        return out
    ctx = ctx or nat.default_context()
    _, pp, npar = nat.params_array(k.native_params(d))
    nat.check(nat.lib().gprc_kernel_matrix(ctx.handle, k.gprc_kernel[0], pp, npar, A.ctypes.data, d, nA, B.ctypes.data, nB,
                                            out.ctypes.data, nA))
    return out
