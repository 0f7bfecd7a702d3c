"""fit(): hyper-parameter selection by maximising the log marginal likelihood (reference R/fit.R:110-169) --
the immediate caller of the hot path.

What runs where
  * the objective `dens(v)` (R/fit.R:117-124: K, Cholesky, alpha, log marginal likelihood) is one native call,
    gprc_gpr_log_marginal; the reference's O(n^4) `min(det(leading minors)) > 0` guard (:119) is the Cholesky's
    own positive-definiteness test;
  * the optimiser driver is host code, as in the reference.  R's `optim(method = "Brent")` is `optimize()`, Brent's
    fmin; it is restated in optim.py (golden section + successive parabolic interpolation, tol = sqrt(.Machine$double.eps))
    so that the one-parameter kernels (sqrexp, constant, linear) and the polynomial degree loop follow the same
    iterates.  `optim_until_error` (R/fit.R:47-69) is kept: a failing evaluation yields the sentinel -10000.
  * the two-parameter kernels gammaexp / rationalquadratic go through `optim(method = "BFGS")` with the gradient
    `dens_deriv` (R/fit.R:126-139).  That gradient is reproduced AS WRITTEN, by the native gprc_fit_gradient: it
    inverts the noise-free K, ignores `noise`, applies `diag(.) %*%` where a trace is meant and binds the parameter
    vector in `deriv`'s argument order, which is the reverse of the kernels' own.  R's BFGS is `vmmin` (Nash's
    variable-metric Algorithm 21); it is restated in optim.py.  Consequences that follow from the reference's code and are
    kept: gammaexp's gradient has a NaN component (0 * log 0 on the diagonal), vmmin then takes its "uphill" exit at
    once and fit() returns the start values (1, 1); a failing gradient (K not invertible) aborts optim and
    optim_until_error falls back to the best objective value seen so far.
Beside the reference-faithful fit() stands an EXACT path (no reference counterpart): `logp_grad` is the log marginal
likelihood and its true gradient in one native call (gprc_gpr_logp_grad: the noisy K_y = K + noise I, a trace, every
parameter and the noise), and `optimize` maximises it over log(theta) (and log(noise)) with the same vmmin.  It is what
makes gammaexp / rationalquadratic searches move and what the d length scales of `sqrexp_ard`, `matern32_ard` and `matern52_ard` need.
Small models come in batches: `logp_grad_batch` is `logp_grad` for B models of at most 128 points in one native call
(gprc_gpr_batch_logp_grad: one model per workgroup), and `optimize_multistart` runs one `vmmin_steps` -- vmmin as a generator -- per
start value in lockstep on it, every start exactly as `optimize` would run it.
Classification has the same pair: `logq_grad` is the Laplace log evidence of GPC and its exact gradient (gprc_gpc_logq_grad: the
mode search of GPC$new, then one contraction), `optimize_gpc` maximises it over log(theta).
The sparse GPR has it too: `elbo_grad` is Titsias' collapsed bound and its exact gradient with respect to the kernel parameters, the
noise and the inducing points (gprc_sgpr_elbo_grad: the fit's pass, a second pass and one contraction), `optimize_sparse` maximises it
over log(theta), log(noise) and the inducing points themselves.
The local GPR learns its parameters on Vecchia's approximation of the likelihood: `vecchia_logp_grad` is the sum of the n conditionals
log p(y_i | y_N(i)) and its exact gradient (gprc_lgpr_vecchia_logp_grad: one small model per workgroup), `optimize_local` maximises it
with the conditioning sets searched once per pass and frozen inside it.
What lives here, and what is shared (the next objective or optimiser uses these, it does not copy a neighbour):
  * fit(), its optim_until_error wrappers, cov_dict and SENTINEL: the reference-faithful part;
  * the objective wrappers dens, dens_deriv, logp_grad, loo_grad, logq_grad, elbo_grad: each is `_staged` (points, targets, context,
    parameter pointers) and one native call;
  * the optimisers optimize, optimize_multistart, optimize_sparse, optimize_iterative, optimize_local, optimize_gpc: each is a `_Front` (start values,
    z = [log theta, log noise, ...] and back, the gradient cut to match, the result dict) around `_maximise_over_log`; how one point
    of z is evaluated -- exp (`_from_log`), range check (`_in_range`), chain factor and one-entry cache (`_Evaluation`) -- is the same
    code for the single optimisers and for every instance of optimize_multistart, which takes the first two for all the points of a
    round at once (tests/test_optimizers_cpu.py pins their iterates);
  * vmmin, vmmin_steps and brent_fmin are optim.py's, re-exported here under their old names.
Parity status: unpinned (the reference holds no numeric expectations for fit(); tests/testthat/test-fit.R:12-17 only
checks which kernel NAME wins); cross-checked against scipy's bounded Brent on the same native objective, and the
BFGS branch against the same driver running on the CPU oracle's objective and gradient.
"""
from __future__ import annotations

import ctypes as C
import math
import sys

import numpy as np

from . import _native as nat
from .covfunc import (CovFunc, as_d_points, as_points, pad_point_sets, constant, linear, polynomial, sqrexp, gammaexp, rationalquadratic, sqrexp_ard, matern32, matern52,
                      matern32_ard, matern52_ard)
from .optim import brent_fmin, vmmin, vmmin_steps

__all__ = ["fit", "dens", "dens_deriv", "logp_grad", "logp_grad_batch", "loo_grad", "optimize", "optimize_multistart", "vmmin_steps", "logq_grad", "optimize_gpc", "elbo", "elbo_grad", "optimize_sparse",
           "vecchia_logp_grad", "optimize_local", "cov_dict", "brent_fmin", "vmmin"]

# R/fit.R:2-33: name -> (kernel generic, display name, start values)
cov_dict = {
    "sqrexp": (sqrexp, "Squared Exponential", (1.0,)),
    "gammaexp": (gammaexp, "Gamma Exponential", (1.0, 1.0)),
    "constant": (constant, "Constant", (1.0,)),
    "linear": (linear, "Linear", (1.0,)),
    "polynomial": (polynomial, "Polynomial", (1.0, 2.0)),
    "rationalquadratic": (rationalquadratic, "Rational Quadratic", (1.0, 1.0)),
}
SENTINEL = -10000.0  # R/fit.R:50


def _staged(X, y, v, ctx, check_y=None):
    """What every objective wrapper stages before its one native call: (Xm, y, d, n, ctx, (p, pp, npar)) -- the points d x n, the
    targets as float64, the context (the default one when none is given) and nat.params_array of the parameter vector v.
    check_y: None -- the length of y is the native layer's to refuse; "size" / "vector": length(y) == ncol(X) (and, for "vector",
    one dimension) is checked here, where the wrapper has always checked it."""
    Xm = as_points(X)
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
    d, n = Xm.shape
    if check_y and (y.size != n or (check_y == "vector" and y.ndim != 1)):
        raise ValueError("length(y) == ncol(X) is not TRUE")
    return Xm, y, d, n, ctx or nat.default_context(), nat.params_array(np.atleast_1d(np.asarray(v, dtype=np.float64)))


def dens(X, y, noise, name, v, ctx=None):
    """dens(v) of R/fit.R:117-124 for kernel `name` with parameter vector v (in the generic's argument order).
    Raises nat.NotPositiveDefinite when K + noise*I is not positive definite (the reference's stopifnot / chol error).
    `name` may also be a kernel of grad_dict that is not in cov_dict: "sqrexp_ard", "matern32_ard", "matern52_ard" (v = one length
    scale per row of X), "matern32", "matern52" (v = the length scale)."""
    func = _kernel_by_name(name)
    Xm, y, d, n, ctx, (_, pp, npar) = _staged(X, y, v, ctx)
    out = C.c_double()
    nat.check(nat.lib().gprc_gpr_log_marginal(ctx.handle, func.kernel_id, pp, npar, Xm.ctypes.data, d, n, y.ctypes.data,
                                              float(noise), C.byref(out)))
    return out.value


def dens_deriv(X, y, name, v, ctx=None):
    """dens_deriv(v) of R/fit.R:126-139 (quirks included, see the module docstring) for kernel `name`.
    Raises nat.NotPositiveDefinite when the noise-free K cannot be inverted (the reference's solve(K) error)."""
    func = cov_dict[name][0]
    Xm, y, d, n, ctx, (p, pp, npar) = _staged(X, y, v, ctx)
    g = np.empty(p.size)
    nat.check(nat.lib().gprc_fit_gradient(ctx.handle, func.kernel_id, pp, npar, Xm.ctypes.data, d, n, y.ctypes.data,
                                          g.ctypes.data_as(C.POINTER(C.c_double))))
    return g


# kernels of the exact gradient: name -> generic (parameter vectors in the ABI's order: {l}, {l, gamma}, {l, alpha}, {l_1..l_d})
grad_dict = {"sqrexp": sqrexp, "gammaexp": gammaexp, "rationalquadratic": rationalquadratic, "sqrexp_ard": sqrexp_ard,
             "matern32": matern32, "matern52": matern52, "matern32_ard": matern32_ard, "matern52_ard": matern52_ard}


def _kernel_by_name(name):
    """The generic of a kernel name: one of cov_dict's six or one of grad_dict's."""
    return cov_dict[name][0] if name in cov_dict else grad_dict[name]


def _is_ard(name):
    return grad_dict[name].kernel_id in nat.ARD_KERNELS


def _default_start(name, d):
    """cov_dict's start values; the kernels outside it: every length scale 1."""
    if name in cov_dict:
        return cov_dict[name][2]
    return np.ones(d if _is_ard(name) else 1)


def _func_of(name, par):
    func = grad_dict[name]
    return CovFunc(func, {"l": np.array(par)} if _is_ard(name) else func.bind(par, {}))


def _value_and_noise_grad(symbol, X, y, noise, name, v, ctx):
    """logp_grad and loo_grad: the two entry points take and return the same things"""
    func = grad_dict[name]
    Xm, y, d, n, ctx, (p, pp, npar) = _staged(X, y, v, ctx)
    g = np.empty(p.size + 1)
    out = C.c_double()
    nat.check(getattr(nat.lib(), symbol)(ctx.handle, func.kernel_id, pp, npar, Xm.ctypes.data, d, n, y.ctypes.data, float(noise),
                                         C.byref(out), g.ctypes.data_as(C.POINTER(C.c_double))))
    return out.value, g


def logp_grad(X, y, noise, name, v, ctx=None):
    """(logp, grad) of GPR(X, y, noise, name(v)): the log marginal likelihood and its exact gradient, one native call
    (gprc_gpr_logp_grad).  `v` in the order `dens` takes it; grad has len(v) + 1 entries, d logp / d noise last
    (noise enters as K + noise * I).  Raises nat.NotPositiveDefinite when K + noise * I is not positive definite."""
    return _value_and_noise_grad("gprc_gpr_logp_grad", X, y, noise, name, v, ctx)


def loo_grad(X, y, noise, name, v, ctx=None):
    """(loo, grad) of GPR(X, y, noise, name(v)): the leave-one-out log predictive probability (Rasmussen & Williams 5.4.2), what
    GPR(...).loo_score returns, and its exact gradient, one native call (gprc_gpr_loo_grad).  The twin of `logp_grad`: `v` in the order
    `dens` takes it; grad has len(v) + 1 entries, d loo / d noise last.  Raises nat.NotPositiveDefinite when K + noise * I is not
    positive definite."""
    return _value_and_noise_grad("gprc_gpr_loo_grad", X, y, noise, name, v, ctx)


def elbo(X, y, noise, k, Z, jitter=1e-6, ctx=None):
    """The collapsed variational bound of the sparse GPR with inducing points Z (sparse.SparseGPR; gprc_sgpr_elbo): a lower bound of
    what `dens` returns for the same kernel and noise, equal to it at Z = X, jitter = 0.  `k` is a cov_func() object, as GPR takes it.
    `elbo_grad` is the same value with its exact gradient, `optimize_sparse` the optimiser over it."""
    from .sparse import elbo as _elbo
    return _elbo(X, y, noise, k, Z, jitter, ctx=ctx)


def elbo_grad(X, y, noise, name, v, Z, jitter=1e-6, with_Z=True, ctx=None):
    """(elbo, grad, dZ) of SparseGPR(X, y, noise, name(v), Z, jitter): the collapsed bound -- the bits `elbo` returns -- and its exact
    gradient, one native call (gprc_sgpr_elbo_grad).  `name` a key of grad_dict, `v` in the order `dens` takes it; grad has len(v) + 1
    entries, d elbo / d noise last; dZ is d x m like Z, d elbo / d Z[c, j], or None when not with_Z (grad has the same bits either
    way).  Raises nat.NotPositiveDefinite when K_uu + jitter I or B is not positive definite."""
    func = grad_dict[name]
    Xm, y, d, n, ctx, (p, pp, npar) = _staged(X, y, v, ctx, check_y="vector")
    Zm = as_d_points(Z, d, "Z")
    g = np.empty(p.size + 1)
    dZ = np.empty(Zm.shape, order="F") if with_Z else None
    out = C.c_double()
    nat.check(nat.lib().gprc_sgpr_elbo_grad(ctx.handle, func.kernel_id, pp, npar, Xm.ctypes.data, d, n, y.ctypes.data, float(noise),
                                            Zm.ctypes.data, Zm.shape[1], float(jitter), C.byref(out), g.ctypes.data,
                                            dZ.ctypes.data if with_Z else None))
    return out.value, g, dZ


def logq_grad(X, y, name, v, epsilon=1e-10, max_iter=0, ctx=None):
    """(logq, grad) of GP classification with kernel name(v) on (X, y), y in {-1, +1}: the Laplace approximation of the log
    evidence and its exact gradient (explicit part and the part through the mode), one native call (gprc_gpc_logq_grad).
    `logq` is the true evidence, -1/2 a.f + sum log sigmoid(y f) - sum(log(diag(L))): NOT GPC's `$logq`, which keeps the
    reference's sum(diag(L)).  The mode search is GPC(X, y, k, epsilon, reference_stop=False)'s; the default epsilon 1e-10
    (not GPC's 1e-5) is what a gradient accurate to 1e-10 needs.  Raises GprcError (ERR_MAXITER) when it does not converge
    within max_iter (0: 1000) steps."""
    func = grad_dict[name]
    Xm, y, d, n, ctx, (p, pp, npar) = _staged(X, y, v, ctx, check_y="size")
    g = np.empty(p.size)
    out = C.c_double()
    nat.check(nat.lib().gprc_gpc_logq_grad(ctx.handle, func.kernel_id, pp, npar, Xm.ctypes.data, d, n, y.ctypes.data, float(epsilon),
                                           int(max_iter), C.byref(out), g.ctypes.data_as(C.POINTER(C.c_double)), None))
    return out.value, g


def _from_log(z, n_log):
    """z -- one vector, or a stack of them, one per row -- with its first n_log entries exponentiated: the one place where an
    optimiser's vector leaves the log scale (an overflow is inf here; who evaluates there asks `_in_range`)"""
    t = z.copy()
    with np.errstate(over="ignore"):
        t[..., :n_log] = np.exp(z[..., :n_log])
    return t


def _in_range(t, n_log):
    """whether a point of _from_log (every row of a stack) can be evaluated: all finite, what came from a logarithm > 0"""
    return np.all(np.isfinite(t), axis=-1) & np.all(t[..., :n_log] > 0, axis=-1)


def _out_of_range():
    return ArithmeticError("parameter out of range")


class _Evaluation:
    """The rule "evaluate a point of z" of every optimiser here, with its one-entry cache: vmmin asks for the gradient at the point
    whose value it has just accepted, so one evaluation serves both.  z's first n_log entries are logarithms (the chain rule
    d / dz = theta * d / dtheta), the rest the variables themselves.  A point that fails is never cached."""

    def __init__(self, n_log):
        self.n_log = n_log
        self.key = self.val = self.grad = None

    def hit(self, z):
        return z.tobytes() == self.key

    def store(self, key, t, val, grad_theta):
        """what the objective returned at t = _from_log(z), key = z.tobytes() (z is the optimiser's working vector: taken before it moves)"""
        chain = np.ones(t.size)
        chain[:self.n_log] = t[:self.n_log]
        self.key, self.val, self.grad = key, float(val), np.asarray(grad_theta, dtype=np.float64) * chain

    def at(self, z, value_and_grad_theta):
        """(value, d value / dz) at z, from the cache or from value_and_grad_theta(theta) -> (value, d value / d theta); ArithmeticError
        when an exp(z) over- or underflows or an entry is not finite"""
        if not self.hit(z):
            key, t = z.tobytes(), _from_log(z, self.n_log)
            if not _in_range(t, self.n_log):
                raise _out_of_range()
            self.store(key, t, *value_and_grad_theta(t))
        return self.val, self.grad


def _maximise_over_log(z0, value_and_grad_theta, maxit, n_log=None, failed=SENTINEL):
    """vmmin on z = log(theta) of a function to MAXIMISE: value_and_grad_theta(theta) -> (value, d value / d theta), evaluated by the
    rule of `_Evaluation`; an evaluation that raises NotPositiveDefinite / ArithmeticError / a native iteration cap, or whose exp(z)
    over- or underflows, is the sentinel -10000 (optim_until_error).  n_log: only the first n_log entries of z are logarithms, the
    rest are the variables themselves (the inducing points of optimize_sparse; they must stay finite).  Returns vmmin's tuple (z in
    the same mixed form).  failed: what such an evaluation counts as instead of the sentinel (optimize_local: -inf, a point vmmin never
    accepts -- at its sizes the objective itself lies below -10000)."""
    point = _Evaluation(len(z0) if n_log is None else n_log)

    def fn(z):
        try:
            return -point.at(z, value_and_grad_theta)[0]
        except (nat.NotPositiveDefinite, ArithmeticError):
            return -failed

    return vmmin(z0, fn, lambda z: -point.at(z, value_and_grad_theta)[1], maxit=maxit)


class _Front:
    """What the six optimisers share around vmmin: the start values (defaulted, checked), the vector z = [log(theta), log(noise) when
    the noise is optimised, whatever else the caller appends] and its inverse, the gradient cut to match, and the result dict.
    noise=None: the objective has none (optimize_gpc).  many: `start` is S x p, one row per start (optimize_multistart)."""

    def __init__(self, who, name, d, start, noise=None, with_noise=False, many=False):
        if start is None:
            start = _default_start(name, d)
        start = np.asarray(start, dtype=np.float64)
        self.starts = np.atleast_2d(start) if many else np.atleast_1d(start).ravel()[None, :]
        if len(self.starts) < 1 or not (np.all(np.isfinite(self.starts)) and np.all(self.starts > 0)):
            raise ValueError(who + ": start values must be finite and > 0")
        self.name, self.noise, self.with_noise = name, noise, with_noise
        self.npar = self.starts.shape[1]
        self.n_log = self.npar + (1 if with_noise else 0)

    def pack(self, s=0, extra=None, log_noise=None):
        """z0 of start s.  log_noise: the noise's logarithm when the caller has its own (optimize_sparse takes libm's, which differs from
        numpy's in the last bit now and then: its iterates stay what they were)"""
        if not self.with_noise:
            z = np.log(self.starts[s])
        elif log_noise is None:
            z = np.log(np.concatenate([self.starts[s], [float(self.noise)]]))
        else:
            z = np.concatenate([np.log(self.starts[s]), [log_noise]])
        return z if extra is None else np.concatenate([z, extra])

    def split(self, t):
        """(theta, noise) of a point on the natural scale; (thetas, noises) of a stack of points, one per row"""
        if t.ndim == 1:
            return t[:self.npar].copy(), float(t[self.npar]) if self.with_noise else float(self.noise)
        return t[:, :self.npar].copy(), t[:, self.npar].copy() if self.with_noise else np.full(len(t), float(self.noise))

    def grad(self, g):
        """the objective's gradient (len(theta) + 1 entries, the noise last) without the noise's entry when the noise is fixed"""
        g = np.asarray(g, dtype=np.float64)
        return g if self.with_noise else g[:self.npar]

    def result(self, vmmin_tuple, **more):
        z, fmin, fncount, grcount, fail = vmmin_tuple
        t = _from_log(z, self.n_log)
        par = tuple(float(v) for v in t[:self.npar])
        noise = {} if self.noise is None else {"noise": self.split(t)[1]}
        return {"par": par, **noise, **more, "value": -fmin, "counts": (fncount, grcount), "convergence": fail, "func": _func_of(self.name, par)}


def optimize(X, y, noise, name, start=None, *, optimize_noise=True, maxit=100, value_and_grad=None, ctx=None, objective="logp"):
    """Maximise the log marginal likelihood of kernel `name` (a key of grad_dict: "sqrexp", "gammaexp", "rationalquadratic", "sqrexp_ard",
    "matern32", "matern52", "matern32_ard", "matern52_ard") over its parameters, and over the noise when `optimize_noise` and noise > 0, with vmmin on z = log(theta): every
    parameter stays positive, and d / dz = theta * d / dtheta.  start: parameter vector (default: cov_dict's start values;
    1 for the Matern kernels, ones(d) for the ARD kernels).  value_and_grad(theta, noise) -> (logp, grad) replaces the native objective (grad: len(theta) + 1,
    noise last).  An evaluation that fails (not positive definite, a parameter over- or underflowing) counts as the sentinel
    -10000, as in optim_until_error.  Returns dict(par, noise, value, counts, convergence, func): GPR(X, y, r["noise"],
    r["func"]) is the fitted model; convergence 0: converged, 1: maxit reached (optim's codes).
    objective: "logp" (the default) maximises the log marginal likelihood (`logp_grad`), "loo" the leave-one-out log predictive
    probability (`loo_grad`), the usual choice when the kernel family may be misspecified; anything else raises ValueError.  A
    `value_and_grad` hook replaces either."""
    if objective not in ("logp", "loo"):
        raise ValueError('optimize: objective must be "logp" or "loo"')
    func = grad_dict[name]   # noqa: F841  (KeyError for a kernel without a gradient)
    Xm = as_points(X)
    front = _Front("optimize", name, Xm.shape[0], start, noise, bool(optimize_noise) and noise > 0)
    if value_and_grad is None:
        ctx = ctx or nat.default_context()
        native = loo_grad if objective == "loo" else logp_grad
        value_and_grad = lambda theta, nz: native(Xm, y, nz, name, theta, ctx)   # noqa: E731

    def vg(t):
        val, g = value_and_grad(*front.split(t))
        return val, front.grad(g)

    return front.result(_maximise_over_log(front.pack(), vg, maxit))


BATCH_MAX_N = 128   # include/gprc_native.h GPRC_BATCH_MAX_N: the points of one batched model


def batch_layout(X, y, B, who="logp_grad_batch"):
    """The arrays the batched entry points take, (Xb, yb, d, n_max, x_stride, y_stride, n_each): one data set shared by B models
    (strides 0, n_each None), or lists of B data sets, which may differ in n, padded with zeros into one strided array each
    (point-major; the padding is never read).  More than 128 points a model: ValueError."""
    shared = not isinstance(X, (list, tuple))
    if shared:
        Xm = as_points(X)
        yb = np.ascontiguousarray(np.asarray(y, dtype=np.float64).ravel())
        d, n_max = Xm.shape
        if yb.size != n_max:
            raise ValueError("length(y) == ncol(X) is not TRUE")
        Xb, x_stride, y_stride, n_each = Xm, 0, 0, None
    else:
        if len(X) != B or len(y) != B:
            raise ValueError("%s: one data set per row of thetas" % who)
        pts = [as_points(x) for x in X]
        ys = [np.asarray(yy, dtype=np.float64).reshape(1, -1) for yy in y]
        d = pts[0].shape[0]
        if any(q.shape[0] != d or yy.size != q.shape[1] for q, yy in zip(pts, ys)):
            raise ValueError("%s: every data set needs the same nrow(X) and length(y) == ncol(X)" % who)
        Xb, n_each, n_max = pad_point_sets(pts)
        yb = pad_point_sets(ys)[0]
        x_stride, y_stride = d * n_max, n_max
    if n_max > BATCH_MAX_N:
        raise ValueError("%s: at most %d points a model; logp_grad takes larger ones" % (who, BATCH_MAX_N))
    return Xb, yb, d, n_max, x_stride, y_stride, n_each


def logp_grad_batch(X, y, noise, name, thetas, ctx=None):
    """`logp_grad` for B small models in ONE native call (gprc_gpr_batch_logp_grad: a model of at most 128 points per workgroup):
    (logp[B], grad[B, p + 1], info[B]).  thetas: B x p, a parameter vector per row in the order `dens` takes it (a vector is one
    model); noise: a scalar or B values; X, y: one data set shared by every model, or lists of B data sets, which may differ in n
    (they are padded into one strided array; the padding is never read).  grad's last column is d logp / d noise.  A model whose
    K + noise I is not positive definite does not raise: info[b] > 0 is the leading minor that failed, and its logp and grad are
    NaN.  More than 128 points: ValueError -- that is what `logp_grad` is for."""
    func = grad_dict[name]
    thetas = np.ascontiguousarray(np.atleast_2d(np.asarray(thetas, dtype=np.float64)))
    B, p = thetas.shape
    noises = np.ascontiguousarray(np.broadcast_to(np.asarray(noise, dtype=np.float64), (B,)))
    Xb, yb, d, n_max, x_stride, y_stride, n_each = batch_layout(X, y, B)
    logp, grad, info = np.empty(B), np.empty((B, p + 1)), np.zeros(B, dtype=np.intc)
    if B == 0:
        return logp, grad, info
    ctx = ctx or nat.default_context()
    nat.check(nat.lib().gprc_gpr_batch_logp_grad(ctx.handle, func.kernel_id, B, thetas.ctypes.data, p, p, noises.ctypes.data, Xb.ctypes.data, d,
                                                 n_max, x_stride, yb.ctypes.data, y_stride, None if n_each is None else n_each.ctypes.data,
                                                 logp.ctypes.data, grad.ctypes.data, None, info.ctypes.data))
    return logp, grad, info


def optimize_multistart(X, y, noise, name, starts=None, *, n_starts=8, rng=None, optimize_noise=True, maxit=100, value_and_grad_batch=None,
                        ctx=None):
    """`optimize` from several start values at about the wall time of one: one `vmmin_steps` instance per start on z = log(theta) (and
    log(noise), as `optimize`), in lockstep.  Every round collects the points the live instances wait on and evaluates them in ONE
    `logp_grad_batch` call (at most 128 points: the batched objective's limit); value and gradient come together and are kept per
    instance, so the gradient vmmin asks for at the point it has just accepted costs nothing; an instance that has finished drops out
    of the batch.  A model that is not positive definite (info > 0) or whose exp(z) over- or underflows is the sentinel -10000 for
    that instance only; at an instance's FIRST point it raises (NotPositiveDefinite / ArithmeticError), as `optimize` does there.
    starts: S x p start values; default: `optimize`'s default start, then n_starts - 1 copies of it multiplied entry by entry by
    log-uniform factors in [1/8, 8] from rng.  value_and_grad_batch(thetas, noises) -> (values, grads, infos) replaces the native
    objective (thetas m x p, noises m; grads m x (p + 1), noise last).  Each instance runs exactly what `optimize` runs from its
    start.  Returns `optimize`'s dict of the best start (the first maximum) with "all", the dict of every start in order, and
    "best_index"."""
    func = grad_dict[name]   # noqa: F841  (KeyError for a kernel without a gradient, as `optimize`)
    shared = not isinstance(X, (list, tuple))
    d = as_points(X).shape[0] if shared else as_points(X[0]).shape[0]
    if starts is None:
        base = np.atleast_1d(np.asarray(_default_start(name, d), dtype=np.float64)).ravel()
        rng = rng if rng is not None else np.random.default_rng()
        extra = np.exp(rng.uniform(math.log(1.0 / 8.0), math.log(8.0), (max(int(n_starts) - 1, 0), base.size)))
        starts = np.vstack([base[None, :], base[None, :] * extra])
    front = _Front("optimize_multistart", name, d, starts, noise, bool(optimize_noise) and noise > 0, many=True)
    if value_and_grad_batch is None:
        ctx = ctx or nat.default_context()
        value_and_grad_batch = lambda thetas, noises: logp_grad_batch(X, y, noises, name, thetas, ctx)   # noqa: E731

    class _Instance:   # one vmmin and the _Evaluation that `optimize` would give it
        def __init__(self, s):
            self.steps = vmmin_steps(front.pack(s), maxit)
            self.point = _Evaluation(front.n_log)
            self.result = None
            self.first = True
            self.want = next(self.steps)

        def advance(self, answer):
            try:
                self.want = self.steps.send(answer)
            except StopIteration as stop:
                self.want, self.result = None, stop.value

        def answer(self):
            """the cached point's value or gradient, whichever the instance waits on"""
            self.advance(-self.point.val if self.want[0] == "f" else -self.point.grad)

        def run_on_cache(self):
            """answers from the cache until the instance finishes or waits on a point that has to be evaluated"""
            while self.want is not None and self.point.hit(self.want[1]):
                self.answer()

        def failed(self, error):
            """the sentinel; vmmin without a gradient to go on raises what `optimize` raises from its gradient call"""
            if self.first or self.want[0] == "g":
                raise error
            self.advance(-SENTINEL)

    inst = [_Instance(s) for s in range(len(front.starts))]
    while True:
        for it in inst:
            it.run_on_cache()
        live = [it for it in inst if it.want is not None]
        if not live:
            break
        T = _from_log(np.array([it.want[1] for it in live]), front.n_log)
        rows = np.flatnonzero(_in_range(T, front.n_log))          # this round's one call: the points that can be evaluated
        if rows.size:
            vals, grads, infos = value_and_grad_batch(*front.split(T[rows]))
        where = {int(r): k for k, r in enumerate(rows)}
        for i, it in enumerate(live):
            k = where.get(i)
            if k is None:
                it.failed(_out_of_range())
            elif int(infos[k]) > 0:
                it.failed(nat.NotPositiveDefinite(int(infos[k])))
            else:
                it.point.store(it.want[1].tobytes(), T[i], vals[k], front.grad(grads[k]))
                it.first = False
                it.answer()

    results = [front.result(it.result) for it in inst]
    best = int(np.argmax([r["value"] for r in results]))
    return dict(results[best], all=results, best_index=best)


def optimize_sparse(X, y, noise, name, Z, start=None, *, optimize_noise=True, optimize_Z=True, jitter=1e-6, maxit=100, value_and_grad=None,
                    ctx=None):
    """Maximise the collapsed bound of the sparse GPR (sparse.SparseGPR) of kernel `name` (a key of grad_dict) over its parameters, over the
    noise when `optimize_noise`, and over the inducing points when `optimize_Z`, with vmmin on [log(theta), log(noise), vec(Z)]: the
    parameters and the noise stay positive (d / dz = theta * d / dtheta), the inducing points move freely (column-major, as Z lies in
    memory).  Z: d x m start positions (sparse.select_inducing picks columns of X); start: parameter vector (default as `optimize`).
    value_and_grad(theta, noise, Z) -> (elbo, grad, dZ) replaces the native objective `elbo_grad` (grad: len(theta) + 1, noise last; dZ:
    d x m, ignored unless optimize_Z).  An evaluation that fails (K_uu + jitter I or B not positive definite, a parameter over- or
    underflowing, an inducing point no longer finite) counts as the sentinel -10000, as in `optimize`.  Returns dict(par, noise, Z,
    value, counts, convergence, func): SparseGPR(X, y, r["noise"], r["func"], r["Z"], jitter) is the fitted model; convergence 0:
    converged, 1: maxit reached."""
    func = grad_dict[name]   # noqa: F841  (KeyError for a kernel without a gradient, as `optimize`)
    Xm = as_points(X)
    d = Xm.shape[0]
    Z0 = as_d_points(Z, d, "Z")
    front = _Front("optimize_sparse", name, d, start, noise, bool(optimize_noise))
    if not (noise > 0 and math.isfinite(noise)):
        raise ValueError("optimize_sparse: noise must be finite and > 0")
    with_Z = bool(optimize_Z)
    if value_and_grad is None:
        ctx = ctx or nat.default_context()
        value_and_grad = lambda theta, nz, Zc: elbo_grad(Xm, y, nz, name, theta, Zc, jitter, with_Z, ctx)   # noqa: E731

    def Z_of(t):   # the inducing points lie behind the logarithms, column-major, as Z lies in memory
        return np.asfortranarray(t[front.n_log:].reshape(Z0.shape, order="F")) if with_Z else Z0

    def vg(t):
        val, g, dZ = value_and_grad(*front.split(t), Z_of(t))
        g = front.grad(g)
        return val, np.concatenate([g, np.asarray(dZ, dtype=np.float64).ravel(order="F")]) if with_Z else g

    z0 = front.pack(extra=Z0.ravel(order="F") if with_Z else None, log_noise=math.log(noise))
    vm = _maximise_over_log(z0, vg, maxit, front.n_log)
    return front.result(vm, Z=Z_of(vm[0]))


def iter_logp_grad(X, y, noise, name, v, *, g1, g2, tol=1e-8, max_iter=1000, precond_rank=128, ctx=None):
    """(logp, se, grad) of IterativeGPR(X, y, noise, name(v), tol, max_iter, precond_rank): the stochastic estimate of the log marginal
    likelihood, its standard error over the probes and the estimate of its gradient (iterative.IterativeGPR.logp_grad;
    gprc_igpr_logp_grad), a deterministic function of the standard normals g2 (n x T) and g1 (precond_rank x T; rows beyond the rank the
    pivoted Cholesky reached are not used, and g1 may be None at precond_rank 0).  `v` in the order `dens` takes it; grad has len(v) + 1
    entries, d logp / d noise last.  Raises GprcError (ERR_MAXITER, ERR_NOT_PD) as the model does."""
    from .iterative import IterativeGPR
    with IterativeGPR(X, y, noise, _func_of(name, np.atleast_1d(np.asarray(v, dtype=np.float64))), tol=tol, max_iter=max_iter,
                      precond_rank=precond_rank, ctx=ctx) as model:
        r, T = model.stats.rank, np.asarray(g2).reshape(model.X.shape[1], -1).shape[1]
        if r > 0:
            g1 = np.asarray(g1, dtype=np.float64).reshape(-1, T)[:r]
        est = model.logp_grad(g1=g1 if r > 0 else None, g2=g2)
    return est.value, est.se, est.grad


def optimize_iterative(X, y, noise, name, start=None, *, n_probes=31, rng=None, tol=1e-8, max_iter=1000, precond_rank=128, optimize_noise=True,
                       maxit=100, value_and_grad=None, ctx=None):
    """`optimize` for the iterative exact GPR (iterative.IterativeGPR), at n where no n x n factor fits: maximise the stochastic estimate of
    the log marginal likelihood (`iter_logp_grad`) of kernel `name` over its parameters, and over the noise when `optimize_noise`, with
    vmmin on z = log(theta).  The standard normals behind the estimate -- g2 (n x n_probes), then g1 (precond_rank x n_probes), from rng
    -- are drawn ONCE and reused at every evaluation (common random numbers), so vmmin sees a deterministic objective.  value_and_grad(theta,
    noise) -> (logp, grad) or (logp, grad, se) replaces the native objective.  An evaluation that fails (the conjugate-gradient loop at
    its iteration cap, a matrix not positive definite in floating point, a parameter over- or underflowing) counts as the sentinel
    -10000.  Returns `optimize`'s dict(par, noise, value, counts, convergence, func) and `se`, the standard error of `value` (nan when
    the hook gives none): IterativeGPR(X, y, r["noise"], r["func"]) is the fitted model."""
    func = grad_dict[name]   # noqa: F841  (KeyError for a kernel without a gradient, as `optimize`)
    Xm = as_points(X)
    d, n = Xm.shape
    front = _Front("optimize_iterative", name, d, start, noise, bool(optimize_noise))
    if not (noise > 0 and math.isfinite(noise)):
        raise ValueError("optimize_iterative: noise must be finite and > 0")
    if value_and_grad is None:
        if int(n_probes) < 2:
            raise ValueError("optimize_iterative: n_probes >= 2 is not TRUE")
        ctx = ctx or nat.default_context()
        rng = rng if rng is not None else np.random.default_rng()
        g2 = np.asfortranarray(rng.standard_normal((n, int(n_probes))))
        g1 = np.asfortranarray(rng.standard_normal((min(int(precond_rank), n), int(n_probes))))

        def value_and_grad(theta, nz):
            try:
                val, se, g = iter_logp_grad(Xm, y, nz, name, theta, g1=g1, g2=g2, tol=tol, max_iter=max_iter, precond_rank=precond_rank, ctx=ctx)
            except nat.GprcError as e:
                if e.status in (nat.ERR_MAXITER, nat.ERR_NOT_PD):
                    raise ArithmeticError("the conjugate-gradient loop did not converge") from e
                raise
            return val, g, se

    se_of = {}

    def vg(t):
        out = value_and_grad(*front.split(t))
        g = front.grad(out[1])
        se_of[float(out[0])] = float(out[2]) if len(out) > 2 else float("nan")   # by value: vmmin returns the value it accepted
        return out[0], g

    r = front.result(_maximise_over_log(front.pack(), vg, maxit))
    return dict(r, se=se_of.get(r["value"], float("nan")))


def _ordered(X, y, order, seed, who):
    """(X, y, label) in the order of conditioning: order a permutation of the columns, "random" / "given" (local.vecchia_order), or None"""
    from .local import vecchia_order
    Xm = as_points(X)
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
    if y.ndim != 1 or y.size != Xm.shape[1]:
        raise ValueError("length(y) == ncol(X) is not TRUE")
    if order is None or (isinstance(order, str) and order == "given"):
        return Xm, y, "given"
    if isinstance(order, str):
        perm, label = vecchia_order(Xm, order, seed), order
    else:
        perm, label = np.asarray(order), "custom"
        if perm.ndim != 1 or perm.size != y.size or not np.array_equal(np.sort(perm), np.arange(y.size)):
            raise ValueError(who + ": order must be a permutation of 0 .. ncol(X) - 1")
    return np.asfortranarray(Xm[:, perm]), np.ascontiguousarray(y[perm]), label


def vecchia_logp_grad(X, y, noise, name, v, m=32, order=None, ctx=None):
    """(logp_V, grad) of LocalGPR(X, y, noise, name(v)): Vecchia's approximation of the log marginal likelihood -- every observation
    conditioned on its min(m, i) nearest earlier ones, in the metric of name(v) -- and its exact gradient, len(v) + 1 entries, d / d noise
    last (local.LocalGPR.vecchia_prepare + vecchia_logp_grad; gprc_lgpr_vecchia_logp_grad).  `name` a key of grad_dict, `v` in the order
    `dens` takes it; m: 1 .. 127; order: None / "given" (the columns as they come), "random", or a permutation.  With m >= n - 1 it is
    `logp_grad`'s value and gradient to rounding.  NaN when a conditional's model is not positive definite."""
    from .local import LocalGPR
    Xo, yo, _ = _ordered(X, y, order, 0, "vecchia_logp_grad")
    with LocalGPR(Xo, yo, noise, _func_of(name, np.atleast_1d(np.asarray(v, dtype=np.float64))), m=min(int(m) + 1, 128), ctx=ctx) as model:
        model.vecchia_prepare(m)
        return model.vecchia_logp_grad()


def optimize_local(X, y, noise, name, start=None, *, m=32, order="random", seed=0, rounds=None, optimize_noise=True, maxit=100, value_and_grad=None,
                   ctx=None):
    """`optimize` for the local GPR (local.LocalGPR), at n where no n x n factor fits: maximise the Vecchia likelihood (`vecchia_logp_grad`)
    of kernel `name` over its parameters, and over the noise when `optimize_noise` and noise > 0, with vmmin on z = log(theta).  (X, y) are
    put into `order` first ("random" with `seed`, "given", or a permutation: local.vecchia_order).  A pass searches the conditioning
    sets in the metric of its start values (vecchia_prepare), freezes them and runs vmmin; `rounds` passes, each from the previous result:
    default 2 for the ARD kernels, whose metric moves with the parameters, 1 otherwise.  value_and_grad(theta, noise) -> (logp_V, grad)
    replaces the native objective; value_and_grad.prepare(theta, noise), when it has one, is called at the start of every pass.  An
    evaluation that fails (a model not positive definite, a parameter over- or underflowing) is a point vmmin never accepts: it counts as
    -inf, not as the siblings' sentinel -10000, which at n = 2^20 lies far ABOVE the likelihood itself.  Returns
    `optimize`'s dict(par, noise, value, counts, convergence, func) of the last pass, counts added over the passes, and `m`, `order`,
    `rounds`: LocalGPR(X, y, r["noise"], r["func"]) is the fitted model."""
    func = grad_dict[name]   # noqa: F841  (KeyError for a kernel without a gradient, as `optimize`)
    if int(m) != m or not 1 <= int(m) <= 127:
        raise ValueError("optimize_local: m must be an integer in 1 .. 127")
    rounds = (2 if _is_ard(name) else 1) if rounds is None else int(rounds)
    if rounds < 1:
        raise ValueError("optimize_local: rounds >= 1 is not TRUE")
    Xo, yo, label = _ordered(X, y, order, seed, "optimize_local")
    d = Xo.shape[0]
    front = _Front("optimize_local", name, d, start, noise, bool(optimize_noise) and noise > 0)
    model = None
    if value_and_grad is None:
        from .local import LocalGPR
        model = LocalGPR(Xo, yo, noise, _func_of(name, front.starts[0]), m=min(int(m) + 1, 128), ctx=ctx)

        def value_and_grad(theta, nz):
            with np.errstate(divide="ignore", over="ignore"):
                if not _in_range(1.0 / theta, theta.size):   # a subnormal length scale: finite and > 0, but 1 / l is not (the native layer refuses it)
                    raise _out_of_range()
            val, g = model.vecchia_logp_grad(theta, nz)
            if model.vecchia_flagged or not math.isfinite(val):
                raise ArithmeticError("a conditional's model is not positive definite")
            return val, g

        def prepare(theta, nz):
            model.set_params(_func_of(name, theta), nz)
            model.vecchia_prepare(int(m))
    else:
        prepare = getattr(value_and_grad, "prepare", lambda theta, nz: None)

    def vg(t):
        val, g = value_and_grad(*front.split(t))
        return val, front.grad(g)

    try:
        z, fn, gr = front.pack(), 0, 0
        for _ in range(rounds):
            prepare(*front.split(_from_log(z, front.n_log)))
            out = _maximise_over_log(z, vg, maxit, failed=-math.inf)
            z, fn, gr = out[0], fn + out[2], gr + out[3]
        return front.result((z, out[1], fn, gr, out[4]), m=int(m), order=label, rounds=rounds)
    finally:
        if model is not None:
            model.close()


def optimize_gpc(X, y, name, start=None, *, epsilon=1e-10, maxit=100, value_and_grad=None, ctx=None):
    """Maximise the Laplace log evidence of GP classification (y in {-1, +1}) over the parameters of kernel `name` ("sqrexp",
    "gammaexp", "rationalquadratic", "sqrexp_ard", "matern32", "matern52", "matern32_ard", "matern52_ard") with vmmin on z = log(theta), exactly as `optimize` does for regression.
    start: parameter vector (default: cov_dict's start values; 1 for the Matern kernels, ones(d) for the ARD kernels).  value_and_grad(theta) -> (logq, grad)
    replaces the native objective `logq_grad`.  An evaluation that fails (a mode search that does not converge, a parameter
    over- or underflowing) counts as the sentinel -10000.  Returns dict(par, value, counts, convergence, func):
    GPC(X, y, r["func"], reference_stop=False) is the fitted classifier; convergence 0: converged, 1: maxit reached."""
    func = grad_dict[name]   # noqa: F841  (KeyError for a kernel without a gradient, as `optimize`)
    Xm = as_points(X)
    front = _Front("optimize_gpc", name, Xm.shape[0], start)
    if value_and_grad is None:
        ctx = ctx or nat.default_context()

        def value_and_grad(theta):
            try:
                return logq_grad(Xm, y, name, theta, epsilon, 0, ctx)
            except nat.GprcError as e:
                if e.status == nat.ERR_MAXITER:
                    raise ArithmeticError("the mode search did not converge") from e
                raise

    return front.result(_maximise_over_log(front.pack(), lambda t: value_and_grad(t.copy()), maxit))


def _optim_brent_until_error(f, lower, upper):
    """optim_until_error(start, f, method = "Brent", lower, upper, control = list(fnscale = -1))  (R/fit.R:47-69):
    failing evaluations return the sentinel; optimize() minimises f / fnscale = -f with tol = sqrt(eps)."""
    def f_new(par):
        try:
            return f(par)
        except (nat.NotPositiveDefinite, ArithmeticError):
            return SENTINEL
    tol = math.sqrt(np.finfo(float).eps)  # optim's default reltol
    xmin = brent_fmin(lambda p_: -f_new(p_), lower, upper, tol)
    return xmin, f_new(xmin)


def _optim_bfgs_until_error(start, f, gr):
    """optim_until_error(start, f, gr = dens_deriv, method = "BFGS", control = list(fnscale = -1))  (R/fit.R:47-69,
    :157-158).  Only f is wrapped by the sentinel (:49-55); an error inside gr aborts optim (:56), after which the best
    (par, value) among the successful evaluations so far is returned (:63-65), or f(start) if there was none (:58-61).
    `f`/`gr` here take the objective/gradient failures as nat.NotPositiveDefinite / ArithmeticError."""
    seen = []  # (par, value) of every successful evaluation, in order

    def f_new(par):
        try:
            out = float(f(par))
        except (nat.NotPositiveDefinite, ArithmeticError):
            return SENTINEL
        if out != SENTINEL:
            seen.append((np.array(par, dtype=np.float64), out))
        return out

    try:  # optim minimises fn / fnscale and gr / fnscale with fnscale = -1
        par, val, *_ = vmmin(np.asarray(start, dtype=np.float64), lambda p_: -f_new(p_), lambda p_: -np.asarray(gr(p_)))
        return tuple(float(x) for x in par), -val
    except (nat.NotPositiveDefinite, ArithmeticError):
        if not seen:
            try:
                value = float(f(np.asarray(start, dtype=np.float64)))
            except (nat.NotPositiveDefinite, ArithmeticError):
                value = SENTINEL
            return tuple(float(x) for x in start), value
        best = max(range(len(seen)), key=lambda i: (seen[i][1], -i))  # which.max: the first maximum
        return tuple(float(x) for x in seen[best][0]), seen[best][1]


def fit(X, y, noise, cov_names=None, *, ctx=None):
    """fit(X, y, noise, cov_names = as.list(cov_df$name))  --  R/fit.R:110-169.
    Returns dict(par, cov, score, func); `func` is a tagged cov_func closure, ready for GPR / GPC."""
    names = list(cov_dict) if cov_names is None else list(cov_names)
    for nm in names:
        if nm not in cov_dict:
            raise KeyError(nm)
    Xm = as_points(X)
    ctx = ctx or nat.default_context()
    params, score = [], []
    for nm in names:
        if nm == "polynomial":  # R/fit.R:146-155: Brent over sigma in [0, 5] for every degree 1..10
            best = None
            for deg in range(1, 11):
                par, val = _optim_brent_until_error(lambda sig, deg=deg: dens(Xm, y, noise, nm, [sig, float(deg)], ctx), 0.0, 5.0)
                if best is None or val > best[1]:   # which.max: first maximum wins
                    best = ((par, float(deg)), val)
            params.append(best[0])
            score.append(best[1])
        elif len(cov_dict[nm][2]) == 2:  # gammaexp, rationalquadratic: BFGS with dens_deriv  (R/fit.R:125-140, 144)
            par, val = _optim_bfgs_until_error(cov_dict[nm][2], lambda v, nm=nm: dens(Xm, y, noise, nm, v, ctx),
                                               lambda v, nm=nm: dens_deriv(Xm, y, nm, v, ctx))
            params.append(par)
            score.append(val)
        else:                   # one parameter: Brent on [0, 10]  (R/fit.R:143, 157-158)
            par, val = _optim_brent_until_error(lambda v: dens(Xm, y, noise, nm, [v], ctx), 0.0, 10.0)
            params.append((par,))
            score.append(val)
    w = int(np.argmax(score))
    name, par = names[w], params[w]
    sys.stderr.write("The optimal covariance function is %s, with parameters %s\n" % (name, ", ".join("%.15g" % p for p in par)))  # :166
    func = cov_dict[name][0]
    return {"par": tuple(par), "cov": name, "score": list(score), "func": CovFunc(func, func.bind(par, {}))}
