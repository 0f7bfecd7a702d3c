"""fit(): hyper-parameter selection by maximising the log marginal likelihood (reference R/fit.R:110-169) --
the immediate caller of the hot path.

What runs where
  * the objective `dens(v)` (R/fit.R:117-124: K, Cholesky, alpha, log marginal likelihood) is one native call,
    gprc_gpr_log_marginal; the reference's O(n^4) `min(det(leading minors)) > 0` guard (:119) is the Cholesky's
    own positive-definiteness test;
  * the optimiser driver is host code, as in the reference.  R's `optim(method = "Brent")` is `optimize()`, Brent's
    fmin; it is restated here (golden section + successive parabolic interpolation, tol = sqrt(.Machine$double.eps))
    so that the one-parameter kernels (sqrexp, constant, linear) and the polynomial degree loop follow the same
    iterates.  `optim_until_error` (R/fit.R:47-69) is kept: a failing evaluation yields the sentinel -10000.
  * the two-parameter kernels gammaexp / rationalquadratic go through `optim(method = "BFGS")` with the gradient
    `dens_deriv` (R/fit.R:126-139).  That gradient is reproduced AS WRITTEN, by the native gprc_fit_gradient: it
    inverts the noise-free K, ignores `noise`, applies `diag(.) %*%` where a trace is meant and binds the parameter
    vector in `deriv`'s argument order, which is the reverse of the kernels' own.  R's BFGS is `vmmin` (Nash's
    variable-metric Algorithm 21); it is restated below.  Consequences that follow from the reference's code and are
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
from .covfunc import (CovFunc, as_points, constant, linear, polynomial, sqrexp, gammaexp, rationalquadratic, sqrexp_ard, matern32, matern52,
                      matern32_ard, matern52_ard)

__all__ = ["fit", "dens", "dens_deriv", "logp_grad", "logp_grad_batch", "loo_grad", "optimize", "optimize_multistart", "vmmin_steps", "logq_grad", "optimize_gpc", "elbo", "elbo_grad", "optimize_sparse",
           "cov_dict", "brent_fmin", "vmmin"]

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


def dens(X, y, noise, name, v, ctx=None):
    """dens(v) of R/fit.R:117-124 for kernel `name` with parameter vector v (in the generic's argument order).
    Raises nat.NotPositiveDefinite when K + noise*I is not positive definite (the reference's stopifnot / chol error).
    `name` may also be a kernel of grad_dict that is not in cov_dict: "sqrexp_ard", "matern32_ard", "matern52_ard" (v = one length
    scale per row of X), "matern32", "matern52" (v = the length scale)."""
    func = _kernel_by_name(name)
    Xm = as_points(X)
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
    d, n = Xm.shape
    ctx = ctx or nat.default_context()
    _, pp, npar = nat.params_array(np.atleast_1d(np.asarray(v, dtype=np.float64)))
    out = C.c_double()
    nat.check(nat.lib().gprc_gpr_log_marginal(ctx.handle, func.kernel_id, pp, npar, Xm.ctypes.data, d, n, y.ctypes.data,
                                              float(noise), C.byref(out)))
    return out.value


def dens_deriv(X, y, name, v, ctx=None):
    """dens_deriv(v) of R/fit.R:126-139 (quirks included, see the module docstring) for kernel `name`.
    Raises nat.NotPositiveDefinite when the noise-free K cannot be inverted (the reference's solve(K) error)."""
    func = cov_dict[name][0]
    Xm = as_points(X)
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
    d, n = Xm.shape
    ctx = ctx or nat.default_context()
    p, pp, npar = nat.params_array(np.atleast_1d(np.asarray(v, dtype=np.float64)))
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


def logp_grad(X, y, noise, name, v, ctx=None):
    """(logp, grad) of GPR(X, y, noise, name(v)): the log marginal likelihood and its exact gradient, one native call
    (gprc_gpr_logp_grad).  `v` in the order `dens` takes it; grad has len(v) + 1 entries, d logp / d noise last
    (noise enters as K + noise * I).  Raises nat.NotPositiveDefinite when K + noise * I is not positive definite."""
    func = grad_dict[name]
    Xm = as_points(X)
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
    d, n = Xm.shape
    ctx = ctx or nat.default_context()
    p, pp, npar = nat.params_array(np.atleast_1d(np.asarray(v, dtype=np.float64)))
    g = np.empty(p.size + 1)
    out = C.c_double()
    nat.check(nat.lib().gprc_gpr_logp_grad(ctx.handle, func.kernel_id, pp, npar, Xm.ctypes.data, d, n, y.ctypes.data, float(noise),
                                           C.byref(out), g.ctypes.data_as(C.POINTER(C.c_double))))
    return out.value, g


def loo_grad(X, y, noise, name, v, ctx=None):
    """(loo, grad) of GPR(X, y, noise, name(v)): the leave-one-out log predictive probability (Rasmussen & Williams 5.4.2), what
    GPR(...).loo_score returns, and its exact gradient, one native call (gprc_gpr_loo_grad).  The twin of `logp_grad`: `v` in the order
    `dens` takes it; grad has len(v) + 1 entries, d loo / d noise last.  Raises nat.NotPositiveDefinite when K + noise * I is not
    positive definite."""
    func = grad_dict[name]
    Xm = as_points(X)
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
    d, n = Xm.shape
    ctx = ctx or nat.default_context()
    p, pp, npar = nat.params_array(np.atleast_1d(np.asarray(v, dtype=np.float64)))
    g = np.empty(p.size + 1)
    out = C.c_double()
    nat.check(nat.lib().gprc_gpr_loo_grad(ctx.handle, func.kernel_id, pp, npar, Xm.ctypes.data, d, n, y.ctypes.data, float(noise),
                                          C.byref(out), g.ctypes.data_as(C.POINTER(C.c_double))))
    return out.value, g


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
    Xm = np.asfortranarray(as_points(X))
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
    d, n = Xm.shape
    if y.ndim != 1 or y.size != n:
        raise ValueError("length(y) == ncol(X) is not TRUE")
    Zm = np.asfortranarray(as_points(Z, d=d, what="Z") if np.ndim(Z) <= 1 else as_points(Z, what="Z"))
    if Zm.shape[0] != d:
        raise ValueError("Z must have nrow(X) rows")
    ctx = ctx or nat.default_context()
    p, pp, npar = nat.params_array(np.atleast_1d(np.asarray(v, dtype=np.float64)))
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
    Xm = as_points(X)
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
    d, n = Xm.shape
    if y.size != n:
        raise ValueError("length(y) == ncol(X) is not TRUE")
    ctx = ctx or nat.default_context()
    p, pp, npar = nat.params_array(np.atleast_1d(np.asarray(v, dtype=np.float64)))
    g = np.empty(p.size)
    out = C.c_double()
    nat.check(nat.lib().gprc_gpc_logq_grad(ctx.handle, func.kernel_id, pp, npar, Xm.ctypes.data, d, n, y.ctypes.data, float(epsilon),
                                           int(max_iter), C.byref(out), g.ctypes.data_as(C.POINTER(C.c_double)), None))
    return out.value, g


def _maximise_over_log(z0, value_and_grad_theta, maxit, n_log=None):
    """vmmin on z = log(theta) of a function to MAXIMISE: value_and_grad_theta(theta) -> (value, d value / d theta); the chain
    rule d / dz = theta * d / dtheta; an evaluation that raises NotPositiveDefinite / ArithmeticError / a native iteration cap,
    or whose exp(z) over- or underflows, is the sentinel -10000 (optim_until_error).  n_log: only the first n_log entries of z are
    logarithms, the rest are the variables themselves (the inducing points of optimize_sparse; they must stay finite).  Returns
    vmmin's tuple (z in the same mixed form)."""
    last = {}   # vmmin asks for the gradient at the point whose value it has just accepted: one evaluation serves both
    n_log = len(z0) if n_log is None else n_log

    def evaluate(z):
        key = z.tobytes()
        if last.get("key") != key:
            t, chain = z.copy(), np.ones(z.size)
            with np.errstate(over="ignore"):
                t[:n_log] = np.exp(z[:n_log])
            chain[:n_log] = t[:n_log]
            if not (np.all(np.isfinite(t)) and np.all(t[:n_log] > 0)):
                raise ArithmeticError("parameter out of range")
            val, g = value_and_grad_theta(t)
            last.update(key=key, val=float(val), grad=np.asarray(g, dtype=np.float64) * chain)
        return last["val"], last["grad"]

    def fn(z):
        try:
            return -evaluate(z)[0]
        except (nat.NotPositiveDefinite, ArithmeticError):
            return -SENTINEL

    return vmmin(z0, fn, lambda z: -evaluate(z)[1], maxit=maxit)


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
    func = grad_dict[name]
    Xm = as_points(X)
    d = Xm.shape[0]
    if start is None:
        start = _default_start(name, d)
    theta0 = np.atleast_1d(np.asarray(start, dtype=np.float64)).ravel()
    npar = theta0.size
    with_noise = bool(optimize_noise) and noise > 0
    if not (np.all(np.isfinite(theta0)) and np.all(theta0 > 0)):
        raise ValueError("optimize: start values must be finite and > 0")
    if value_and_grad is None:
        ctx = ctx or nat.default_context()
        native = loo_grad if objective == "loo" else logp_grad
        value_and_grad = lambda theta, nz: native(Xm, y, nz, name, theta, ctx)   # noqa: E731
    z0 = np.log(np.concatenate([theta0, [float(noise)]]) if with_noise else theta0)

    def vg(t):
        val, g = value_and_grad(t[:npar].copy(), float(t[npar]) if with_noise else float(noise))
        g = np.asarray(g, dtype=np.float64)
        return val, (g if with_noise else g[:npar])

    z, fmin, fncount, grcount, fail = _maximise_over_log(z0, vg, maxit)
    t = np.exp(z)
    par = tuple(float(v) for v in t[:npar])
    return {"par": par, "noise": float(t[npar]) if with_noise else float(noise), "value": -fmin, "counts": (fncount, grcount),
            "convergence": fail, "func": _func_of(name, par)}


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
        d = pts[0].shape[0]
        n_each = np.array([q.shape[1] for q in pts], dtype=np.int64)
        n_max = int(n_each.max())
        Xb, yb = np.zeros((B, d * n_max)), np.zeros((B, n_max))
        for b, (q, yy) in enumerate(zip(pts, y)):
            yy = np.asarray(yy, dtype=np.float64).ravel()
            if q.shape[0] != d or yy.size != q.shape[1]:
                raise ValueError("%s: every data set needs the same nrow(X) and length(y) == ncol(X)" % who)
            Xb[b, :q.size] = q.ravel(order="F")
            yb[b, :yy.size] = yy
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
    starts = np.atleast_2d(np.asarray(starts, dtype=np.float64))
    S, npar = starts.shape
    if S < 1 or not (np.all(np.isfinite(starts)) and np.all(starts > 0)):
        raise ValueError("optimize_multistart: start values must be finite and > 0")
    with_noise = bool(optimize_noise) and noise > 0
    if value_and_grad_batch is None:
        ctx = ctx or nat.default_context()
        value_and_grad_batch = lambda thetas, noises: logp_grad_batch(X, y, noises, name, thetas, ctx)   # noqa: E731

    class _Instance:   # one vmmin with _maximise_over_log's cache: the last evaluated point, its value and chained gradient
        def __init__(self, theta0):
            self.steps = vmmin_steps(np.log(np.concatenate([theta0, [float(noise)]]) if with_noise else theta0), maxit)
            self.key = self.val = self.grad = self.result = None
            self.first = True
            self.want = next(self.steps)

        def advance(self, answer):
            try:
                self.want = self.steps.send(answer)
            except StopIteration as stop:
                self.want, self.result = None, stop.value

        def run_on_cache(self):
            """answers from the cache until the instance finishes or waits on a point that has to be evaluated"""
            while self.want is not None and self.want[1].tobytes() == self.key:
                self.advance(-self.val if self.want[0] == "f" else -self.grad)

    inst = [_Instance(starts[s]) for s in range(S)]
    while True:
        for it in inst:
            it.run_on_cache()
        live = [it for it in inst if it.want is not None]
        if not live:
            break
        with np.errstate(over="ignore"):
            T = np.array([np.exp(it.want[1]) for it in live])
        in_range = np.all(np.isfinite(T), axis=1) & np.all(T > 0, axis=1)
        rows = np.flatnonzero(in_range)
        vals = grads = infos = None
        if rows.size:
            vals, grads, infos = value_and_grad_batch(T[rows, :npar].copy(), T[rows, npar].copy() if with_noise else np.full(rows.size, float(noise)))
            grads = np.asarray(grads, dtype=np.float64)
        where = {int(r): k for k, r in enumerate(rows)}
        for i, it in enumerate(live):
            k = where.get(i)
            failed = k is None or int(infos[k]) > 0
            if failed:
                if it.first or it.want[0] == "g":   # vmmin has no gradient to go on: what `optimize` raises from its gradient call
                    raise (ArithmeticError("parameter out of range") if k is None else nat.NotPositiveDefinite(int(infos[k])))
                it.first = False
                it.advance(-SENTINEL)
                continue
            g = grads[k] if with_noise else grads[k][:npar]
            it.key, it.val, it.grad = it.want[1].tobytes(), float(vals[k]), g * T[i]
            it.first = False
            it.advance(-it.val if it.want[0] == "f" else -it.grad)

    results = []
    for it in inst:
        z, fmin, fncount, grcount, fail = it.result
        t = np.exp(z)
        par = tuple(float(v) for v in t[:npar])
        results.append({"par": par, "noise": float(t[npar]) if with_noise else float(noise), "value": -fmin, "counts": (fncount, grcount),
                        "convergence": fail, "func": _func_of(name, par)})
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
    func = grad_dict[name]
    Xm = as_points(X)
    d = Xm.shape[0]
    Z0 = np.asfortranarray(as_points(Z, d=d, what="Z") if np.ndim(Z) <= 1 else as_points(Z, what="Z"))
    if Z0.shape[0] != d:
        raise ValueError("Z must have nrow(X) rows")
    m = Z0.shape[1]
    if start is None:
        start = _default_start(name, d)
    theta0 = np.atleast_1d(np.asarray(start, dtype=np.float64)).ravel()
    npar = theta0.size
    if not (np.all(np.isfinite(theta0)) and np.all(theta0 > 0)):
        raise ValueError("optimize_sparse: start values must be finite and > 0")
    if not (noise > 0 and math.isfinite(noise)):
        raise ValueError("optimize_sparse: noise must be finite and > 0")
    with_noise, with_Z = bool(optimize_noise), bool(optimize_Z)
    if value_and_grad is None:
        ctx = ctx or nat.default_context()
        value_and_grad = lambda theta, nz, Zc: elbo_grad(Xm, y, nz, name, theta, Zc, jitter, with_Z, ctx)   # noqa: E731
    n_log = npar + (1 if with_noise else 0)
    z0 = np.concatenate([np.log(theta0), [math.log(noise)] if with_noise else [], Z0.ravel(order="F") if with_Z else []])

    def split(t):
        return (t[:npar].copy(), float(t[npar]) if with_noise else float(noise),
                np.asfortranarray(t[n_log:].reshape((d, m), order="F")) if with_Z else Z0)

    def vg(t):
        val, g, dZ = value_and_grad(*split(t))
        g = np.asarray(g, dtype=np.float64)
        return val, np.concatenate([g if with_noise else g[:npar], np.asarray(dZ, dtype=np.float64).ravel(order="F") if with_Z else []])

    z, fmin, fncount, grcount, fail = _maximise_over_log(z0, vg, maxit, n_log)
    t = z.copy()
    t[:n_log] = np.exp(z[:n_log])
    par_v, noise_v, Z_v = split(t)
    par = tuple(float(v) for v in par_v)
    return {"par": par, "noise": noise_v, "Z": Z_v, "value": -fmin, "counts": (fncount, grcount), "convergence": fail,
            "func": _func_of(name, par)}


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
    if start is None:
        start = _default_start(name, d)
    theta0 = np.atleast_1d(np.asarray(start, dtype=np.float64)).ravel()
    npar = theta0.size
    if not (np.all(np.isfinite(theta0)) and np.all(theta0 > 0)):
        raise ValueError("optimize_iterative: start values must be finite and > 0")
    if not (noise > 0 and math.isfinite(noise)):
        raise ValueError("optimize_iterative: noise must be finite and > 0")
    with_noise = bool(optimize_noise)
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

    z0 = np.log(np.concatenate([theta0, [float(noise)]]) if with_noise else theta0)
    se_of = {}

    def vg(t):
        out = value_and_grad(t[:npar].copy(), float(t[npar]) if with_noise else float(noise))
        g = np.asarray(out[1], dtype=np.float64)
        se_of[float(out[0])] = float(out[2]) if len(out) > 2 else float("nan")   # by value: vmmin returns the value it accepted
        return out[0], (g if with_noise else g[:npar])

    z, fmin, fncount, grcount, fail = _maximise_over_log(z0, vg, maxit)
    t = np.exp(z)
    par = tuple(float(v) for v in t[:npar])
    return {"par": par, "noise": float(t[npar]) if with_noise else float(noise), "value": -fmin, "counts": (fncount, grcount),
            "convergence": fail, "func": _func_of(name, par), "se": se_of.get(-fmin, float("nan"))}


def optimize_gpc(X, y, name, start=None, *, epsilon=1e-10, maxit=100, value_and_grad=None, ctx=None):
    """Maximise the Laplace log evidence of GP classification (y in {-1, +1}) over the parameters of kernel `name` ("sqrexp",
    "gammaexp", "rationalquadratic", "sqrexp_ard", "matern32", "matern52", "matern32_ard", "matern52_ard") with vmmin on z = log(theta), exactly as `optimize` does for regression.
    start: parameter vector (default: cov_dict's start values; 1 for the Matern kernels, ones(d) for the ARD kernels).  value_and_grad(theta) -> (logq, grad)
    replaces the native objective `logq_grad`.  An evaluation that fails (a mode search that does not converge, a parameter
    over- or underflowing) counts as the sentinel -10000.  Returns dict(par, value, counts, convergence, func):
    GPC(X, y, r["func"], reference_stop=False) is the fitted classifier; convergence 0: converged, 1: maxit reached."""
    func = grad_dict[name]
    Xm = as_points(X)
    d = Xm.shape[0]
    if start is None:
        start = _default_start(name, d)
    theta0 = np.atleast_1d(np.asarray(start, dtype=np.float64)).ravel()
    if not (np.all(np.isfinite(theta0)) and np.all(theta0 > 0)):
        raise ValueError("optimize_gpc: start values must be finite and > 0")
    if value_and_grad is None:
        ctx = ctx or nat.default_context()

        def value_and_grad(theta):
            try:
                return logq_grad(Xm, y, name, theta, epsilon, 0, ctx)
            except nat.GprcError as e:
                if e.status == nat.ERR_MAXITER:
                    raise ArithmeticError("the mode search did not converge") from e
                raise

    z, fmin, fncount, grcount, fail = _maximise_over_log(np.log(theta0), lambda t: value_and_grad(t.copy()), maxit)
    par = tuple(float(v) for v in np.exp(z))
    return {"par": par, "value": -fmin, "counts": (fncount, grcount), "convergence": fail,
            "func": _func_of(name, par)}


def vmmin(b0, fn, gr, maxit=100, abstol=-math.inf, reltol=math.sqrt(np.finfo(float).eps)):
    """R's optim(method = "BFGS") core: Nash's variable-metric minimiser (Compact Numerical Methods, Algorithm 21)
    with R's constants (stepredn 0.2, acctol 1e-4, reltest 10).  Minimises fn; returns (par, value, fncount, grcount,
    fail).  The algorithm is `vmmin_steps`; this is its driver for one instance: every value it asks for is fn's, every
    gradient gr's."""
    steps = vmmin_steps(b0, maxit, abstol, reltol)
    try:
        kind, point = next(steps)
        while True:
            kind, point = steps.send(fn(point) if kind == "f" else gr(point))
    except StopIteration as stop:
        return stop.value


def vmmin_steps(b0, maxit=100, abstol=-math.inf, reltol=math.sqrt(np.finfo(float).eps)):
    """`vmmin` as a generator, so that several instances can run in lockstep on one batched objective (`optimize_multistart`): it
    yields ("f", point) when it wants the value at `point` and ("g", point) when it wants the gradient there, is sent the answer, and
    returns vmmin's tuple (par, value, fncount, grcount, fail) as the value of its StopIteration.  `point` is the instance's own
    working vector: it is valid until the answer is sent.  Restated from the published algorithm; control flow details that matter
    for the reference's behaviour: a non-finite initial value is an error (ArithmeticError, raised into whoever drives the
    generator); a search direction that is not downhill (including a NaN gradient projection) resets B once and then terminates."""
    stepredn, acctol, reltest = 0.2, 1e-4, 10.0
    b = np.array(b0, dtype=np.float64)
    n = b.size
    if maxit <= 0:
        return b, float((yield ("f", b))), 0, 0, 0
    f = float((yield ("f", b)))
    if not math.isfinite(f):
        raise ArithmeticError("initial value in 'vmmin' is not finite")
    fmin = f
    funcount = gradcount = 1
    g = np.array((yield ("g", b)), dtype=np.float64)
    it = 1
    ilast = gradcount
    B = np.zeros((n, n))
    count = 0
    while True:
        if ilast == gradcount:
            B = np.eye(n)
        X = b.copy()
        c = g.copy()
        t = np.empty(n)
        gradproj = 0.0
        for i in range(n):
            sacc = 0.0
            for j in range(i + 1):
                sacc -= B[i, j] * g[j]
            for j in range(i + 1, n):
                sacc -= B[j, i] * g[j]
            t[i] = sacc
            gradproj += sacc * g[i]
        if gradproj < 0.0:  # downhill
            steplength = 1.0
            accpoint = False
            while True:
                count = 0
                for i in range(n):
                    b[i] = X[i] + steplength * t[i]
                    if reltest + X[i] == reltest + b[i]:
                        count += 1
                if count < n:
                    f = float((yield ("f", b)))
                    funcount += 1
                    accpoint = math.isfinite(f) and f <= fmin + gradproj * steplength * acctol
                    if not accpoint:
                        steplength *= stepredn
                if count == n or accpoint:
                    break
            enough = f > abstol and abs(f - fmin) > reltol * (abs(fmin) + reltol)
            if not enough:
                count = n
                fmin = f
            if count < n:  # making progress
                fmin = f
                g = np.array((yield ("g", b)), dtype=np.float64)
                gradcount += 1
                it += 1
                D1 = 0.0
                for i in range(n):
                    t[i] = steplength * t[i]
                    c[i] = g[i] - c[i]
                    D1 += t[i] * c[i]
                if D1 > 0:
                    D2 = 0.0
                    for i in range(n):
                        sacc = 0.0
                        for j in range(i + 1):
                            sacc += B[i, j] * c[j]
                        for j in range(i + 1, n):
                            sacc += B[j, i] * c[j]
                        X[i] = sacc
                        D2 += sacc * c[i]
                    D2 = 1.0 + D2 / D1
                    for i in range(n):
                        for j in range(i + 1):
                            B[i, j] += (D2 * t[i] * t[j] - X[i] * t[j] - t[i] * X[j]) / D1
                else:
                    ilast = gradcount
            else:  # no progress
                if ilast < gradcount:
                    count = 0
                    ilast = gradcount
        else:  # uphill search direction (or NaN): reset B, or stop if it has just been reset
            count = 0
            if ilast == gradcount:
                count = n
            else:
                ilast = gradcount
        if it >= maxit:
            break
        if gradcount - ilast > 2 * n:
            ilast = gradcount  # periodic restart
        if not (count != n or ilast != gradcount):
            break
    return b, fmin, funcount, gradcount, (0 if it < maxit else 1)


def brent_fmin(f, ax, bx, tol):
    """Brent's fmin, the algorithm behind R's optimize() / optim(method = "Brent"): minimum of f on [ax, bx].
    Restated from the published algorithm (Brent 1973, ch. 5; netlib fmin)."""
    c = (3.0 - math.sqrt(5.0)) * 0.5
    eps = math.sqrt(np.finfo(float).eps)
    a, b = ax, bx
    v = a + c * (b - a)
    w = x = v
    d = e = 0.0
    fx = f(x)
    fv = fw = fx
    tol3 = tol / 3.0
    while True:
        xm = (a + b) * 0.5
        tol1 = eps * abs(x) + tol3
        t2 = tol1 * 2.0
        if abs(x - xm) <= t2 - (b - a) * 0.5:
            break
        p = q = r = 0.0
        if abs(e) > tol1:  # fit a parabola
            r = (x - w) * (fx - fv)
            q = (x - v) * (fx - fw)
            p = (x - v) * q - (x - w) * r
            q = (q - r) * 2.0
            if q > 0.0:
                p = -p
            else:
                q = -q
            r = e
            e = d
        if abs(p) >= abs(q * 0.5 * r) or p <= q * (a - x) or p >= q * (b - x):  # golden-section step
            e = (b - x) if x < xm else (a - x)
            d = c * e
        else:  # parabolic-interpolation step
            d = p / q
            u = x + d
            if u - a < t2 or b - u < t2:  # f must not be evaluated too close to a or b
                d = tol1 if x < xm else -tol1
        if abs(d) >= tol1:  # f must not be evaluated too close to x
            u = x + d
        elif d > 0.0:
            u = x + tol1
        else:
            u = x - tol1
        fu = f(u)
        if fu <= fx:
            if u < x:
                b = x
            else:
                a = x
            v, w, x = w, x, u
            fv, fw, fx = fw, fx, fu
        else:
            if u < x:
                a = u
            else:
                b = u
            if fu <= fw or w == x:
                v, fv = w, fw
                w, fw = u, fu
            elif fu <= fv or v == x or v == w:
                v, fv = u, fu
    return x


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
