"""multivariate_normal() and the numeric half of the posterior-draw plots (reference
R/GPRclass.R:360-376, :190-199).

The factorisation of the covariance -- t(chol(.)), or eigen() when the Cholesky fails, which for a posterior covariance
is the normal case -- and `mean + L %*% Z` run on the MI355X (gprc_mvn_sample).  The standard normal matrix Z is drawn
on the host, as R's rnorm is; pass `z` to supply it, or `rng` (a numpy Generator) to control it.  R's Mersenne-Twister
stream is not reproduced (parity of the draws themselves is unpinned and, through eigen()'s sign freedom, not even
defined); what is pinned is L %*% t(L) = covariance (projected on the PSD cone) and the reference's acceptance rule.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _native as nat
from .covfunc import as_test_points

__all__ = ["multivariate_normal", "expand_range", "mvn_factor", "sym_eigen", "spectral_frequencies", "SamplePaths", "PathMaxima", "maximize_paths"]


def _sq(cov, what="covariance"):
    cov = np.asfortranarray(np.asarray(cov, dtype=np.float64))
    if cov.ndim != 2 or cov.shape[0] != cov.shape[1]:
        raise ValueError(f"{what} must be a square matrix")
    return cov


def sym_eigen(A, *, vectors=True, ctx=None):
    """eigen(A, symmetric = TRUE): (values in decreasing order, vectors as columns or None).  Lower triangle read."""
    A = _sq(A, "A")
    m = A.shape[0]
    ctx = ctx or nat.default_context()
    val = np.empty(m)
    vec = np.empty((m, m), order="F") if vectors else None
    sweeps = C.c_int()
    nat.check(nat.lib().gprc_sym_eigen(ctx.handle, A.ctypes.data, m, m, val.ctypes.data, vec.ctypes.data if vectors else None,
                                       C.byref(sweeps)))
    return val, vec


def mvn_factor(covariance, tol=1e-6, *, ctx=None):
    """(L, method): L = t(chol(covariance)) [method "chol"] or eigen$vectors %*% diag(sqrt(pmax(eigen$values, 0)))
    [method "eigen"]  --  R/GPRclass.R:362-368.  Raises ValueError when an eigenvalue is below -tol * |largest| (:366)."""
    cov = _sq(covariance)
    m = cov.shape[0]
    ctx = ctx or nat.default_context()
    L = np.empty((m, m), order="F")
    method = C.c_int()
    try:
        nat.check(nat.lib().gprc_mvn_factor(ctx.handle, cov.ctypes.data, m, m, float(tol), L.ctypes.data, C.byref(method)))
    except nat.GprcError as e:
        if e.status == nat.ERR_NOT_PD:
            raise ValueError("all(eigval > -tol * abs(eigval[1])) is not TRUE") from e
        raise
    return L, {1: "chol", 2: "eigen"}[method.value]


def multivariate_normal(n, mean, covariance, tol=1e-6, *, z=None, rng=None, ctx=None):
    """multivariate_normal(n, mean, covariance, tol = 1e-6)  --  R/GPRclass.R:360-370.
    Returns a length(mean) x n array, one draw per column: drop(mean) + L %*% matrix(rnorm(n * length(mean)), nrow = length(mean))."""
    cov = _sq(covariance)
    mean = np.ascontiguousarray(np.asarray(mean, dtype=np.float64).ravel())
    m = mean.size
    if m != cov.shape[0]:
        raise ValueError("length(mean) == nrow(covariance) is not TRUE")               # :361
    n = int(n)
    if z is None:
        rng = rng if rng is not None else np.random.default_rng()
        z = rng.standard_normal((n, m)).T                                              # column-major m x n fill order, as matrix(rnorm(.), nrow = m)
    z = np.asfortranarray(np.asarray(z, dtype=np.float64).reshape(m, n))
    ctx = ctx or nat.default_context()
    out = np.empty((m, n), order="F")
    method = C.c_int()
    try:
        nat.check(nat.lib().gprc_mvn_sample(ctx.handle, cov.ctypes.data, m, m, mean.ctypes.data, float(tol), z.ctypes.data, n,
                                            out.ctypes.data, C.byref(method)))
    except nat.GprcError as e:
        if e.status == nat.ERR_NOT_PD:
            raise ValueError("all(eigval > -tol * abs(eigval[1])) is not TRUE") from e
        raise
    return out


def expand_range(x):
    """expand_range(x)  --  R/GPRclass.R:372-376: the range of x widened by 20 % about its midpoint."""
    x = np.asarray(x, dtype=np.float64)
    lo, hi = float(x.min()), float(x.max())
    mid = (lo + hi) / 2.0
    return mid - 1.2 * (mid - lo), mid + 1.2 * (hi - mid)


def spectral_frequencies(k, d, D, rng):
    """Random Fourier frequencies of a stationary kernel: Nu (d x D, column-major, one frequency per column) in CYCLES, nu = omega / (2 pi)
    with omega drawn from the kernel's spectral density, so that E cos(2 pi nu . r) = k(r).  With z ~ N(0, I_d):

        sqrexp (l)                    omega = z / l
        sqrexp_ard (l_1..l_d)         omega_c = z_c / l_c
        matern32, matern52 (+ _ard)   omega = (z / l) sqrt(2 nu / g),   g ~ chi^2(2 nu),  nu = 3/2 or 5/2   (a multivariate t with 2 nu dof)
        rationalquadratic (l, alpha)  omega = (z / l) sqrt(tau),        tau ~ Gamma(shape alpha, scale 1 / alpha)

    gammaexp (an alpha-stable mixture), constant, linear and polynomial (not stationary) raise ValueError.
    Order of the draws, so that a seed reproduces: first rng.standard_normal((D, d)) -- feature by feature, the d coordinates of a feature
    together -- then, for the Matern kernels and rationalquadratic only, the D mixing variables in one call (rng.chisquare(2 nu, D) or
    rng.gamma(alpha, 1 / alpha, D))."""
    kid = k.gprc_kernel[0]
    d, D = int(d), int(D)
    par = np.atleast_1d(np.asarray(k.native_params(d), dtype=np.float64))
    if D < 1:
        raise ValueError("D >= 1 is not TRUE")
    stationary = (nat.SQREXP, nat.SQREXP_ARD, nat.RATQUAD, nat.MATERN32, nat.MATERN52, nat.MATERN32_ARD, nat.MATERN52_ARD)
    if kid == nat.GAMMAEXP:
        raise ValueError("spectral_frequencies: gammaexp's spectral density (an alpha-stable mixture) is not implemented")
    if kid not in stationary:
        raise ValueError("spectral_frequencies: the kernel is not stationary (constant, linear and polynomial have no spectral density)")
    z = rng.standard_normal((D, d))
    l = par if kid in nat.ARD_KERNELS else np.full(d, par[0])
    omega = z / l[None, :]
    if kid in (nat.MATERN32, nat.MATERN32_ARD, nat.MATERN52, nat.MATERN52_ARD):
        dof = 3.0 if kid in (nat.MATERN32, nat.MATERN32_ARD) else 5.0
        omega = omega * np.sqrt(dof / rng.chisquare(dof, D))[:, None]
    elif kid == nat.RATQUAD:
        alpha = par[1]
        omega = omega * np.sqrt(rng.gamma(alpha, 1.0 / alpha, D))[:, None]
    return np.asfortranarray(omega.T / (2.0 * np.pi))


class PathMaxima(NamedTuple):
    """what maximize_paths returns"""
    x_best: np.ndarray    # d x n_paths: the best point of every path
    f_best: np.ndarray    # n_paths: its value, as the evaluator returned it at exactly that point
    x: np.ndarray         # d x (n_paths n_starts): all candidates; candidate q belongs to path q mod n_paths
    f: np.ndarray         # their values under their own path
    pg: np.ndarray        # their projected-gradient norms  max_c |clip(x + g)_c - x_c|
    n_evals: int          # calls of the evaluator


def maximize_paths(eval_grad, lower, upper, n_paths, *, n_starts=16, max_iter=200, gtol=1e-8, x0=None, rng=None):
    """Maximise n_paths functions over the box [lower, upper] (each of length d) by a batched multi-start projected gradient ascent.

    `eval_grad(X)` takes d x m points (Fortran order) and returns (F m x n_paths, dF m x n_paths x d): SamplePaths.paths_grad, or any
    function of that shape (the tests run it on the numpy reference).  There are n_paths * n_starts candidates, candidate q belongs to
    path q mod n_paths, and every iteration is ONE eval_grad call on all candidates, of which each candidate uses its own column.

    Starts: x0 (d x n_paths n_starts) when given; else uniform in the box from `rng`, candidate by candidate.  The first call has then
    evaluated every draw under every path, so a path keeps the better half of its own draws and takes the best other draws under it for
    the rest: no further evaluation, and a path's starts no longer depend on its own luck alone.
    Step: x+ = clip(x + a g) with a Barzilai-Borwein step a = -s.s / s.y where the curvature along the last step is negative (else four
    times the last step), safeguarded by Armijo's condition f+ >= f_ref + 1e-4 g.(x+ - x) up to the rounding of f, with f_ref the
    smallest of the candidate's last five accepted values (Barzilai-Borwein steps are not monotone; against f itself the d = 2 problem
    of the tests left 100 of 256 candidates unconverged after 200 iterations, this way all converge within 90): a rejected candidate
    keeps its point and quarters its step.  A candidate stops when its projected-gradient norm max_c |clip(x + g)_c - x_c| <= gtol;
    one that has not converged at max_iter returns the best point it visited.
    Deterministic for a given rng (or x0).  Returns a PathMaxima."""
    lower = np.atleast_1d(np.asarray(lower, dtype=np.float64)).ravel()
    upper = np.atleast_1d(np.asarray(upper, dtype=np.float64)).ravel()
    d, S, T = lower.size, int(n_paths), int(n_starts)
    if upper.size != d or not (np.isfinite(lower).all() and np.isfinite(upper).all() and (lower < upper).all()):
        raise ValueError("lower and upper must be finite, of one length, lower < upper")
    if S < 1 or T < 1 or int(max_iter) < 0:
        raise ValueError("n_paths >= 1, n_starts >= 1, max_iter >= 0 are not all TRUE")
    Q = S * T
    lo, hi = lower[:, None], upper[:, None]
    qi = np.arange(Q)
    path = qi % S

    def clip(x):
        return np.minimum(np.maximum(x, lo), hi)

    def own(x):
        F, dF = eval_grad(np.asfortranarray(x))
        F, dF = np.asarray(F), np.asarray(dF)
        if F.shape != (Q, S) or dF.shape != (Q, S, d):
            raise ValueError("eval_grad must return (m x n_paths, m x n_paths x d)")
        return F, dF

    if x0 is not None:
        x = clip(np.array(x0, dtype=np.float64).reshape(d, Q))
        F, dF = own(x)
        f, g = F[qi, path].copy(), dF[qi, path, :].T.copy()
    else:
        rng = rng if rng is not None else np.random.default_rng()
        draws = clip(lo + (hi - lo) * rng.random((Q, d)).T)
        F, dF = own(draws)
        pick = qi.copy()                                             # the draw candidate q starts from
        keep = T - T // 2
        for s in range(S):
            mine = qi[path == s]
            mine = mine[np.argsort(-F[mine, s], kind="stable")]      # this path's own draws, best first
            rest = np.argsort(-F[:, s], kind="stable")
            rest = rest[path[rest] != s][:T - keep]                  # the best draws of the other paths under this one
            pick[qi[path == s]] = np.concatenate([mine[:keep], rest, mine[keep:]])[:T]   # (one path: there are no other draws)
        x = draws[:, pick]
        f, g = F[pick, path].copy(), dF[pick, path, :].T.copy()
    n_evals = 1

    def pgnorm(x, g):
        return np.abs(clip(x + g) - x).max(axis=0)

    width = float((upper - lower).min())
    pg = pgnorm(x, g)
    step = 0.05 * width / np.maximum(np.abs(g).max(axis=0), 1e-300)  # the first move is a twentieth of the box
    active = pg > gtol
    eps = 4.0 * np.finfo(np.float64).eps
    hist = np.repeat(f[None, :], 5, axis=0)                          # the last five accepted values: Armijo against their minimum
    xb, fb, gb = x.copy(), f.copy(), g.copy()                        # the best point a candidate has visited
    for _ in range(int(max_iter)):
        if not active.any():
            break
        xt = np.where(active[None, :], clip(x + step[None, :] * g), x)
        F, dF = own(xt)
        n_evals += 1
        ft, gt = F[qi, path], dF[qi, path, :].T
        sv = xt - x
        gain = (g * sv).sum(axis=0)
        fref = hist.min(axis=0)
        ok = active & (ft >= fref + 1e-4 * gain - eps * np.maximum(1.0, np.abs(fref)))
        hist[:, ok] = np.vstack([hist[1:, ok], ft[None, ok]])
        yv = gt - g
        ss, sy = (sv * sv).sum(axis=0), (sv * yv).sum(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            bb = np.where(sy < 0.0, -ss / sy, 4.0 * step)
        step = np.where(ok, bb, np.where(active, 0.25 * step, step))
        x = np.where(ok[None, :], xt, x)
        g = np.where(ok[None, :], gt, g)
        f = np.where(ok, ft, f)
        up = f > fb
        xb, gb, fb = np.where(up[None, :], x, xb), np.where(up[None, :], g, gb), np.where(up, f, fb)
        pg = pgnorm(x, g)
        moved = step * np.abs(g).max(axis=0) > 1e-17 * width        # a step below the spacing of the coordinates cannot move the point
        active = active & (pg > gtol) & moved
    back = (pg > gtol) & (fb > f)                                    # not converged and below an earlier point: that point is returned
    x, g, f = np.where(back[None, :], xb, x), np.where(back[None, :], gb, g), np.where(back, fb, f)
    pg = pgnorm(x, g)
    best = np.array([qi[path == s][np.argmax(f[path == s])] for s in range(S)])
    return PathMaxima(np.asfortranarray(x[:, best]), f[best].copy(), np.asfortranarray(x), f, pg, n_evals)


class SamplePaths(nat.Handle):
    """Posterior sample paths of a fitted GPR (GPR.sample_paths; gprc_gpr_paths_*): n_paths functions that can be evaluated at any points,
    again and again.  They describe the posterior at creation and stay valid after GPR.add_data or GPR.close.  `paths(X_star)` returns
    the n* x n_paths array of their values; `paths_grad(X_star)` the values and their gradients with respect to the points;
    `maximize(lower, upper)` every path's maximiser over a box (maximize_paths); `.weights` the n x n_paths matrix U of the update term;
    `.close()` releases the device memory (also a context manager)."""
    _slot, _free, _closed = "_h", "gprc_gpr_paths_free", "sample paths already closed"

    def __init__(self, model_handle, d, nu, phase, w, e):
        self._h = C.c_void_p()
        self._d = int(d)
        D, S = w.shape
        nat.check(nat.lib().gprc_gpr_paths_create(model_handle, nu.ctypes.data, phase.ctypes.data, D, w.ctypes.data, e.ctypes.data, S,
                                                  C.byref(self._h)))
        self.n, self.n_features, self.n_paths = e.shape[0], D, S

    def paths(self, X_star):
        """f_s(X_star[, i]) as an n* x n_paths array; X_star as GPR.predict takes it"""
        Xs = as_test_points(X_star, self._d)
        ns = Xs.shape[1]
        out = np.empty((ns, self.n_paths), order="F")
        nat.check(nat.lib().gprc_gpr_paths_eval(self.handle, Xs.ctypes.data, ns, out.ctypes.data, ns))
        return out

    def paths_grad(self, X_star):
        """(F, dF): the values f_s(X_star[, i]) as `paths` returns them (the same bits), n* x n_paths, and their gradients with respect
        to the point, dF[i, s, c] = d f_s / d x_c, n* x n_paths x d; both in Fortran order (gprc_gpr_paths_eval_grad)"""
        Xs = as_test_points(X_star, self._d)
        ns = Xs.shape[1]
        F = np.empty((ns, self.n_paths), order="F")
        dF = np.empty((ns, self.n_paths, self._d), order="F")
        nat.check(nat.lib().gprc_gpr_paths_eval_grad(self.handle, Xs.ctypes.data, ns, F.ctypes.data, ns, dF.ctypes.data, ns))
        return F, dF

    def maximize(self, lower, upper, **kw):
        """maximize_paths over these paths on the device: every iteration is one paths_grad call on all candidates"""
        return maximize_paths(self.paths_grad, lower, upper, self.n_paths, **kw)

    @property
    def weights(self):
        U = np.empty((self.n, self.n_paths), order="F")
        nat.check(nat.lib().gprc_gpr_paths_get_weights(self.handle, U.ctypes.data))
        return U
