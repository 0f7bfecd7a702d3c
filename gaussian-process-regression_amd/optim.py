"""The two host optimisers the reference gets from R, restated from their published algorithms: `vmmin` / `vmmin_steps`, Nash's
variable-metric minimiser behind optim(method = "BFGS"), and `brent_fmin`, Brent's fmin behind optimize() / optim(method = "Brent").
Pure numerics on small vectors: nothing here knows of kernels, data or the native library.  fit.py drives them and re-exports them.
"""
from __future__ import annotations

import math

import numpy as np

__all__ = ["vmmin", "vmmin_steps", "brent_fmin"]


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
