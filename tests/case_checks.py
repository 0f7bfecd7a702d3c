"""The checks that run for every kernel but are called from more than one test file, with their case tables, each written once.  The
Matern kernels' cases keep the test names and ids they have had since they arrived (tests/test_matern_cpu.py, tests/test_gpu_matern.py);
the other kernels' cases run in tests/test_pred_grad_cpu.py, tests/test_gpu_ard_grad.py and tests/test_gpu_gpc_grad.py.  Where two
families differ, a column of the case table or the case itself decides -- never the file that calls.  A plain module: importing it needs
no GPU; the functions of sections 2 and 3 do."""
import numpy as np

import ard_grad_ref
import gpc_grad_ref
import kernel_ref as K
import pred_grad_ref as G
from conftest import TOL, nerr
from gprc_amd import GPC
from gprc_amd import _native as nat
from gprc_amd.fit import dens, grad_dict, logp_grad
from gpu_calls import EPS, gpc_problem, grad_problem, kfun, raw_logq_grad
from oracle import oracle as orc

LD = np.longdouble

# ---- 1. the prediction-gradient reference judges itself (CPU) -----------------------------------------------------------------
_CACHE = {}


def outputs(case, size):
    """float64 and longdouble (mean, var, dmean, dvar) and the longdouble factor, once per (case, size)"""
    key = (K.case_id(case), size)
    if key not in _CACHE:
        name, par, d = case
        n, noise = size
        X, y, Xs = G.make_case(case, n)
        f64 = G.predict_grad(name, par, X, y, noise, Xs, np.float64)
        fac = G.fit(name, par, X, y, noise, LD)
        ld = G.predict_grad(name, par, X, y, noise, Xs, LD, factor=fac)
        _CACHE[key] = (X, y, Xs, f64, ld, fac)
    return _CACHE[key]


def check_float64_reference_against_longdouble(case, size):
    X, _, _, f64, ld, _ = outputs(case, size)
    if case[0] in K.MATERN_NAMES:
        cond = np.linalg.cond(K.kernel(case[0], case[1], X) + size[1] * np.eye(size[0]))
        print(K.case_id(case), size, "cond(K_y) %.3g" % cond)
        assert cond <= 1.1e4
    for what, a, b in zip(("mean", "var", "dmean", "dvar"), f64, ld):
        e = G.nerr(np.asarray(a, dtype=LD), b)
        print(K.case_id(case), size, what, "%.2e" % e)
        assert e <= 1e-11, (what, e)


def check_gradients_against_central_differences(case, size):
    name, par, d = case
    X, _, Xs, _, ld, (L, alpha) = outputs(case, size)
    h = LD(1e-6)
    keep = np.ones(Xs.shape[1], dtype=bool)                  # every test point, x*_0 = x_5 included ...
    if name == "gammaexp" and par[1] <= 1.0:
        keep[0] = False                                   # ... but here: not differentiable there
    dm, dv = np.empty((d, Xs.shape[1]), dtype=LD), np.empty((d, Xs.shape[1]), dtype=LD)
    Xl = np.asarray(X, dtype=LD)
    for c in range(d):
        up, dn = np.asarray(Xs, dtype=LD).copy(), np.asarray(Xs, dtype=LD).copy()
        up[c] += h
        dn[c] -= h
        mu, vu = G.mean_var(name, par, Xl, L, alpha, up, LD)
        md, vd = G.mean_var(name, par, Xl, L, alpha, dn, LD)
        dm[c], dv[c] = (mu - md) / (2 * h), (vu - vd) / (2 * h)
    for what, a, b in (("dmean", ld[2], dm), ("dvar", ld[3], dv)):
        e = G.nerr(b[:, keep], a[:, keep])
        print(K.case_id(case), size, what, "%.2e" % e)
        assert e <= 1e-8, (what, e)


# ---- 2. gprc_gpr_logp_grad against the closed form (GPU) ------------------------------------------------------------------------
# name -> (kernel, parameters (None: the d length scales of grad_problem), d, oracle, block):
#   oracle  the oracle fit that must succeed at the first attempt: "same" (its own kernel of that name), "scaled" (its isotropic squared
#           exponential on X / l), None (no such kernel: numpy's Cholesky raising is the precondition)
#   block   the parameter block is also bounded on its own (the noise entry dominates the norm of the whole vector)
# d > 16: the contraction stages the coordinates 16 at a time, so d = 17 takes two passes and d = 33 three, the last of one coordinate
# each, and ARD stages them again for its second pass.  The length scales are multiplied by sqrt(d / 3): at the scales of d = 3 the
# kernel matrix of 17 coordinates is nearly the identity, the length-scale gradient is ~1e-2 of the noise derivative and a normwise
# bound over the whole vector would hide a wrong coordinate.  With the scaling (numpy reference, ard17, n = 300, noise 0.1):
# max |d/dl| = 1.39, min |d/dl| = 0.018, d/dnoise = -28.9.
LOGP_CASES = {
    "sqrexp": ("sqrexp", [1.3], 3, "same", False), "gammaexp1.5": ("gammaexp", [0.9, 1.5], 3, "same", False),
    "gammaexp1": ("gammaexp", [1.2, 1.0], 3, "same", False), "ratquad": ("rationalquadratic", [1.1, 1.7], 3, "same", False),
    "ard3": ("sqrexp_ard", None, 3, "scaled", False), "ard8": ("sqrexp_ard", None, 8, "scaled", False),
    "ard17": ("sqrexp_ard", None, 17, "scaled", True), "sqrexp_d17": ("sqrexp", [1.3], 17, "same", True),
    "ard33": ("sqrexp_ard", None, 33, "scaled", True),
    "matern32": ("matern32", [0.9], 3, None, True), "matern52": ("matern52", [1.1], 3, None, True),
    "matern32_ard": ("matern32_ard", None, 3, None, True), "matern52_ard": ("matern52_ard", None, 3, None, True),
    "matern52_ard8": ("matern52_ard", None, 8, None, True), "matern32_ard17": ("matern32_ard", None, 17, None, True),
    "matern52_ard17": ("matern52_ard", None, 17, None, True),
}


def logp_case(case, n):
    """(name, theta, X, y, oracle fit's (kernel id, parameters, inputs) or None) of a named case at size n"""
    name, theta, d, oracle, _ = LOGP_CASES[case]
    X, y, ell = grad_problem(n, d)
    theta = ell if theta is None else np.array(theta)
    if d > 16:
        theta = theta * np.sqrt(d / 3)
    if oracle == "same":
        return name, theta, X, y, (orc.KERNEL_IDS[name], list(theta), X)
    if oracle == "scaled":
        return name, theta, X, y, (orc.SQREXP, [1.0], X / theta[:, None])
    return name, theta, X, y, None


def check_logp_grad_against_the_closed_form(case, n, noise):
    name, theta, X, y, oracle_fit = logp_case(case, n)
    if oracle_fit is not None:
        kid, opar, Xo = oracle_fit
        assert orc.gpr_fit(kid, opar, Xo, y, noise)["attempts"] == 1
    want_logp, want = ard_grad_ref.logp_grad(name, theta, X, y, noise)           # numpy's Cholesky of K_y as it stands
    logp, grad = logp_grad(X, y, noise, name, theta)
    assert grad.shape == (theta.size + 1,)
    e = nerr(grad, want)
    print(f"logp_grad {case} n={n} noise={noise}: nerr(grad)={e:.3e} rel(logp)={abs(logp - want_logp) / abs(want_logp):.3e}")
    assert e <= TOL
    if LOGP_CASES[case][4]:
        eb = nerr(grad[:-1], want[:-1])
        print(f"logp_grad {case} n={n}: nerr(parameter block)={eb:.3e} max|d/dtheta|={np.abs(want[:-1]).max():.3g} "
              f"min|d/dtheta|={np.abs(want[:-1]).min():.3g} d/dnoise={want[-1]:.3g}")
        assert eb <= TOL
    assert abs(logp - want_logp) <= TOL * abs(want_logp)
    assert logp == dens(X, y, noise, name, theta)          # the value is the existing objective, bit for bit


# ---- 3. gprc_gpc_logq_grad: cases, reference, the tie to the fitted classifier (GPU) ------------------------------------------------
LOGQ_CASES = {"sqrexp": ("sqrexp", [0.8], 3), "gammaexp1.5": ("gammaexp", [0.9, 1.5], 3), "gammaexp1": ("gammaexp", [1.2, 1.0], 3),
              "ratquad": ("rationalquadratic", [1.1, 1.7], 3), "ard3": ("sqrexp_ard", [0.8, 1.1, 1.9], 3),
              "ard8": ("sqrexp_ard", np.linspace(1.0, 3.0, 8), 8)}
# d > 16: the contraction stages the coordinates 16 at a time, so d = 17 takes two passes and d = 33 three, the last of one coordinate
# each, and ARD stages them again for its second pass.  The length scales are multiplied by sqrt(d / 3): at the scales of d = 3 the
# kernel matrix of 17 coordinates is nearly the identity.  The gradient has no noise entry here: the whole vector is the parameter
# block, and the normwise bound is on it.
LOGQ_WIDE_CASES = {"ard17": ("sqrexp_ard", np.linspace(1.0, 3.0, 17) * np.sqrt(17 / 3), 17), "sqrexp_d17": ("sqrexp", [0.8 * np.sqrt(17 / 3)], 17),
                   "ard33": ("sqrexp_ard", np.linspace(1.0, 3.0, 33) * np.sqrt(33 / 3), 33)}
# the Matern kernels run at n = 600 and 1100 (d = 3) and, scaled as above, at d = 17
LOGQ_MATERN_CASES = {"matern32": ("matern32", [0.8], 3), "matern52": ("matern52", [0.9], 3), "matern32_ard": ("matern32_ard", [0.8, 1.1, 1.9], 3),
                     "matern52_ard": ("matern52_ard", [0.8, 1.1, 1.9], 3)}
LOGQ_MATERN_WIDE = {"matern52_ard17": ("matern52_ard", np.linspace(1.0, 3.0, 17) * np.sqrt(17 / 3), 17), "matern32_d17": ("matern32", [0.8 * np.sqrt(17 / 3)], 17)}
LOGQ_ALL = {**LOGQ_CASES, **LOGQ_WIDE_CASES, **LOGQ_MATERN_CASES, **LOGQ_MATERN_WIDE}


def logq_case(case, n):
    name, theta, d = LOGQ_ALL[case]
    X, y = gpc_problem(n, d)
    return name, np.asarray(theta, dtype=float), X, y


def logq_reference(name, theta, X, y):
    """the numpy reference, with the two preconditions on it that make the comparison meaningful"""
    want_logq, want, iters, decrements = gpc_grad_ref.logq_grad(name, theta, X, y, EPS)
    assert iters < 50
    assert not any(EPS / 1.2 <= dcr <= 1.2 * EPS for dcr in decrements), decrements
    return want_logq, want, iters


def check_value_is_tied_to_the_fitted_classifier(case, n):
    """logq = GPC$logq + sum(diag(L)) - sum(log(diag(L))): the same mode search through the shared fills"""
    name, theta, X, y = logq_case(case, n)
    Xf = np.asfortranarray(X)                                      # kept alive: the call borrows its memory
    logq, _, iters = raw_logq_grad(grad_dict[name].kernel_id, theta, Xf.ctypes.data, X.shape[0], n, y.ctypes.data, nat.default_context())
    gc = GPC(X, y, kfun(name, theta), EPS, reference_stop=False)
    dl = np.diag(gc.L)
    want = gc.logq + dl.sum() - np.log(dl).sum()
    print(f"logq_grad {case} n={n}: logq={logq!r} from the classifier {want!r} iterations {gc.iterations} / {iters}")
    assert gc.iterations == iters
    assert abs(logq - want) <= TOL * abs(want)
    gc.close()
