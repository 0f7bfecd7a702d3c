"""What the GPU test files share: the time limit of a step, a kernel object for any of fit.grad_dict's names, the raw C-ABI calls
of the three gradients, and the random problems of the evidence-gradient tests.  A plain module: a test file imports `step_time_limit`
by name so that pytest finds the autouse fixture in that file's namespace.  Importing it needs no GPU: the CPU tests of the
references (tests/test_matern_cpu.py, tests/test_gpc_grad_cpu.py) and tests/case_checks.py take the random problems from here, so
that the references are judged on the very inputs the GPU tests use, and do not import the fixture."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

from gprc_amd import _native as nat
from gprc_amd.fit import _func_of

STEP_LIMIT_S = 900   # a hung step ends the process (with every thread's traceback) instead of holding the GPU
EPS = 1e-10          # the mode search's epsilon of every Laplace-evidence test


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def kfun(name, par):
    """the kernel object of a name of fit.grad_dict, parameters in the ABI's order"""
    return _func_of(name, tuple(float(v) for v in np.atleast_1d(par)))


def raw_logp_grad(kid, theta, Xptr, d, n, yptr, noise, ctx):
    _, pp, npar = nat.params_array(theta)
    g, lp = np.empty(npar + 1), C.c_double()
    nat.check(nat.lib().gprc_gpr_logp_grad(ctx.handle, kid, pp, npar, Xptr, d, n, yptr, noise, C.byref(lp), g.ctypes.data_as(C.POINTER(C.c_double))))
    return lp.value, g


def raw_logq_grad(kid, theta, Xptr, d, n, yptr, ctx, epsilon=EPS, max_iter=0):
    _, pp, npar = nat.params_array(theta)
    g, lq, it = np.empty(npar), C.c_double(), C.c_int()
    nat.check(nat.lib().gprc_gpc_logq_grad(ctx.handle, kid, pp, npar, Xptr, d, n, yptr, epsilon, max_iter, C.byref(lq),
                                           g.ctypes.data_as(C.POINTER(C.c_double)), C.byref(it)))
    return lq.value, g, it.value


def call_predict_grad(g, Xs, mean=True, var=True, dmean=True, dvar=True):
    """gprc_gpr_predict_grad with host pointers; an output not asked for is passed as NULL and returned as None"""
    d, ns = Xs.shape
    Xs = np.asfortranarray(Xs)
    out = [np.full(ns, np.nan) if mean else None, np.full(ns, np.nan) if var else None,
           np.full((d, ns), np.nan, order="F") if dmean else None, np.full((d, ns), np.nan, order="F") if dvar else None]
    nat.check(nat.lib().gprc_gpr_predict_grad(g._model, Xs.ctypes.data, ns, *[o.ctypes.data if o is not None else None for o in out]))
    return out


def same_bits(a, b):
    """two lists of outputs (arrays, scalars, None for an output not asked for) are equal entry by entry, bit for bit"""
    return all((x is None and y is None) or np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def grad_problem(n, d):
    """(X, y, d length scales) of the marginal-likelihood gradient tests"""
    rng = np.random.default_rng(1000 + n + d)
    X = rng.uniform(-2, 2, (d, n))
    y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
    return X, y, rng.uniform(0.7, 2.0, d)


def gpc_problem(n, d):
    """(X, y) of the Laplace-evidence tests, y in {-1, +1}"""
    rng = np.random.default_rng(7000 + n + d)
    X = rng.uniform(-1, 1, (d, n))
    y = np.sign(X[0] - 0.5 * X[d - 1] + 0.3 * rng.normal(size=n))
    y[y == 0] = 1.0
    return X, y
