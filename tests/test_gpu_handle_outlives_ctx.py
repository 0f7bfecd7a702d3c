"""Every native handle type may outlive its context (a host language's garbage collector finalises in any order): a use then says so,
the free succeeds and hands no block to the dead context's pool, and the next context works.  Through ctypes on the raw library, one
case per handle type at n = 16, d = 2; the local model has had a gprc_lgpr_vecchia_prepare, so that it owns its neighbour table too."""
import ctypes as C

import numpy as np
import pytest

from gprc_amd import _native as nat
from gpu_calls import step_time_limit  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu

N, D_IN = 16, 2
RNG = np.random.default_rng(16)
X = np.ascontiguousarray(RNG.uniform(-1, 1, (N, D_IN)))        # d x n, column-major
Y = np.sin(X.sum(1)) + 0.1 * RNG.normal(size=N)
XS = np.ascontiguousarray(RNG.uniform(-1, 1, (3, D_IN)))
NOISE = 0.1
THETA, PP, NPAR = nat.params_array([0.8])                            # PP points into THETA


def gpr_fit(ctx):
    h = C.c_void_p()
    rc = nat.lib().gprc_gpr_fit(ctx.handle, nat.SQREXP, PP, NPAR, X.ctypes.data, D_IN, N, Y.ctypes.data, NOISE, C.byref(h))
    assert rc == nat.OK, nat.last_error()
    return h


def make_model(ctx):
    return gpr_fit(ctx)


def use_model(h):
    mean, var, score = np.full(N, np.nan), np.full(N, np.nan), C.c_double(np.nan)
    return nat.lib().gprc_gpr_loo(h, mean.ctypes.data, var.ctypes.data, None, C.byref(score)), [mean, var, score.value]


def make_paths(ctx, feats=8, S=2):
    g, h = gpr_fit(ctx), C.c_void_p()
    nu, phase = RNG.standard_normal((feats, D_IN)), RNG.uniform(0, 1, feats)             # d x D
    W, E = RNG.standard_normal((S, feats)), RNG.standard_normal((S, N))                   # D x S, n x S
    rc = nat.lib().gprc_gpr_paths_create(g, nu.ctypes.data, phase.ctypes.data, feats, W.ctypes.data, E.ctypes.data, S, C.byref(h))
    assert rc == nat.OK, nat.last_error()
    assert nat.lib().gprc_model_free(g) == nat.OK                                         # the paths are what is kept
    return h


def use_paths(h, S=2):
    out = np.full((S, len(XS)), np.nan)                                                   # n* x S
    return nat.lib().gprc_gpr_paths_eval(h, XS.ctypes.data, len(XS), out.ctypes.data, len(XS)), [out]


def make_batch(ctx, B=2):
    h, theta, noise = C.c_void_p(), np.array([0.8, 1.2]), np.full(B, NOISE)
    logp, info = np.full(B, np.nan), np.full(B, -1, dtype=np.intc)
    rc = nat.lib().gprc_gpr_batch_fit(ctx.handle, nat.SQREXP, B, theta.ctypes.data, 1, 1, noise.ctypes.data, X.ctypes.data, D_IN, N, 0, Y.ctypes.data, 0, None,
                                      C.byref(h), logp.ctypes.data, info.ctypes.data)
    assert rc == nat.OK and not info.any() and np.isfinite(logp).all(), nat.last_error()
    return h


def use_batch(h, B=2):
    alpha = np.full((B, N), np.nan)
    return nat.lib().gprc_gpr_batch_get_alpha(h, alpha.ctypes.data), [alpha]


def make_local(ctx):
    h = C.c_void_p()
    rc = nat.lib().gprc_lgpr_create(ctx.handle, nat.SQREXP, PP, NPAR, X.ctypes.data, D_IN, N, Y.ctypes.data, NOISE, 4, C.byref(h))
    assert rc == nat.OK, nat.last_error()
    assert nat.lib().gprc_lgpr_vecchia_prepare(h, 3) == nat.OK, nat.last_error()
    return h


def use_local(h):
    mean, var = np.full(len(XS), np.nan), np.full(len(XS), np.nan)
    return nat.lib().gprc_lgpr_predict(h, XS.ctypes.data, len(XS), mean.ctypes.data, var.ctypes.data, None), [mean, var]


# handle type -> (create on a context, one use: (status, outputs), its free, what a use says once the context is gone)
CASES = {
    "gprc_model": (make_model, use_model, "gprc_model_free", "loo: the model's context has been destroyed"),
    "gprc_paths": (make_paths, use_paths, "gprc_gpr_paths_free", "paths_eval: the context of the paths has been destroyed"),
    "gprc_batch_model": (make_batch, use_batch, "gprc_batch_model_free", "batch_get_alpha: the model's context has been destroyed"),
    "gprc_local_model": (make_local, use_local, "gprc_lgpr_free", "lgpr_predict: the model's context has been destroyed"),
}


@pytest.mark.parametrize("kind", list(CASES))
def test_a_handle_outlives_its_context(kind):
    make, use, free, gone = CASES[kind]
    own = nat.Context(0)
    h = make(own)
    rc, outs = use(h)
    assert rc == nat.OK, nat.last_error()
    assert all(np.isfinite(o).all() for o in outs)
    own.close()
    rc, _ = use(h)
    assert rc == nat.ERR_ARG and nat.last_error() == gone
    assert getattr(nat.lib(), free)(h) == nat.OK
    with nat.Context(0) as fresh:                                                         # the freed blocks did not land in a dead pool
        g, logp = gpr_fit(fresh), C.c_double(np.nan)
        assert nat.lib().gprc_gpr_get_logp(g, C.byref(logp)) == nat.OK and np.isfinite(logp.value)
        assert nat.lib().gprc_model_free(g) == nat.OK
