"""The references of the batched and the local classifier judge themselves, on the inputs the GPU tests use (tests/batch_gpc_ref.py), and
the argument errors of gprc_gpc_batch_fit that need no device.  No GPU.

Worst figures of a run here (numpy model against the tightly converged reference).  The batch sizes: f_hat 2.9e-14, latent mean 4.9e-14,
variance 1.2e-14 relative, probability 2.5e-14, logq 5.3e-16; iterations 3 (n_b = 1, 2) .. 5 (127, 128).  The local models: latent mean
4.8e-13 absolute, variance 6.0e-14 relative, probability 6.0e-14; iterations 3 .. 7; single-class neighbourhoods 37 of 37 at m = 1,
9 .. 12 at m = 17.  Against the oracle at n = 100: 3.7e-15 at most, the same 5 iterations."""
import numpy as np
import pytest
from scipy.linalg import solve_triangular

import batch_gpc_ref as G
from gprc_amd import _native as nat
from gprc_amd.fit import grad_dict
from oracle import oracle as orc

MODEL_TOL = 1e-11   # the numpy model (the loop stopped at EPS) against the tightly converged reference


def _check_model(st, ref, what):
    worst = dict(f=np.abs(st["f"] - ref["f"]).max() / max(np.abs(ref["f"]).max(), 1e-300), fs=np.abs(st["fs"] - ref["fs"]).max() / np.abs(ref["fs"]).max(),
                 vf=G.var_err(st["vf"], ref["vf"]), prob=np.abs(st["prob"] - ref["prob"]).max(),
                 logq=abs(st["logq"] - ref["logq"]) / max(1.0, abs(ref["logq"])))
    print(what, {k: "%.2e" % v for k, v in worst.items()}, "iterations", st["iters"], ref["iters"])
    assert st["info"] == 0
    assert all(v <= MODEL_TOL for v in worst.values()), worst
    assert st["iters"] == ref["iters"] <= 10
    return worst


@pytest.mark.parametrize("case", list(G.CASES))
def test_numpy_model_reaches_the_converged_mode_at_every_batch_size(case):
    for nb in G.SIZES:
        _check_model(G.batch_model(case, nb), G.batch_reference(case, nb), f"{case} n_b={nb}")


def test_the_batch_holds_models_of_different_iteration_counts():
    for case in G.CASES:
        assert G.batch_reference(case, 1)["iters"] == 3
        assert G.batch_reference(case, 128)["iters"] >= 5


@pytest.mark.parametrize("m", G.LOCAL_MS)
@pytest.mark.parametrize("case", list(G.CASES))
def test_numpy_model_reaches_the_converged_mode_of_every_local_model(case, m):
    ref, mod = G.local_reference(case, m), G.local_reference(case, m, model=True)
    worst = dict(fs=np.abs(mod["fs"] - ref["fs"]).max(), vf=G.var_err(mod["vf"], ref["vf"]), prob=np.abs(mod["prob"] - ref["prob"]).max())
    print(case, m, {k: "%.2e" % v for k, v in worst.items()}, "iterations", ref["iters"].min(), "..", ref["iters"].max(), "single-class", ref["single_class"])
    assert all(v <= MODEL_TOL for v in worst.values()), worst
    assert 3 <= ref["iters"].min() and ref["iters"].max() <= 10
    assert np.array_equal(mod["iters"], ref["iters"])
    assert (ref["vf"] > 0).all()
    if m == 1:
        assert ref["single_class"] == G.NS        # one point is one class: the neighbourhoods of a single label are part of the test


@pytest.mark.parametrize("case", list(G.CASES))
def test_prediction_through_wt_is_the_substitution(case):
    name, theta, X, y, Xs = G.case_data(case)
    for nb in (17, 128):
        st = G.batch_model(case, nb)
        Ks = G.kmat(name, theta, X[:, :nb], Xs)
        v = solve_triangular(st["L"], st["sw"][:, None] * Ks, lower=True)
        assert np.abs(st["Wt"] @ Ks - v).max() <= 1e-14 * nb
        assert np.array_equal(np.triu(st["Wt"], 1), np.zeros((nb, nb)))
        fs, vf = G.predict_by_substitution(st, Ks)
        assert np.abs(fs - st["fs"]).max() <= 1e-14 and G.var_err(st["vf"], vf) <= 1e-13


def test_class_probability_quadrature_against_closed_cases():
    # fs = 0: the integrand's odd part vanishes, P = 1/2 for any sd; sd -> 0: P -> sigmoid(fs)
    assert np.abs(G.class_prob(np.zeros(3), [0.05, 0.5, 1.0]) - 0.5).max() <= 1e-15
    assert abs(G.class_prob([0.7], [1e-9])[0] - G.GR.sigmoid(0.7)) <= 1e-15
    # and against a rule of another kind: Gauss-Hermite with 120 nodes
    x, w = np.polynomial.hermite_e.hermegauss(120)
    fs, vf = np.array([-2.3, 0.4, 1.9]), np.array([0.9, 0.3, 0.6])
    gh = (G.GR.sigmoid(fs[:, None] + vf[:, None] * x[None, :]) * w[None, :]).sum(1) / np.sqrt(2 * np.pi)
    assert np.abs(G.class_prob(fs, vf) - gh).max() <= 1e-13


# the oracle has the reference's kernels: the isotropic cases as they are, sqrexp_ard as its squared exponential on X / l; it has no Matern
ORACLE_CASES = {"sqrexp": None, "gammaexp1.5": None, "ratquad": None, "ard3": "scaled"}


@pytest.mark.parametrize("case", list(ORACLE_CASES))
def test_against_the_oracle(case):
    name, theta, X, y, Xs = G.case_data(case)
    n = 100
    X, y = X[:, :n], y[:n]
    if ORACLE_CASES[case] == "scaled":
        kid, par, Xo, Xso = orc.SQREXP, [1.0], X / theta[:, None], Xs / theta[:, None]
    else:
        kid, par, Xo, Xso = orc.KERNEL_IDS[name], list(theta), X, Xs
    fit = orc.gpc_fit(kid, par, Xo, y, epsilon=G.EPS, divergence_stop=False)
    ofs, ovf = orc.gpc_predict_latent(kid, par, Xo, y, fit["f_hat"], fit["L"], Xso)
    st = G.numpy_model(name, theta, X, y, Xs)
    worst = dict(f=np.abs(st["f"] - fit["f_hat"]).max() / np.abs(fit["f_hat"]).max(), fs=np.abs(st["fs"] - ofs).max() / np.abs(ofs).max(), vf=G.var_err(st["vf"], ovf))
    print(case, {k: "%.2e" % v for k, v in worst.items()}, "iterations", st["iters"], fit["iters"])
    assert all(v <= MODEL_TOL for v in worst.values()), worst
    assert abs(st["iters"] - fit["iters"]) <= 1


# ---- argument errors that need no device: gprc_gpc_batch_fit judges its arguments before it looks at the context -------------------------
def _fit_error(expect, **kw):
    rng = np.random.default_rng(3)
    d, n = 2, 5
    args = dict(null_ctx=True, name="sqrexp", thetas=[[0.8], [0.9]], X=G.flat(rng.normal(size=(d, n))), d=d, n_max=n, y=np.ones(n))
    args.update(kw)
    rc, h, *_ = G.call_fit(**args)
    assert rc == nat.ERR_ARG and not h
    assert expect in nat.last_error(), nat.last_error()


def test_argument_errors_without_a_device():
    _fit_error("null context")                                   # everything else is in order: only then is the context asked for
    _fit_error("epsilon", epsilon=0.0)
    _fit_error("epsilon", epsilon=-1e-12)
    _fit_error("epsilon", epsilon=float("nan"))
    _fit_error("max_iter", max_iter=1001)
    _fit_error("null context", max_iter=1000)
    _fit_error("n_max = 129", n_max=129, X=np.zeros(2 * 129), y=np.ones(129))
    _fit_error("n_max < 1", n_max=0)
    _fit_error("defined for", name=nat.LINEAR)
    _fit_error("defined for", name=99)
    _fit_error("null input pointer", X=None)
    _fit_error("null input pointer", y=None)
    _fit_error("null output pointer", model=False)
    _fit_error("null output pointer", logq=False)
    _fit_error("null output pointer", info=False)
    _fit_error("null context", iters=False)                      # iters_out may be NULL
    _fit_error("x_stride", x_stride=9)
    _fit_error("y_stride", y_stride=4)
    _fit_error("n_each", n_each=[5, 6], x_stride=10, y_stride=5)
    _fit_error("n_each", n_each=[0, 5], x_stride=10, y_stride=5)


def test_batch_gpc_checks_its_labels_before_any_native_call():
    from gprc_amd import BatchGPC, LocalGPC, cov_func, sqrexp
    X = np.random.default_rng(5).normal(size=(2, 6))
    with pytest.raises(ValueError, match="labels"):
        BatchGPC(X, [1, -1, 0, 1, 1, -1], "sqrexp", [[0.8]])
    with pytest.raises(ValueError, match="labels"):
        BatchGPC([X, X[:, :4]], [np.ones(6), [1, -1, 2, 1]], "sqrexp", [[0.8], [0.9]])
    with pytest.raises(ValueError, match="labels"):
        LocalGPC(X, [1, -1, 0.5, 1, 1, -1], cov_func(sqrexp, l=0.8))
    assert sorted(grad_dict) and BatchGPC._free == "gprc_batch_model_free" and LocalGPC._free == "gprc_lgpr_free"
