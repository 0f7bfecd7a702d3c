"""gprc_gpr_predict_grad / GPR.predict_grad on the MI355X against tests/pred_grad_ref.py (float64; itself within 1.6e-13 of the
longdouble formulas, tests/test_pred_grad_cpu.py), normwise TOL = 1e-10 on each of mean, variance and the two gradients; the mean and
the variance are also the very bits of gprc_gpr_predict.  (The Matern kernels: tests/test_gpu_matern.py, against the longdouble reference.)
Geometry: n = 1, 512 (no padding, one panel), 700 (padding of 324 columns: not
a multiple of 128), 1100 (three panels); n* = 1, 129, 300; d = 1, 3, 8 and 17 (two passes over the coordinates, three coordinate groups).
Then what must not change the bits (chunking, the solve's schedule, where the pointers live, which outputs are asked for), the reversed
factor's life (built on demand, dropped by add_data), the refusals, and a loose cross-check against differences of GPR.predict."""
import numpy as np
import pytest

from conftest import TOL
from gprc_amd import GPR, GPC, cov_func, polynomial, sqrexp
from gprc_amd import _native as nat
from gpu_calls import call_predict_grad as call, kfun, same_bits, step_time_limit  # noqa: F401  (the autouse fixture)
import kernel_ref as K
import pred_grad_ref as G

pytestmark = pytest.mark.gpu

NOISE = 0.1
SQ3, SQ8, ARD3, GE15, GE10, RQ = K.BASE_CASES[:6]


def check_against_reference(case, n, ns, at_training_point=None):
    name, par, d = case
    X, y, Xs = G.make_case(case, n, m=ns, at_training_point=at_training_point)
    g = GPR(X, y, NOISE, kfun(name, par))
    got = call(g, Xs)
    ref = G.predict_grad(name, par, X, y, NOISE, Xs)
    for what, a, b in zip(("mean", "var", "dmean", "dvar"), got, ref):
        e = G.nerr(a, b)
        print("%s n %d n* %d %s %.2e" % (K.case_id(case), n, ns, what, e))
        assert np.isfinite(a).all() and e <= TOL, (what, e)
    pred = g.predict(Xs)
    assert np.array_equal(got[0], pred[:, 0]) and np.array_equal(got[1], pred[:, 1])    # the bits of gprc_gpr_predict(pointwise = 1)
    g.close()
    return got


@pytest.mark.parametrize("case", K.BASE_CASES, ids=K.case_id)
def test_every_kernel_against_the_reference(case):
    check_against_reference(case, 700, 129)


@pytest.mark.parametrize("n,ns", [(512, 1), (512, 300), (1100, 1), (1100, 300), (700, 300)])
def test_geometry_against_the_reference(n, ns):
    check_against_reference(SQ3, n, ns)


@pytest.mark.parametrize("d", [1, 17])
@pytest.mark.parametrize("name", ["sqrexp", "sqrexp_ard"])
def test_one_and_seventeen_coordinates(name, d):
    par = [1.1] if name == "sqrexp" else list(np.linspace(0.8, 2.4, d))
    if d == 17 and name == "sqrexp":
        par = [2.5]                                       # points of [-2, 2]^17 are far apart
    check_against_reference((name, par, d), 700, 129)


@pytest.mark.parametrize("case", [SQ3, GE15], ids=K.case_id)
def test_one_training_point_one_test_point_far_apart(case):
    name, par, d = case
    X, y, Xs = np.zeros((d, 1), order="F"), np.array([1.3]), np.full((d, 1), 1.5, order="F")
    g = GPR(X, y, NOISE, kfun(name, par))
    got = call(g, Xs)
    ref = G.predict_grad(name, par, X, y, NOISE, Xs)
    for a, b in zip(got, ref):
        assert G.nerr(a, b) <= TOL
    assert np.abs(ref[2]).max() > 0 and np.abs(ref[3]).max() > 0


def test_gammaexp_at_a_training_point_takes_h_zero():
    """x*_0 = x_5, gamma = 1.5: the pair contributes 0 (the limit) -- a NaN or an Inf from 0 / 0 or log 0 would show"""
    got = check_against_reference(GE15, 700, 129, at_training_point=5)
    assert np.isfinite(got[2][:, 0]).all() and np.isfinite(got[3][:, 0]).all()


def test_chunked_call_is_bitwise_chunk_invariant(monkeypatch):
    name, par, d = SQ3
    X, y, Xs = G.make_case(SQ3, 700, m=600, at_training_point=None)
    g = GPR(X, y, NOISE, kfun(name, par))
    whole = call(g, Xs)
    monkeypatch.setenv("GPRC_CHUNK_BYTES", str(256 * 1024 * 8))   # 256 rows per chunk at n_pad = 1024
    ctx2 = nat.Context(0)
    g2 = GPR(X, y, NOISE, kfun(name, par), ctx=ctx2)
    parts = call(g2, Xs)
    assert same_bits(whole, parts)
    assert same_bits(call(g2, Xs, mean=False, var=False, dvar=False)[2:3], whole[2:3])   # the mean's gradient alone, chunked too
    g2.close()
    ctx2.close()
    g.close()


def test_solve_schedules_give_the_same_bits(monkeypatch):
    name, par, d = RQ
    X, y, Xs = G.make_case(RQ, 1100, m=129, at_training_point=None)
    g = GPR(X, y, NOISE, kfun(name, par))
    base = call(g, Xs)
    for mode in ("left", "right"):
        monkeypatch.setenv("GPRC_SOLVE", mode)
        assert same_bits(call(g, Xs), base), mode
    g.close()


def test_device_pointers_give_the_bits_of_host_pointers():
    torch = pytest.importorskip("torch")
    name, par, d = ARD3
    X, y, Xs = G.make_case(ARD3, 700, m=129, at_training_point=None)
    g = GPR(X, y, NOISE, kfun(name, par))
    hostv = call(g, Xs)
    ns = Xs.shape[1]
    Xsd = torch.from_numpy(np.ascontiguousarray(Xs.T)).to("cuda")          # row-major n* x d = column-major d x n*
    outs = [torch.full((ns,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2)]
    outs += [torch.full((ns, d), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()                                               # the context's own stream is not ordered with torch's
    nat.check(nat.lib().gprc_gpr_predict_grad(g._model, Xsd.data_ptr(), ns, *[o.data_ptr() for o in outs]))
    devv = [outs[0].cpu().numpy(), outs[1].cpu().numpy(), outs[2].cpu().numpy().T, outs[3].cpu().numpy().T]
    assert same_bits(hostv, devv)
    g.close()


def test_null_outputs_switch_stages_off_and_keep_the_bits():
    name, par, d = SQ8
    X, y, Xs = G.make_case(SQ8, 700, m=129, at_training_point=None)
    g = GPR(X, y, NOISE, kfun(name, par))                  # a fresh model: no reversed factor yet
    lib = nat.lib()
    lib.gprc_prof_enable(1)
    try:
        lib.gprc_prof_reset()
        only_dmean = call(g, Xs, mean=False, var=False, dvar=False)
        prof = nat.prof_summary()
        assert prof["reverse_factor"]["count"] == 0 and prof["pred_grad_contract"]["count"] == 1
        assert prof["solve_panel"]["count"] == 0 and prof["fill"]["count"] == 0          # no chunk of K*, no solve
        no_dvar = call(g, Xs, dvar=False)
        assert nat.prof_summary()["reverse_factor"]["count"] == 0                      # still nothing is factor-reversed
        full = call(g, Xs)
        assert nat.prof_summary()["reverse_factor"]["count"] == 1                      # built by the first call that needs it ...
        again = call(g, Xs)
        assert nat.prof_summary()["reverse_factor"]["count"] == 1                      # ... and kept in the model
    finally:
        lib.gprc_prof_enable(0)
        lib.gprc_prof_reset()
    assert only_dmean[0] is None and only_dmean[1] is None and only_dmean[3] is None
    assert np.array_equal(only_dmean[2], full[2])
    assert no_dvar[3] is None and same_bits(no_dvar[:3], full[:3])
    assert same_bits(again, full)
    only_dvar = call(g, Xs, mean=False, var=False, dmean=False)
    assert np.array_equal(only_dvar[3], full[3])
    only_pred = call(g, Xs, dmean=False, dvar=False)
    assert same_bits(only_pred[:2], full[:2])
    ref = G.predict_grad(name, par, X, y, NOISE, Xs)
    assert all(G.nerr(a, b) <= TOL for a, b in zip(full, ref))
    g.close()


def test_gradients_follow_add_data():
    """the reversed factor is built, then the model grows by 30 points (n_pad unchanged, so a stale one would have the right size): the
    gradients are those of a fresh fit on all 730"""
    name, par, d = SQ3
    X, y, Xs = G.make_case(SQ3, 730, m=129, at_training_point=None)
    g = GPR(X[:, :700], y[:700], NOISE, kfun(name, par))
    before = call(g, Xs)
    g.add_data(X[:, 700:], y[700:])
    after = call(g, Xs)
    fresh = GPR(X, y, NOISE, kfun(name, par))
    want = call(fresh, Xs)
    for what, a, b, c in zip(("mean", "var", "dmean", "dvar"), after, want, before):
        assert G.nerr(a, b) <= 1e-10, what
        assert G.nerr(c, b) > 1e-6, what                   # the 30 points matter: the old factor's answers would not pass
    ref = G.predict_grad(name, par, X, y, NOISE, Xs)
    assert all(G.nerr(a, b) <= TOL for a, b in zip(after, ref))
    g.close()
    fresh.close()


def test_refusals():
    name, par, d = SQ3
    X, y, Xs = G.make_case(SQ3, 150, m=20, at_training_point=None)
    lib = nat.lib()
    ns = Xs.shape[1]
    mean, var, dm, dv = np.empty(ns), np.empty(ns), np.empty((d, ns), order="F"), np.empty((d, ns), order="F")
    args = (mean.ctypes.data, var.ctypes.data, dm.ctypes.data, dv.ctypes.data)

    def refused(model, n_star=ns, xs=Xs.ctypes.data, outs=args):
        rc = lib.gprc_gpr_predict_grad(model, xs, n_star, *outs)
        return rc == nat.ERR_ARG and nat.last_error().startswith("predict_grad:")

    g = GPR(X, y, NOISE, kfun(name, par))
    assert refused(g._model, n_star=0) and refused(g._model, xs=None) and refused(g._model, outs=(None, None, None, None))
    assert refused(None)
    Xc = np.linspace(-1, 1, 21).reshape(1, -1)
    gc = GPC(Xc, 2.0 * (Xc[0] > 0) - 1, cov_func(sqrexp, l=0.4), 1e-5)
    assert refused(gc._model)                              # a GPC model
    gp = GPR(X, y, NOISE, cov_func(polynomial, sigma=0.5, p=2.0))
    assert refused(gp._model)                              # a kernel without a gradient
    with pytest.raises(nat.GprcError, match="predict_grad"):
        gp.predict_grad(Xs)
    gm = GPR(X, y, NOISE, kfun(name, par), devices=[0, 0])  # two virtual ranks on one GPU: rank 0's model is borrowed
    assert refused(gm._model)
    with pytest.raises(ValueError, match="refit"):
        gm.predict_grad(Xs)
    with pytest.raises(ValueError, match="nrow"):
        g.predict_grad(np.ones((2, 3)))
    assert same_bits(call(g, Xs)[:2], list(g.predict(Xs).T))   # the model is as usable as before
    for m in (g, gc, gp, gm):
        m.close()


@pytest.mark.parametrize("case", [SQ3, RQ], ids=K.case_id)
def test_public_api_against_differences_of_predict(case):
    """loose on purpose (central differences of float64 predictions, h = 1e-5): a sign, a factor 2 or a transposed layout shows"""
    name, par, d = case
    X, y, Xs = G.make_case(case, 300, m=10, at_training_point=None)
    g = GPR(X, y, NOISE, kfun(name, par))
    pred, dmean, dvar = g.predict_grad(Xs)
    assert pred.shape == (10, 2) and dmean.shape == (d, 10) and dvar.shape == (d, 10)
    assert np.array_equal(pred, g.predict(Xs))
    pm, dm, none = g.predict_grad(Xs, variance=False)
    assert none is None and np.array_equal(pm, pred) and np.array_equal(dm, dmean)
    h = 1e-5
    for c in range(d):
        up, dn = Xs.copy(), Xs.copy()
        up[c] += h
        dn[c] -= h
        diff = (g.predict(up) - g.predict(dn)) / (2 * h)
        assert np.abs(diff[:, 0] - dmean[c]).max() <= 1e-5 * max(1.0, np.abs(dmean).max())
        assert np.abs(diff[:, 1] - dvar[c]).max() <= 1e-5 * max(1.0, np.abs(dvar).max())
    g.close()
