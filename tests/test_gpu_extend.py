"""GPR.add_data / gprc_gpr_extend on the MI355X: an extended model matches a fresh GPR on the concatenated data (and the CPU
oracle up to n' = 3000) in alpha, logp, $L and both predict forms, normwise 1e-10; the geometry cases cover an unchanged n_pad,
aligned n, p0 = 0, tails that cross panels, m > n, the grouped predict solve and the grouped left-looking factor of the tail."""
import ctypes as C

import numpy as np
import pytest

from conftest import TOL, nerr, oracle_params
from gprc_amd import GPR, GPC, GprcError, NotPositiveDefinite, cov_func, constant, linear, polynomial, sqrexp, gammaexp, rationalquadratic
from gprc_amd import _native as nat
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

GENERIC = {"constant": constant, "linear": linear, "polynomial": polynomial, "sqrexp": sqrexp, "gammaexp": gammaexp,
           "rationalquadratic": rationalquadratic}
KERNELS = [("constant", dict(c=1.7)), ("linear", dict(sigma=0.7)), ("polynomial", dict(sigma=0.5, p=3.0)), ("sqrexp", dict(l=1.3)),
           ("gammaexp", dict(l=0.9, gamma=1.5)), ("rationalquadratic", dict(l=1.1, alpha=1.5))]
NOISE = 0.3


def kfun(kind, par):
    return cov_func(GENERIC[kind], **par)


def data(n, d, seed):
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(rng.uniform(-1, 1, (d, n)))
    y = 0.1 * (X ** 3).sum(0) + rng.normal(0, 0.1, n)
    return X, y


def nerr_cols(got, ref, step=2048):
    """nerr for large square matrices, a block of columns at a time (no full-size temporaries)"""
    assert got.shape == ref.shape
    num = den = 0.0
    for c in range(0, ref.shape[1], step):
        g, r = got[:, c:c + step], ref[:, c:c + step]
        assert np.isfinite(g).all()
        num, den = max(num, float(np.abs(g - r).max())), max(den, float(np.abs(r).max()))
    return num / max(den, 1e-300)


def check_against_fresh_fit(g, X, y, noise, kind, par, seed=0):
    d, n1 = X.shape
    assert g.X.shape == (d, n1) and np.array_equal(g.X, X) and np.array_equal(g.y, y)
    ref = GPR(X, y, noise, kfun(kind, par))
    assert ref.noise == noise and g.noise == noise
    assert nerr(g.alpha, ref.alpha) <= TOL, (kind, n1)
    assert abs(g.logp - ref.logp) <= TOL * abs(ref.logp), (kind, n1)
    assert nerr_cols(g.L, ref.L) <= TOL, (kind, n1)
    Xs = np.asfortranarray(np.random.default_rng(seed + 1).uniform(-1, 1, (d, 97)))
    pr, prr = g.predict(Xs), ref.predict(Xs)
    assert nerr(pr[:, 0], prr[:, 0]) <= TOL and nerr(pr[:, 1], prr[:, 1]) <= TOL, (kind, n1)
    mean, cov = g.predict(Xs, pointwise_var=False)
    meanr, covr = ref.predict(Xs, pointwise_var=False)
    assert nerr(mean, meanr) <= TOL and nerr(cov, covr) <= TOL, (kind, n1)
    if n1 <= 3000:
        kid, op = orc.KERNEL_IDS[kind], oracle_params(kind, par)
        f = orc.gpr_fit(kid, op, X, y, noise)
        assert nerr(g.alpha, f["alpha"]) <= TOL and abs(g.logp - f["logp"]) <= TOL * abs(f["logp"])
        assert nerr(g.L, f["L"]) <= TOL
        mo, vo = orc.gpr_predict(kid, op, X, f["L"], f["alpha"], Xs)
        assert nerr(pr[:, 0], mo) <= TOL and nerr(pr[:, 1], vo) <= TOL
        _, co = orc.gpr_predict(kid, op, X, f["L"], f["alpha"], Xs, pointwise=False)
        assert nerr(cov, co) <= TOL
    ref.close()


def extend_case(n, m, d, kind, par, seed):
    X, y = data(n + m, d, seed)
    g = GPR(X[:, :n], y[:n], NOISE, kfun(kind, par))
    assert g.add_data(X[:, n:], y[n:]) is g
    return g, X, y


@pytest.mark.parametrize("kind,par", KERNELS, ids=[k for k, _ in KERNELS])
def test_extend_all_kernels_from_below_one_panel(kind, par):
    g, X, y = extend_case(300, 50, 3, kind, par, seed=11)
    check_against_fresh_fit(g, X, y, NOISE, kind, par)


@pytest.mark.parametrize("n,m", [(1000, 20),      # n_pad unchanged
                                 (1024, 1),       # aligned n: the tail is the new points only
                                 (511, 1),        # p0 = 0
                                 (1000, 700),     # the tail crosses panels
                                 (100, 2000),     # m > n
                                 (16000, 5000),   # t_pad = 5248: the predict solve runs in groups of 25 < 31 panels
                                 (1000, 21000)])  # a tail of 21504 > 20480: grouped left-looking factor on the sub-view
def test_extend_sqrexp_geometry(n, m):
    g, X, y = extend_case(n, m, 8, "sqrexp", dict(l=1.0), seed=n + m)
    n_out, d_out = C.c_int64(), C.c_int64()
    nat.check(nat.lib().gprc_model_dims(g._model, C.byref(n_out), C.byref(d_out)))
    assert (n_out.value, d_out.value) == (n + m, 8)
    check_against_fresh_fit(g, X, y, NOISE, "sqrexp", dict(l=1.0), seed=n)


def test_chained_extends_match_one_fit():
    X, y = data(300 + 10 * 37, 4, 5)
    k = kfun("rationalquadratic", dict(l=1.1, alpha=1.5))
    g = GPR(X[:, :300], y[:300], NOISE, k)
    for i in range(10):
        a = 300 + 37 * i
        g.add_data(X[:, a:a + 37], y[a:a + 37])
    check_against_fresh_fit(g, X, y, NOISE, "rationalquadratic", dict(l=1.1, alpha=1.5))


def test_extend_is_bitwise_repeatable():
    runs = []
    for _ in range(2):
        g, X, y = extend_case(1000, 700, 8, "sqrexp", dict(l=1.0), seed=3)
        runs.append((g.alpha.copy(), g.logp, g.L.copy(), g.predict(X[:, :64])))
        g.close()
    (a0, l0, L0, p0), (a1, l1, L1, p1) = runs
    assert np.array_equal(a0, a1) and l0 == l1 and np.array_equal(L0, L1) and np.array_equal(p0, p1)


def test_device_inputs_give_the_bits_of_host_inputs():
    torch = pytest.importorskip("torch")
    n, m, d = 1000, 700, 8
    X, y = data(n + m, d, 9)
    k = kfun("sqrexp", dict(l=1.0))
    host = GPR(X[:, :n], y[:n], NOISE, k).add_data(X[:, n:], y[n:])
    dev = GPR(X[:, :n], y[:n], NOISE, k)
    Xt = torch.from_numpy(np.ascontiguousarray(X[:, n:].T)).to("cuda")    # row-major m x d = column-major d x m
    yt = torch.from_numpy(np.ascontiguousarray(y[n:])).to("cuda")
    torch.cuda.synchronize()                                             # the context's own stream is not ordered with torch's
    nat.check(nat.lib().gprc_gpr_extend(dev._model, Xt.data_ptr(), m, yt.data_ptr()))
    alpha, lp = np.empty(n + m), C.c_double()
    nat.check(nat.lib().gprc_gpr_get_alpha(dev._model, alpha.ctypes.data))
    nat.check(nat.lib().gprc_gpr_get_logp(dev._model, C.byref(lp)))
    assert np.array_equal(alpha, host.alpha) and lp.value == host.logp
    L = np.empty((n + m, n + m), order="F")
    nat.check(nat.lib().gprc_model_get_L(dev._model, L.ctypes.data, n + m))
    assert np.array_equal(L, host.L)


def test_caches_and_accessors_follow_the_extend():
    X, y = data(700, 2, 21)
    g = GPR(X[:, :600], y[:600], NOISE, kfun("sqrexp", dict(l=0.8)))
    assert g.L.shape == (600, 600)           # the $L cache is filled before the extend ...
    g.add_data(X[:, 600:].ravel(order="F"), y[600:])   # a bare vector is filled column by column into nrow(X) rows
    assert g.L.shape == (700, 700)           # ... and dropped by it
    assert np.array_equal(g.X, X) and np.array_equal(g.y, y) and g.alpha.shape == (700,)
    n_out = C.c_int64()
    nat.check(nat.lib().gprc_model_dims(g._model, C.byref(n_out), None))
    assert n_out.value == 700
    check_against_fresh_fit(g, X, y, NOISE, "sqrexp", dict(l=0.8))


def test_extend_keeps_the_jittered_noise():
    X, y = data(350, 2, 4)
    k = kfun("constant", dict(c=1.0))        # c 1 1^T is singular: the fit moves the noise from 0 to 0.01
    with pytest.warns(UserWarning, match="Noise got changed to 0.01"):
        g = GPR(X[:, :300], y[:300], 0, k)
    assert g.noise == 0.01
    g.add_data(X[:, 300:], y[300:])
    assert g.noise == 0.01
    check_against_fresh_fit(g, X, y, 0.01, "constant", dict(c=1.0))


def test_non_pd_extension_raises_and_leaves_the_model_unchanged():
    g = GPR(np.array([[2.0]]), np.array([1.0]), 0, kfun("polynomial", dict(sigma=-1.0, p=1.0)))   # k(2, 2) = 3
    before = (g.alpha.copy(), g.logp, g.predict(np.array([0.5, 1.5])))
    with pytest.raises(NotPositiveDefinite) as e:   # second pivot: -0.99 - 0.8^2 / 3 < 0
        g.add_data(np.array([[0.1]]), np.array([0.0]))
    assert e.value.info == 2
    assert nat.last_error().startswith("extend:")
    assert np.array_equal(g.alpha, before[0]) and g.logp == before[1]
    assert np.array_equal(g.predict(np.array([0.5, 1.5])), before[2])
    assert np.array_equal(g.X, [[2.0]]) and g.L.shape == (1, 1)
    alpha = np.empty(1)
    nat.check(nat.lib().gprc_gpr_get_alpha(g._model, alpha.ctypes.data))
    assert np.array_equal(alpha, before[0])


def test_extend_refusals():
    X, y = data(200, 3, 8)
    k = kfun("sqrexp", dict(l=1.0))
    g = GPR(X[:, :150], y[:150], NOISE, k)
    with pytest.raises(ValueError, match="length\\(X_new\\) %% nrow\\(self\\$X\\) == 0"):
        g.add_data(np.ones(4), np.ones(1))                               # 4 values do not fill columns of 3
    with pytest.raises(ValueError, match="nrow"):
        g.add_data(np.ones((2, 3)), np.ones(3))                          # d mismatch
    with pytest.raises(ValueError, match="length\\(y_new\\) == ncol\\(X_new\\)"):
        g.add_data(X[:, 150:], y[150:160])
    with pytest.raises(TypeError):
        g.add_data(np.array([["a", "b", "c"]]).T, np.ones(1))
    with pytest.raises(GprcError):                                       # m = 0
        g.add_data(np.empty((3, 0)), np.empty(0))
    assert nat.last_error().startswith("extend:")
    assert g.X.shape == (3, 150)
    xs = X[:, 150:]
    assert nat.lib().gprc_gpr_extend(g._model, xs.ctypes.data, 0, y[150:].ctypes.data) == nat.ERR_ARG
    assert nat.lib().gprc_gpr_extend(g._model, None, 50, y[150:].ctypes.data) == nat.ERR_ARG
    Xc = np.linspace(-1, 1, 21).reshape(1, -1)
    gc = GPC(Xc, 2.0 * (Xc[0] > 0) - 1, cov_func(sqrexp, l=0.4), 1e-5)   # GPC: the Laplace fit must iterate again
    xc, yc = np.array([0.05]), np.array([1.0])
    assert nat.lib().gprc_gpr_extend(gc._model, xc.ctypes.data, 1, yc.ctypes.data) == nat.ERR_ARG
    assert nat.last_error().startswith("extend:")
    gm = GPR(X[:, :150], y[:150], NOISE, k, devices=[0, 0])             # two virtual ranks on one GPU
    with pytest.raises(ValueError, match="refit"):
        gm.add_data(X[:, 150:], y[150:])
    assert nat.lib().gprc_gpr_extend(gm._model, xs.ctypes.data, 50, y[150:].ctypes.data) == nat.ERR_ARG   # rank 0's borrowed model
    assert nat.last_error().startswith("extend:")
    assert gm.X.shape == (3, 150)
