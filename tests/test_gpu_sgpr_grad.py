"""The gradient of the sparse GPR's bound on the MI355X: gprc_sgpr_elbo_grad (fit.elbo_grad, fit.optimize_sparse) and its contraction
kernel alone (gprc_dev_cross_grad), against the float64 formulas of tests/sgpr_grad_ref.py (which tests/test_sgpr_grad_cpu.py ties to
their longdouble twin and to central differences) and against the library's own exact gradient at Z = X.

Gates: the project's TOL = 1e-10 -- relative on every kernel parameter's entry and on the noise's, normwise (conftest.nerr) on dZ;
bitwise equality of the bound with gprc_sgpr_elbo, of two calls, of the call without dZ, of host and device pointers; agreement to TOL
between one chunk and 256-row chunks; at Z = X, jitter 0 the entries of gprc_gpr_logp_grad to TOL and max |dZ| <= 1e-10 max |grad|;
the contraction alone on a standard-normal G inside |got - ref| <= TOL * sum |terms| of every output, the reference summed by
math.fsum.

Shapes (sgpr_grad_ref.CASES): n and m off every tile size; m_pad = 512 and 1024; m = 130; d = 2, 3, 9 (three coordinate groups of the
column sums, ARD) and 20 (seven groups, the second staging pass); gammaexp with s = 0 pairs (Z is a subset of X); for the contraction
alone also 4200 rows (two row tiles per stripe), NaN in G's padding rows and columns, and a dZ that is added to.

Measured on an MI355X (every test prints its figures), 21 passed in 14 s: against the float64 reference every theta entry and the noise
<= 7.6e-15, the bound <= 5.2e-15, dZ 6.9e-13, 7.0e-14, 9.5e-13, 3.2e-13, 1.3e-14, 2.0e-15, 1.9e-15, 2.5e-14 (cases 0..7); 256-row chunks
against one chunk: theta and noise the same bits, dZ 1.4e-16; Z = X against gprc_gpr_logp_grad: <= 2.3e-13, max |dZ| 3.8e-8 against
max |grad| 3.7e3 (sqrexp {0.3}, the bound 3.7e-7) and 7.1e-12 against 4.1e3 (matern52_ard); the contraction alone at <= 2.4e-16 of
sum |terms|; optimize_sparse (n = 1500, m = 60, 12 iterations): bound -255.2 -> 1263.3, l 1.5 -> 1.69, noise 0.2 -> 0.0099.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import sgpr_grad_ref as G
import sgpr_ref as R
from conftest import TOL, nerr
from gprc_amd import NotPositiveDefinite, SparseGPR, select_inducing
from gprc_amd import _native as nat
from gprc_amd.fit import elbo, elbo_grad, grad_dict, logp_grad, optimize_sparse
from gpu_calls import kfun, same_bits, step_time_limit  # noqa: F401  (the autouse fixture)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def reference(index):
    """the problem and the float64 reference of case `index`, computed once and shared; the arrays are never written to"""
    name, theta, n, m, d = G.CASES[index]
    X, y, Z = G.problem(index)
    r = G.elbo_grad(name, theta, X, y, G.NOISE, Z, G.JITTER)
    out = dict(X=X, y=y, Z=Z, name=name, theta=theta, elbo=float(r["elbo"]), grad=np.asarray(r["grad"], dtype=float), dZ=np.asarray(r["dZ"], dtype=float))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def raw(ctx, name, theta, X, y, noise, Z, jitter, with_Z=True, ptrs=None):
    """gprc_sgpr_elbo_grad -> (rc, elbo, grad, dZ); ptrs: dict(X=, y=, Z=, dZ=) of device addresses in place of the host arrays (a
    device dZ is the caller's to read)"""
    ptrs = ptrs or {}
    d, n = X.shape
    m = Z.shape[1]
    _, pp, npar = nat.params_array(np.asarray(theta, dtype=float))
    g, e = np.full(npar + 1, np.nan), C.c_double(float("nan"))
    dZ = np.full((d, m), np.nan, order="F") if with_Z else None
    dzp = ptrs.get("dZ") or (dZ.ctypes.data if with_Z else None)
    rc = nat.lib().gprc_sgpr_elbo_grad(ctx.handle, grad_dict[name].kernel_id if name in grad_dict else name, pp, npar, ptrs.get("X") or X.ctypes.data, d, n,
                                       ptrs.get("y") or y.ctypes.data, noise, ptrs.get("Z") or Z.ctypes.data, m, jitter, C.byref(e), g.ctypes.data, dzp)
    return rc, e.value, g, dZ


def errors(grad, dZ, ref_grad, ref_dZ):
    e = {"theta%d" % k: abs(grad[k] - ref_grad[k]) / abs(ref_grad[k]) for k in range(len(grad) - 1)}
    e["noise"] = abs(grad[-1] - ref_grad[-1]) / abs(ref_grad[-1])
    if dZ is not None:
        e["dZ"] = nerr(dZ, ref_dZ)
    return e


# ---- 1. values ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(G.CASES)), ids=G.CASE_IDS)
def test_gradient_against_the_float64_reference(index):
    ref = reference(index)
    value, grad, dZ = elbo_grad(ref["X"], ref["y"], G.NOISE, ref["name"], ref["theta"], ref["Z"], G.JITTER)
    errs = errors(grad, dZ, ref["grad"], ref["dZ"])
    errs["elbo"] = abs(value - ref["elbo"]) / abs(ref["elbo"])
    print("sgpr gradient case %d (%s): %s; max |grad| %.3g max |dZ| %.3g" % (index, ref["name"], {k: "%.2e" % v for k, v in errs.items()},
                                                                           np.abs(grad).max(), np.abs(dZ).max()))
    assert max(errs.values()) <= TOL, errs
    assert value == elbo(ref["X"], ref["y"], G.NOISE, kfun(ref["name"], ref["theta"]), ref["Z"], G.JITTER)   # the bits of gprc_sgpr_elbo


# ---- 2. bits --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [0, 4, 5], ids=[G.CASE_IDS[i] for i in (0, 4, 5)])
def test_two_calls_and_the_call_without_dZ_give_the_same_bits(index):
    ref = reference(index)
    ctx = nat.default_context()
    args = (ctx, ref["name"], ref["theta"], ref["X"], ref["y"], G.NOISE, ref["Z"], G.JITTER)
    first, second, without = raw(*args), raw(*args), raw(*args, with_Z=False)
    assert first[0] == 0 and same_bits(first, second)
    assert without[0] == 0 and without[3] is None and same_bits(without[:3], first[:3])


def test_host_and_device_pointers_give_the_same_bits():
    torch = pytest.importorskip("torch")
    ref = reference(3)
    ctx = nat.default_context()
    args = (ctx, ref["name"], ref["theta"], ref["X"], ref["y"], G.NOISE, ref["Z"], G.JITTER)
    host = raw(*args)
    dev = {k: torch.from_numpy(np.array(ref[k].T if ref[k].ndim == 2 else ref[k], order="C", copy=True)).cuda() for k in ("X", "y", "Z")}
    dzd = torch.full((ref["Z"].shape[1], ref["Z"].shape[0]), float("nan"), dtype=torch.float64).cuda()   # m x d row-major = d x m column-major
    torch.cuda.synchronize()
    got = raw(*args, ptrs=dict(X=dev["X"].data_ptr(), y=dev["y"].data_ptr(), Z=dev["Z"].data_ptr(), dZ=dzd.data_ptr()))
    torch.cuda.synchronize()
    assert host[0] == 0 and got[0] == 0
    assert same_bits(got[:3], host[:3]) and np.array_equal(dzd.cpu().numpy().T, host[3])


# ---- 3. chunking ------------------------------------------------------------------------------------------------------------------------
def test_chunks_of_256_rows_agree_with_one_chunk(monkeypatch):
    ref = reference(2)                                              # n = 900, m = 600: m_pad = 1024
    whole = raw(nat.default_context(), ref["name"], ref["theta"], ref["X"], ref["y"], G.NOISE, ref["Z"], G.JITTER)
    monkeypatch.setenv("GPRC_CHUNK_BYTES", str(256 * 1024 * 8))     # 256 rows per chunk at m_pad = 1024: four chunks
    ctx2 = nat.Context(0)
    parts = raw(ctx2, ref["name"], ref["theta"], ref["X"], ref["y"], G.NOISE, ref["Z"], G.JITTER)
    again = raw(ctx2, ref["name"], ref["theta"], ref["X"], ref["y"], G.NOISE, ref["Z"], G.JITTER)
    ctx2.close()
    assert whole[0] == 0 and parts[0] == 0
    errs = errors(parts[2], parts[3], whole[2], whole[3])
    print("256-row chunks against one chunk: %s" % {k: "%.2e" % v for k, v in errs.items()})
    assert parts[1] == whole[1]                                     # the bound: bit for bit under every chunking
    assert max(errs.values()) <= TOL, errs
    assert same_bits(parts, again)                                  # bit-reproducible at a fixed chunking


# ---- 4. tight at Z = X --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index,case", list(enumerate(R.TIGHT_CASES)), ids=[c[0] for c in R.TIGHT_CASES])
def test_inducing_points_equal_to_the_data_give_the_exact_gradient(index, case):
    name, theta = case
    X, y, _, _ = R.problem(len(R.CASES) + index, R.TIGHT_N, 1, R.TIGHT_D)
    lp, gl = logp_grad(X, y, R.NOISE, name, theta)
    value, grad, dZ = elbo_grad(X, y, R.NOISE, name, theta, X, 0.0)
    errs = {"elbo": abs(value - lp) / abs(lp)}
    errs.update({"g%d" % k: abs(grad[k] - gl[k]) / abs(gl[k]) for k in range(len(gl))})
    print("Z = X %s: %s; max |dZ| %.2e against max |grad| %.3g" % (name, {k: "%.2e" % v for k, v in errs.items()}, np.abs(dZ).max(), np.abs(grad).max()))
    assert max(errs.values()) <= TOL, errs
    assert np.abs(dZ).max() <= 1e-10 * np.abs(grad).max()


# ---- 5. the contraction kernel alone --------------------------------------------------------------------------------------------------
CROSS = [   # (kernel, parameters, rows, cols, d, coincident points)
    ("sqrexp_ard", list(np.linspace(0.8, 1.9, 20)), 200, 100, 20, 0),
    ("gammaexp", [0.9, 1.3], 300, 130, 2, 50),
    ("matern52", [0.7], 4200, 70, 3, 0),
    ("rationalquadratic", [0.8, 1.4], 129, 65, 4, 0),
]


@pytest.mark.parametrize("case", CROSS, ids=[c[0] for c in CROSS])
def test_cross_grad_on_a_standard_normal_matrix(case):
    torch = pytest.importorskip("torch")
    name, theta, rows, cols, d, same = case
    rng = np.random.default_rng(11 + rows)
    A, Z = rng.uniform(-2, 2, (d, rows)), rng.uniform(-2, 2, (d, cols))
    A[:, :same] = Z[:, :same]                                       # s = 0 pairs
    Gm = rng.standard_normal((rows, cols))
    D0 = rng.standard_normal((d, cols))
    f = 0.37
    rows_pad, cols_pad = -(-rows // 128) * 128, -(-cols // 64) * 64
    ld = rows_pad + 2
    Gd = np.full((cols_pad, ld), np.nan)                            # column j of G = row j of the C-ordered host image; NaN in all the padding
    Gd[:cols, :rows] = Gm.T
    ctx = nat.Context(0, torch.cuda.current_stream().cuda_stream)
    gdev, adev, zdev = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (Gd, A.T, Z.T))
    _, pp, npar = nat.params_array(np.asarray(theta, dtype=float))

    def run(with_Z):
        g = np.full(npar, np.nan)
        dz = torch.from_numpy(np.ascontiguousarray(D0.T)).cuda() if with_Z else None
        torch.cuda.synchronize()
        nat.check(nat.lib().gprc_dev_cross_grad(ctx.handle, grad_dict[name].kernel_id, pp, npar, gdev.data_ptr(), ld, adev.data_ptr(), rows, zdev.data_ptr(),
                                                cols, d, f, g.ctypes.data, dz.data_ptr() if with_Z else None))
        torch.cuda.synchronize()
        return g, (dz.cpu().numpy().T if with_Z else None)

    g1, dz1 = run(True)
    g2, dz2 = run(True)
    g0, _ = run(False)
    torch.cuda.synchronize()
    ctx.close()
    assert np.array_equal(g1, g2) and np.array_equal(dz1, dz2) and np.array_equal(g0, g1)
    th, zt = G.cross_terms(name, theta, Gm, A, Z)
    worst = 0.0
    for k, terms in enumerate(th):
        want, mag = f * math.fsum(terms.ravel()), f * math.fsum(np.abs(terms).ravel())
        worst = max(worst, abs(g1[k] - want) / mag)
        assert abs(g1[k] - want) <= TOL * mag, (k, g1[k], want)
    for c in range(d):
        for j in range(cols):
            want = D0[c, j] + f * math.fsum(zt[c, :, j])
            mag = abs(D0[c, j]) + f * math.fsum(np.abs(zt[c, :, j]))
            worst = max(worst, abs(dz1[c, j] - want) / mag)
            assert abs(dz1[c, j] - want) <= TOL * mag, (c, j, dz1[c, j], want)
    print("cross_grad %s %d x %d, d = %d: worst |got - ref| / sum |terms| %.2e" % (name, rows, cols, d, worst))


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    ref = reference(3)
    ctx = nat.default_context()
    X, y, Z = ref["X"], ref["y"], ref["Z"]
    rc, *_ = raw(ctx, nat.LINEAR, [1.3], X, y, G.NOISE, Z, G.JITTER)
    assert rc == nat.ERR_ARG and nat.last_error()
    Zdup = np.asfortranarray(np.hstack([Z[:, :1], Z[:, :1], Z[:, 1:]]))   # k(z,z) = 1 = l_10^2 exactly: singular at the second pivot
    rc, *_ = raw(ctx, "sqrexp", [0.6], X, y, G.NOISE, Zdup, 0.0)
    assert rc == 2 and "K_uu" in nat.last_error()
    with pytest.raises(NotPositiveDefinite):
        elbo_grad(X, y, G.NOISE, "sqrexp", [0.6], Zdup, 0.0)
    rc, e, g, dZ = raw(ctx, "sqrexp", [0.6], X, y, G.NOISE, Zdup, G.JITTER)   # with a jitter the same Z has a gradient
    assert rc == 0 and np.isfinite(e) and np.isfinite(g).all() and np.isfinite(dZ).all()
    d, n = X.shape
    _, pp, npar = nat.params_array(np.asarray([0.6]))
    val = C.c_double()
    assert nat.lib().gprc_sgpr_elbo_grad(ctx.handle, nat.SQREXP, pp, npar, X.ctypes.data, d, n, y.ctypes.data, G.NOISE, Z.ctypes.data, Z.shape[1],
                                         G.JITTER, C.byref(val), None, None) == nat.ERR_ARG                 # grad_out is required


# ---- 7. the optimiser -----------------------------------------------------------------------------------------------------------------
def test_optimize_sparse_raises_the_bound_and_gives_a_model():
    n, m, d = 1500, 60, 2
    X, y, _, Xs = R.problem(40, n, m, d)
    Z0 = select_inducing(X, m, rng=3)
    start, noise0 = [1.5], 0.2
    before = elbo(X, y, noise0, kfun("sqrexp", start), Z0)
    r = optimize_sparse(X, y, noise0, "sqrexp", Z0, start, maxit=12)
    print("optimize_sparse: bound %.3f -> %.3f, l %.4f, noise %.4f, counts %s, convergence %d; Z moved by at most %.3f"
          % (before, r["value"], r["par"][0], r["noise"], r["counts"], r["convergence"], np.abs(r["Z"] - Z0).max()))
    assert r["value"] > before and r["Z"].shape == (d, m) and r["noise"] > 0 and r["convergence"] in (0, 1)
    s = SparseGPR(X, y, r["noise"], r["func"], r["Z"])
    assert abs(s.elbo - r["value"]) <= 1e-8 * abs(r["value"])       # (vmmin may return a last trial point a rounding away from the accepted one)
    mean, var = s.predict(Xs)
    s.close()
    assert np.isfinite(mean).all() and (var > -1e-9).all()
    fixed = optimize_sparse(X, y, noise0, "sqrexp", Z0, start, optimize_Z=False, optimize_noise=False, maxit=5)
    assert fixed["noise"] == noise0 and np.array_equal(fixed["Z"], Z0) and fixed["value"] > before
