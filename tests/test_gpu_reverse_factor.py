"""gprc_dev_reverse_factor on the MI355X: the reversed factor M = J L^T J and its block inverses are, bit for bit, the numpy construction
of tests/pred_grad_ref.py from the very buffers the device read -- zeros above the diagonal included, whatever the input holds there -- and
gprc_dev_solve_rows with them is a backward-stable solve with M, under the two bounds tests/test_gpu_blocks.py puts on solve_rows with L:
    omega <= gamma_{n_pad+1} kappa_blk        and        omega <= RATIO["solve_rows"] max(omega_LAPACK, u)
on the pair (M, B J): the right-hand sides column-reversed, M's identity padding in the LEADING n_pad - n rows and columns (324 of them
at n = 700, 436 at n = 1100: not a multiple of 128)."""
import numpy as np
import pytest
import scipy.linalg as sl

torch = pytest.importorskip("torch")
import gprc_amd  # noqa: E402,F401
from gprc_amd import _native as nat  # noqa: E402
import packed_ref as R  # noqa: E402
import pred_grad_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu

RATIO_SOLVE_ROWS = 4.0                                    # tests/test_gpu_blocks.py, RATIO["solve_rows"]
U, gamma = R.U, R.gamma
_FACTORS = {}


@pytest.fixture
def ctx():
    c = nat.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c
    torch.cuda.synchronize()
    c.close()


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64).cuda()
    torch.cuda.synchronize()
    return t


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def reverse_on_device(ctx, a, w, n_pad):
    ar = torch.full_like(a, float("nan"))
    wr = torch.full_like(w, float("nan"))
    torch.cuda.synchronize()
    nat.check(nat.lib().gprc_dev_reverse_factor(ctx.handle, a.data_ptr(), w.data_ptr(), n_pad, ar.data_ptr(), wr.data_ptr()))
    return ar, wr


@pytest.mark.parametrize("n_pad", [512, 1024, 1536])
def test_reversed_factor_is_bitwise_the_numpy_construction(ctx, n_pad):
    rng = np.random.default_rng(n_pad)
    g = R.geometry(n_pad)
    L = np.tril(rng.normal(size=(n_pad, n_pad)))
    packed = R.pack(L + np.triu(rng.normal(size=(n_pad, n_pad)), 1), n_pad)   # stale non-zero values above the diagonal
    assert all((R.panel_view(packed, g, p)[:g.NB][np.triu_indices(g.NB, 1)] != 0).all() for p in range(g.P))
    winv = rng.normal(size=g.winv_size)
    a, w = dev(packed), dev(winv)
    ar, wr = reverse_on_device(ctx, a, w, n_pad)
    want_p, want_w = G.reverse_packed(host(a), host(w), n_pad)
    got_p, got_w = host(ar), host(wr)
    assert np.array_equal(host(a), packed) and np.array_equal(host(w), winv)   # the inputs are untouched
    assert np.array_equal(got_w, want_w)
    assert np.array_equal(got_p, want_p), int((got_p != want_p).sum())          # NaN anywhere = an element never written
    for p in range(g.P):
        assert not np.triu(R.panel_view(got_p, g, p)[:g.NB], 1).any()           # exact zeros above the diagonal


def factored(ctx, cond):
    """spd(1100, cond) factored on the device, its reversed factor, and host copies; once per cond"""
    if cond not in _FACTORS:
        n = 1100
        K = R.spd(n, cond, R.SEED)
        g = R.geometry(n)
        a = dev(R.pack(K, n))
        w = torch.zeros(g.winv_size, dtype=torch.float64, device="cuda")
        info = torch.zeros(4, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        nat.check(nat.lib().gprc_dev_factor_all(ctx.handle, a.data_ptr(), g.n_pad, w.data_ptr(), info.data_ptr(), None))
        torch.cuda.synchronize()
        assert int(info[0]) == 0
        ar, wr = reverse_on_device(ctx, a, w, g.n_pad)
        Lp = R.unpack_lower(host(a), g.n_pad)
        Mp = R.unpack_lower(host(ar), g.n_pad)
        assert np.array_equal(Mp, Lp[::-1, ::-1].T)
        _FACTORS[cond] = dict(n=n, g=g, a=a, w=w, ar=ar, wr=wr, Lp=Lp, Mp=Mp)
    return _FACTORS[cond]


@pytest.mark.parametrize("shape", R.SOLVE_ROWS_SHAPES, ids=lambda s: "m%d-ld%d" % s)
@pytest.mark.parametrize("cond", R.SOLVE_CONDS)
def test_backward_solve_through_solve_rows(ctx, cond, shape):
    """vt := (B J) M^-T: residual B J - Y M^T on the valid block, the zero padding columns (now the LEADING ones) stay zero, the
    ld - m_pad rows between the columns are not touched; and Y J solves X L = B."""
    m_pad, ld = shape
    f = factored(ctx, cond)
    n, g, Mp = f["n"], f["g"], f["Mp"]
    pad = g.n_pad - n
    M = Mp[pad:, pad:]                                    # the n x n lower factor behind the identity padding
    kap = R.kappa_blk(Mp, 512)
    rng = np.random.default_rng(R.SEED + 3)
    buf = rng.normal(size=(g.n_pad, ld))                  # [column j of the chunk, row i]
    buf[n:, :m_pad] = 0.0                                 # B: zero in L's padding columns ...
    bufJ = buf.copy()
    bufJ[:, :m_pad] = buf[::-1, :m_pad]                   # ... B J: the chunk's columns reversed (the gap rows stay where they are)
    vt = dev(bufJ)
    nat.check(nat.lib().gprc_dev_solve_rows(ctx.handle, f["ar"].data_ptr(), f["wr"].data_ptr(), g.n_pad, vt.data_ptr(), ld, m_pad))
    out = host(vt).reshape(g.n_pad, ld)
    assert np.isfinite(out).all()
    assert np.array_equal(out[:, m_pad:], bufJ[:, m_pad:])
    assert not out[:pad, :m_pad].any()
    B, X = bufJ[pad:, :m_pad], out[pad:, :m_pad]          # columns = right-hand sides: M X = (B J)^T
    wg = R.omega_tri(M, X, B)
    wl = R.omega_tri(M, sl.solve_triangular(M, B, lower=True), B)
    case = "n1100-cond%.0e m_pad %d ld %d" % (cond, m_pad, ld)
    print("reversed solve_rows %s: omega_gpu %.2f u, omega_lapack %.2f u, kappa_blk %.3g" % (case, wg / U, wl / U, kap))
    assert wg <= gamma(g.n_pad + 1) * kap, (case, wg / U)
    assert wg <= RATIO_SOLVE_ROWS * max(wl, U), (case, wg / U, wl / U)
    # the same numbers read the other way round: rows of Y J against X L = B, L the device's own factor
    L = f["Lp"][:n, :n]
    wL = R.omega_tri(L, out[::-1, :m_pad][:n], buf[:n, :m_pad], transpose=True)
    assert wL <= gamma(g.n_pad + 1) * kap, (case, wL / U)
