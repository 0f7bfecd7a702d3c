"""gprc_dev_knn_before on the device against the numpy reference of tests/vecchia_ref.py: exact index equality, order included, with -1
and +inf exactly at the ranks no predecessor fills; exact ties on the integer lattice; windows of queries, host and device pointers and a
wider pitch give the bits of the full call; the argument errors; gprc_dev_knn itself is untouched.  tests/test_vecchia_cpu.py shows that
no two of a point's first m + 1 reference distances are closer than 1e-12 relative on these inputs (measured: 2.8e-9), and the device's
sums are within (d + 4) 2.3e-16 of the reference's, so the device must give the reference's indices."""
import numpy as np
import pytest

import local_ref as LR
import vecchia_ref as V
from gprc_amd import _native as nat
from gprc_amd import knn_before
from gpu_calls import step_time_limit  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu

U = 2.3e-16   # as tests/test_gpu_knn.py: the relative error of a distance is at most (d + 4) U


def check_rows(idx, dist, want_i, want_d, first, m, d, what):
    assert np.array_equal(idx[:, :m], want_i[:, :m]), what
    rank = np.arange(m)[None, :]
    empty = rank >= (first + np.arange(len(idx)))[:, None]
    assert np.array_equal(idx[:, :m] == -1, empty) and np.array_equal(np.isposinf(dist[:, :m]), empty), what
    got, want = dist[:, :m][~empty], want_d[:, :m][~empty]
    assert (np.abs(got - want) <= (d + 4) * U * want).all(), what


@pytest.mark.parametrize("scaled", [False, True], ids=["euclid", "scaled"])
@pytest.mark.parametrize("d", LR.KNN_DIMS)
def test_indices_equal_the_reference(d, scaled):
    """m in {1, 2, 63, 64, 65, 127, 128}, n in {1, m, m + 1, 300, 4099}: a query has fewer candidates than m, exactly m, more; one tile,
    several, several parts"""
    scale = LR.knn_scale(d) if scaled else None
    for m in V.BEFORE_MS:
        for n in sorted({1, m, m + 1, 300, LR.N_MASTER}):
            X = LR.knn_data(d, n)[0]
            want_i, want_d = V.before_reference(d, n, scaled)
            rc, idx, dist = V.call_knn_before(LR.flat(X), d, n, m, scale)
            assert rc == nat.OK, nat.last_error()
            check_rows(idx, dist, want_i, want_d, 0, m, d, (d, scaled, m, n))


@pytest.mark.parametrize("m", [1, 3, 64, 65, 128])
def test_exact_ties_go_to_the_lower_index(m):
    X, _, scale = LR.lattice_data()
    d, n = X.shape
    for sc in (None, scale):
        want_i, want_d = V.knn_before_ref(X, m, sc)
        rc, idx, dist = V.call_knn_before(LR.flat(X), d, n, m, sc)
        assert rc == nat.OK, nat.last_error()
        assert np.array_equal(idx, want_i) and np.array_equal(dist, want_d)      # every distance is exact: the bits too
    assert want_i[411, 0] == 10 if m == 1 else list(want_i[411, :2]) == [10, 200]   # the corner's earlier copies, the lower index first


@pytest.mark.parametrize("m,scaled", [(17, True), (65, False), (128, True)])
def test_a_window_has_the_bits_of_the_full_call(m, scaled):
    """(first, count) at the 32 queries of a workgroup, at the last point alone (the candidates are split into parts and merged) and in the
    middle; host and device pointers; a wider pitch; without dist_out; two calls"""
    torch = pytest.importorskip("torch")
    d, n = 3, LR.N_MASTER
    scale = LR.knn_scale(d) if scaled else None
    xf = LR.flat(LR.knn_data(d, n)[0])
    rc, idx, dist = V.call_knn_before(xf, d, n, m, scale)
    assert rc == nat.OK, nat.last_error()
    assert np.array_equal(idx, V.before_reference(d, n, scaled)[0][:, :m])
    xd = torch.from_numpy(xf).cuda()
    for first, count in ((0, n), (n - 1, 1), (4000, 65)) + V.BEFORE_WINDOWS:
        rc, iw, dw = V.call_knn_before(xf, d, n, m, scale, first, count)
        assert rc == nat.OK, nat.last_error()
        assert np.array_equal(iw, idx[first:first + count]) and np.array_equal(dw, dist[first:first + count]), (first, count)
        rc, iw, dw = V.call_knn_before(xf, d, n, m, scale, first, count, ld=m + 3)     # a wider pitch: the gap keeps the caller's values
        assert rc == nat.OK and np.array_equal(iw[:, :m], idx[first:first + count]) and np.array_equal(dw[:, :m], dist[first:first + count])
        assert (iw[:, m:] == -7).all() and (dw[:, m:] == -7.0).all()
        rc, io, do = V.call_knn_before(xf, d, n, m, scale, first, count, want_dist=False)
        assert rc == nat.OK and do is None and np.array_equal(io, idx[first:first + count])
        it = torch.full((count, m + 3), -7, dtype=torch.int32, device="cuda")
        dt = torch.full((count, m + 3), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rc, _, _ = V.call_knn_before(xd, d, n, m, scale, first, count, ld=m + 3, idx=it, dist=dt)
        assert rc == nat.OK, nat.last_error()
        ih, dh = it.cpu().numpy(), dt.cpu().numpy()
        assert np.array_equal(ih[:, :m], idx[first:first + count]) and np.array_equal(dh[:, :m], dist[first:first + count]), (first, count)
        assert (ih[:, m:] == -7).all() and (dh[:, m:] == -7.0).all()
    rc, i2, d2 = V.call_knn_before(xd, d, n, m, scale)                                  # device X, host outputs; a second full call
    assert rc == nat.OK and np.array_equal(i2, idx) and np.array_equal(d2, dist)


def test_dev_knn_is_unchanged_by_the_new_flag():
    """gprc_dev_knn before and after predecessor-constrained calls on the same inputs: the same bits, and the reference's indices"""
    for d, n, m, scaled in ((3, LR.N_MASTER, 128, False), (8, 1000, 17, True)):
        scale = LR.knn_scale(d) if scaled else None
        X, Xs = LR.knn_data(d, n)
        xf, xsf = LR.flat(X), LR.flat(Xs)
        rc, idx, dist = LR.call_knn(xf, d, n, xsf, 300, m, scale)
        assert rc == nat.OK, nat.last_error()
        assert V.call_knn_before(xf, d, n, m, scale)[0] == nat.OK
        rc, idx2, dist2 = LR.call_knn(xf, d, n, xsf, 300, m, scale)
        assert rc == nat.OK and np.array_equal(idx, idx2) and np.array_equal(dist, dist2)
        assert np.array_equal(idx, LR.knn_reference(d, n, scaled)[0][:300, :m])


def test_the_python_wrapper():
    X = LR.knn_data(3, 1000)[0]
    want_i, want_d = V.before_reference(3, 1000, True)
    idx, dist = knn_before(X, 10, scale=LR.knn_scale(3))
    assert idx.shape == (1000, 10) and np.array_equal(idx, want_i[:, :10])
    assert np.allclose(dist[10:], want_d[10:, :10], rtol=1e-14, atol=0) and np.isposinf(dist[0]).all()
    iw, dw = knn_before(X, 10, scale=LR.knn_scale(3), first=500, count=7)
    assert np.array_equal(iw, idx[500:507]) and np.array_equal(dw, dist[500:507])


def test_argument_errors():
    xf = LR.flat(LR.knn_data(3, 100)[0])
    lib, ctx = nat.lib(), nat.default_context()
    idx, dist = np.zeros((4, 8), dtype=np.intc), np.zeros((4, 8))

    def bad(rc, word):
        assert rc == nat.ERR_ARG and word in nat.last_error(), (rc, nat.last_error())

    bad(lib.gprc_dev_knn_before(None, xf.ctypes.data, 3, 100, 0, 4, None, 8, idx.ctypes.data, dist.ctypes.data, 8), "null context")
    bad(lib.gprc_dev_knn_before(ctx.handle, None, 3, 100, 0, 4, None, 8, idx.ctypes.data, dist.ctypes.data, 8), "null input")
    bad(lib.gprc_dev_knn_before(ctx.handle, xf.ctypes.data, 3, 100, 0, 4, None, 8, None, dist.ctypes.data, 8), "null output")
    for m in (0, 129):
        bad(V.call_knn_before(xf, 3, 100, m, ld=200)[0], "outside 1 .. 128")
    bad(V.call_knn_before(xf, 3, 100, 8, ld=7)[0], "ld_out < m")
    bad(V.call_knn_before(xf, 3, 2 ** 31, 8, count=4)[0], "2^31")
    bad(V.call_knn_before(xf, 0, 100, 8)[0], "d < 1")
    for first, count in ((-1, 4), (0, -1), (97, 4), (101, 0)):
        bad(V.call_knn_before(xf, 3, 100, 8, first=first, count=count)[0], "window")
    for sc in ([1.0, 0.0, 1.0], [1.0, np.inf, 1.0], [np.nan, 1.0, 1.0]):
        bad(V.call_knn_before(xf, 3, 100, 8, scale=sc)[0], "scale")
    rc, i0, d0 = V.call_knn_before(xf, 3, 100, 8, first=50, count=0)                 # no queries: nothing to do
    assert rc == nat.OK and (i0 == -7).all() and (d0 == -7.0).all()
    rc, i1, _ = V.call_knn_before(xf, 3, 100, 128)                                    # m may exceed n
    assert rc == nat.OK and (i1[:, 99:] == -1).all() and np.array_equal(i1[99, :99], V.knn_before_ref(LR.knn_data(3, 100)[0], 99)[0][99])
