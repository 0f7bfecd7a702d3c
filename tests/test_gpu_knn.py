"""gprc_dev_knn on the device against the numpy reference of tests/local_ref.py: exact index equality, order included, at the sizes where
a tile tail, a lane boundary of the register-resident list or a full list can go wrong; the distances within their derived bound; exact
ties on an integer lattice; the bit contract (a point alone, host and device pointers, a wider pitch, two calls); the argument errors.
tests/test_local_cpu.py shows that no two of a point's first m + 1 reference distances are closer than 1e-9 relative on these inputs,
so the device's differently rounded distances (fused multiply-adds) must give the reference's indices."""
import numpy as np
import pytest

import local_ref as LR
from gprc_amd import _native as nat
from gprc_amd import knn
from gpu_calls import step_time_limit  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu

U = 2.3e-16   # a little above 2^-52: three roundings per term and d - 1 additions of non-negative terms bound the relative error by (d + 4) U


def check_against_reference(idx, dist, order, sdist, ns, m, d, n, what):
    assert np.array_equal(idx[:ns, :m], order[:ns, :m]), what
    want = sdist[:ns, :m]
    err = np.abs(dist[:ns, :m] - want)
    assert (err <= (d + 4) * U * want).all(), (what, float((err / np.maximum(want, 1e-300)).max()))
    k = min(5, n, ns)                                   # the first test points are the first training points: distance exactly 0, first
    assert np.array_equal(idx[:k, 0], np.arange(k)) and not dist[:k, 0].any(), what


@pytest.mark.parametrize("m", LR.KNN_MS)
@pytest.mark.parametrize("scaled", [False, True], ids=["euclid", "scaled"])
@pytest.mark.parametrize("d", LR.KNN_DIMS)
def test_knn_indices_equal_the_reference(d, scaled, m):
    """n in {m, m + 1, 1000, 4099} (4099: the candidates are split over workgroups and merged), n* in {1, 63, 64, 65, 300}"""
    scale = LR.knn_scale(d) if scaled else None
    for n in LR.knn_sizes(m):
        X, Xs = LR.knn_data(d, n)
        order, sdist = LR.knn_reference(d, n, scaled)
        xf, xsf = LR.flat(X), LR.flat(Xs)
        for ns in LR.KNN_NS:
            rc, idx, dist = LR.call_knn(xf, d, n, xsf, ns, m, scale)
            assert rc == nat.OK, nat.last_error()
            check_against_reference(idx, dist, order, sdist, ns, m, d, n, (d, scaled, m, n, ns))


@pytest.mark.parametrize("m", [1, 3, 64, 65, 128])
def test_exact_ties_go_to_the_lower_index(m):
    X, Xs, scale = LR.lattice_data()
    d, n = X.shape
    ns = Xs.shape[1]
    for sc in (None, scale):
        want_i, want_d = LR.knn_ref(X, Xs, m, sc)
        rc, idx, dist = LR.call_knn(LR.flat(X), d, n, LR.flat(Xs), ns, m, sc)
        assert rc == nat.OK, nat.last_error()
        assert np.array_equal(idx, want_i) and np.array_equal(dist, want_d)      # every distance is exact: the bits too
        if m >= 3:
            assert list(idx[0, :3]) == [10, 200, 411] and not dist[0, :3].any()


@pytest.mark.parametrize("n,m,scaled", [(1000, 65, True), (4099, 128, False), (4099, 17, True)])
def test_a_point_s_bits_do_not_depend_on_the_call(n, m, scaled):
    """every point alone, a prefix of the points, a wider pitch, two calls, device pointers for inputs and outputs"""
    torch = pytest.importorskip("torch")
    d, ns = 3, 65
    scale = LR.knn_scale(d) if scaled else None
    X, Xs = LR.knn_data(d, n)
    xf, xsf = LR.flat(X), LR.flat(Xs)[:d * ns].copy()
    rc, idx, dist = LR.call_knn(xf, d, n, xsf, ns, m, scale)
    assert rc == nat.OK, nat.last_error()
    assert np.array_equal(idx, LR.knn_reference(d, n, scaled)[0][:ns, :m])
    rc, idx2, dist2 = LR.call_knn(xf, d, n, xsf, ns, m, scale)
    assert rc == nat.OK and np.array_equal(idx, idx2) and np.array_equal(dist, dist2)
    for j in range(ns):
        rc, i1, d1 = LR.call_knn(xf, d, n, xsf[j * d:(j + 1) * d].copy(), 1, m, scale)
        assert rc == nat.OK and np.array_equal(i1[0], idx[j]) and np.array_equal(d1[0], dist[j]), j
    rc, iw, dw = LR.call_knn(xf, d, n, xsf, ns, m, scale, ld=m + 3)                 # a wider pitch: the gap keeps the caller's values
    assert rc == nat.OK and np.array_equal(iw[:, :m], idx) and np.array_equal(dw[:, :m], dist)
    assert (iw[:, m:] == -7).all() and (dw[:, m:] == -7.0).all()
    rc, io, do = LR.call_knn(xf, d, n, xsf, ns, m, scale, want_dist=False)         # without dist_out
    assert rc == nat.OK and do is None and np.array_equal(io, idx)
    xd, xsd = torch.from_numpy(xf).cuda(), torch.from_numpy(xsf).cuda()
    for ld in (m, m + 3):
        it = torch.full((ns, ld), -7, dtype=torch.int32, device="cuda")
        dt = torch.full((ns, ld), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rc, _, _ = LR.call_knn(xd, d, n, xsd, ns, m, scale, ld=ld, idx=it, dist=dt)
        assert rc == nat.OK, nat.last_error()
        ih, dh = it.cpu().numpy(), dt.cpu().numpy()
        assert np.array_equal(ih[:, :m], idx) and np.array_equal(dh[:, :m], dist)
        assert (ih[:, m:] == -7).all() and (dh[:, m:] == -7.0).all()
    rc, ih, dh = LR.call_knn(xd, d, n, xsf, ns, m, scale)                           # device X, host X_star and outputs
    assert rc == nat.OK and np.array_equal(ih, idx) and np.array_equal(dh, dist)


def test_wide_points_take_several_coordinate_chunks():
    """d = 37: three staged chunks of coordinates, the last of five; the partial sums carry over in order"""
    rng = np.random.default_rng(5)
    d, n, ns, m = 37, 700, 40, 20
    X, Xs = rng.uniform(-1, 1, (d, n)), rng.uniform(-1, 1, (d, ns))
    Xs[:, 0] = X[:, 3]
    scale = np.linspace(0.5, 1.5, d)
    for sc in (None, scale):
        order, sdist = LR.knn_order(X, Xs, sc)
        assert LR.smallest_gaps(sdist, m).min() >= 1e-9
        rc, idx, dist = LR.call_knn(LR.flat(X), d, n, LR.flat(Xs), ns, m, sc)
        assert rc == nat.OK, nat.last_error()
        assert np.array_equal(idx, order[:, :m])
        assert (np.abs(dist - sdist[:, :m]) <= (d + 4) * U * sdist[:, :m]).all()
        assert idx[0, 0] == 3 and dist[0, 0] == 0.0


def test_the_python_wrapper():
    X, Xs = LR.knn_data(3, 1000)
    idx, dist = knn(X, Xs[:, :50], 10, scale=LR.knn_scale(3))
    order, sdist = LR.knn_reference(3, 1000, True)
    assert idx.shape == (50, 10) and np.array_equal(idx, order[:50, :10])
    assert np.allclose(dist, sdist[:50, :10], rtol=1e-14, atol=0)


def test_argument_errors():
    X, Xs = LR.knn_data(3, 100)
    xf, xsf = LR.flat(X), LR.flat(Xs)
    lib, ctx = nat.lib(), nat.default_context()
    idx, dist = np.zeros((4, 8), dtype=np.intc), np.zeros((4, 8))

    def bad(rc, word):
        assert rc == nat.ERR_ARG and word in nat.last_error(), (rc, nat.last_error())

    bad(lib.gprc_dev_knn(None, xf.ctypes.data, 3, 100, xsf.ctypes.data, 4, None, 8, idx.ctypes.data, dist.ctypes.data, 8), "null context")
    bad(lib.gprc_dev_knn(ctx.handle, None, 3, 100, xsf.ctypes.data, 4, None, 8, idx.ctypes.data, dist.ctypes.data, 8), "null input")
    bad(lib.gprc_dev_knn(ctx.handle, xf.ctypes.data, 3, 100, None, 4, None, 8, idx.ctypes.data, dist.ctypes.data, 8), "null input")
    bad(lib.gprc_dev_knn(ctx.handle, xf.ctypes.data, 3, 100, xsf.ctypes.data, 4, None, 8, None, dist.ctypes.data, 8), "null output")
    for m in (0, 101, 129):
        bad(LR.call_knn(xf, 3, 100, xsf, 4, m, ld=200)[0], "outside 1 .. min(n, 128)")
    bad(LR.call_knn(xf, 3, 100, xsf, 4, 8, ld=7)[0], "ld_out < m")
    bad(LR.call_knn(xf, 3, 2 ** 31, xsf, 4, 8)[0], "2^31")
    bad(LR.call_knn(xf, 0, 100, xsf, 4, 8)[0], "d < 1")
    for sc in ([1.0, 0.0, 1.0], [1.0, -2.0, 1.0], [1.0, np.inf, 1.0], [np.nan, 1.0, 1.0]):
        bad(LR.call_knn(xf, 3, 100, xsf, 4, 8, scale=sc)[0], "scale")
    rc, i0, d0 = LR.call_knn(xf, 3, 100, xsf, 0, 8)                                  # no test points: nothing to do
    assert rc == nat.OK and (i0 == -7).all() and (d0 == -7.0).all()
