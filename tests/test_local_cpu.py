"""The numpy references of the local GPR and of the neighbour search (tests/local_ref.py) judged without a GPU, on the inputs of the GPU
tests: the search against an independent per-point sort, the validity of the random inputs (no two of a point's first m + 1 distances
so close that an index comparison would be unfair), the local closed form against the exact GP where they must coincide, the
ordering of the variances, and the Python layer's argument errors and exports."""
import numpy as np
import pytest

import local_ref as LR
from conftest import nerr
from gprc_amd import _native as nat

GAP = 1e-9   # the smallest relative gap among a point's first m + 1 distances that the GPU tests' random inputs must keep


def test_knn_ref_agrees_with_a_stable_sort_per_point():
    for d in LR.KNN_DIMS:
        X, Xs = LR.knn_data(d, 1000)
        for scale in (None, LR.knn_scale(d)):
            idx, dist = LR.knn_ref(X, Xs, 128, scale)
            for j in range(0, Xs.shape[1], 7):
                t = Xs[:, j:j + 1] - X
                if scale is not None:
                    t = t * scale[:, None]
                dj = np.zeros(X.shape[1])
                for c in range(d):
                    dj += t[c] * t[c]
                want = np.argsort(dj, kind="stable")[:128]
                assert np.array_equal(idx[j], want) and np.array_equal(dist[j], dj[want])
    X, Xs, scale = LR.lattice_data()
    idx, dist = LR.knn_ref(X, Xs, 128, scale)
    for j in range(Xs.shape[1]):
        dj = (((Xs[:, j:j + 1] - X) * scale[:, None]) ** 2).sum(0)
        want = np.argsort(dj, kind="stable")[:128]
        assert np.array_equal(idx[j], want) and np.array_equal(dist[j], dj[want])
    assert list(idx[0, :3]) == [10, 200, 411] and not dist[0, :3].any()


def test_the_random_inputs_of_the_gpu_tests_have_no_near_ties():
    worst = 1.0
    for d in LR.KNN_DIMS:
        for scaled in (False, True):
            for n in sorted({n for m in LR.KNN_MS for n in LR.knn_sizes(m)}):
                _, dist = LR.knn_reference(d, n, scaled)
                for m in LR.KNN_MS:
                    if m <= n:
                        worst = min(worst, LR.smallest_gaps(dist, m).min())
    print(f"knn inputs: smallest relative gap among the first m + 1 distances = {worst:.3e}")
    assert worst >= GAP
    worst = 1.0
    for case in LR.PREDICT_CASES:
        name, theta, X, _, _, Xs = LR.predict_case(case)
        _, dist = LR.knn_order(X, Xs, LR.metric_of(name, theta))
        for m in LR.PREDICT_MS + LR.ORDER_MS:
            worst = min(worst, LR.smallest_gaps(dist, m).min())
    name, theta, X, _, _, Xs = LR.predict_case("ard3", 100)
    worst = min(worst, LR.smallest_gaps(LR.knn_order(X, Xs, LR.metric_of(name, theta))[1], 100).min())
    print(f"local predict inputs: smallest relative gap = {worst:.3e}")
    assert worst >= GAP


def test_the_flagged_inputs_touch_only_the_two_coincident_points():
    """of the test points of local_ref.flagged_data only the first two have an appended duplicate among their neighbours, and they have
    it in rank 1, behind its original: every other point's local model is the one of the data without the duplicates"""
    _, _, X, Xdup, _, _, Xs, m = LR.flagged_data()
    idx, dist = LR.knn_ref(Xdup, Xs, m)
    n = X.shape[1]
    assert list(idx[0, :2]) == [7, n] and list(idx[1, :2]) == [11, n + 1] and not dist[:2, :2].any()
    assert (idx[2:] < n).all()
    assert np.array_equal(idx[2:], LR.knn_ref(X, Xs[:, 2:], m)[0])
    assert LR.smallest_gaps(LR.knn_order(X, Xs[:, 2:])[1], m).min() >= GAP


def test_with_every_point_a_neighbour_the_local_form_is_the_exact_gp():
    for case in ("sqrexp", "ard3", "matern52_ard8"):
        name, theta, X, y, noise, Xs = LR.predict_case(case, 100)
        mean, var, idx = LR.local_predict_ref(name, theta, X, y, noise, Xs, 128)
        assert idx.shape == (Xs.shape[1], 100)
        want_m, want_v = LR.exact_ref(name, theta, X, y, noise, Xs)
        assert nerr(mean, want_m) <= 1e-12 and nerr(var, want_v) <= 1e-12


@pytest.mark.parametrize("case", ["sqrexp", "ard3", "matern52_ard8"])
def test_conditioning_on_more_neighbours_cannot_raise_the_variance(case):
    """the neighbour sets are nested: var(m = 16) >= var(32) >= var(64) >= the exact GP's, up to the cancellation in a variance at
    noise >= 1e-2 (1e-9)"""
    vs = [LR.predict_reference(case, m)[1] for m in LR.ORDER_MS] + [LR.exact_reference(case)[1]]
    for a, b in zip(vs, vs[1:]):
        assert (a >= b - 1e-9).all(), float((b - a).max())
    sets = [LR.predict_reference(case, m)[2] for m in LR.ORDER_MS]
    assert np.array_equal(sets[0], sets[1][:, :16]) and np.array_equal(sets[1], sets[2][:, :32])


def test_the_package_exports_the_local_gpr():
    import gprc_amd
    assert callable(gprc_amd.LocalGPR) and callable(gprc_amd.knn)
    assert "LocalGPR" in gprc_amd.__all__ and "knn" in gprc_amd.__all__
    for name in ("gprc_dev_knn", "gprc_lgpr_create", "gprc_lgpr_set_params", "gprc_lgpr_predict", "gprc_lgpr_neighbours", "gprc_lgpr_dims",
                 "gprc_lgpr_free"):
        assert name in nat.PROTOTYPES and hasattr(nat.lib(), name)


def test_argument_errors_that_need_no_device():
    from gprc_amd import LocalGPR, cov_func, knn, linear, sqrexp, sqrexp_ard
    X = np.arange(12.0).reshape(2, 6)
    y = np.arange(6.0)
    k = cov_func(sqrexp, l=1.0)
    for m in (0, 129, -3, 2.5):
        with pytest.raises(ValueError):
            LocalGPR(X, y, 0.1, k, m=m)
        with pytest.raises(ValueError):
            knn(X, X, m)
    with pytest.raises(ValueError):
        LocalGPR(X, y[:5], 0.1, k)                              # length(y) != ncol(X)
    with pytest.raises(ValueError):
        LocalGPR(X, y, 0.1, cov_func(linear, sigma=1.0))        # no batched small-model path
    with pytest.raises(ValueError):
        LocalGPR(X, y, 0.1, cov_func(sqrexp_ard, l=[1.0, 2.0, 3.0]))   # three length scales, two coordinates
    with pytest.raises(TypeError):
        LocalGPR(X, y, 0.1, lambda a, b: 1.0)                   # not a cov_func
    with pytest.raises(ValueError):
        knn(X, np.zeros((3, 4)), 2)                             # rows differ
    with pytest.raises(ValueError):
        knn(X, X, 7)                                            # m > n
    for scale in ([1.0], [1.0, -1.0], [1.0, np.inf], [0.0, 1.0]):
        with pytest.raises(ValueError):
            knn(X, X, 2, scale=scale)
