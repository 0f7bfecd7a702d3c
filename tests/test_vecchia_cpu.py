"""The Vecchia likelihood without a GPU: the numpy model of the device kernel's algorithm (tests/vecchia_ref.py) against the
difference-of-marginals reference and against np.longdouble at every shape the GPU tests use; the reference gradient against central
differences with frozen neighbours; m >= n - 1 is the exact likelihood; the validity of the search inputs (no two of a point's first
m + 1 prefix distances nearly tied); fit.optimize_local on the numpy model; the argument errors of the Python layer."""
import sys

import numpy as np
import pytest

import ard_grad_ref
import local_ref as LR
import vecchia_ref as V
from conftest import TOL, nerr
from gprc_amd import local as L

F = sys.modules["gprc_amd.fit"]   # the module: the package attribute `fit` is the function


@pytest.mark.parametrize("m_cond", V.M_CONDS)
@pytest.mark.parametrize("case", V.CASES)
def test_the_kernel_s_algorithm_against_the_difference_of_marginals(case, m_cond):
    """L only, z, w, a, a', G: the same conditionals and gradient as two closed-form models, to the bounds the device is held to"""
    name, theta, X, y, noise = V.case(case)
    idx, _ = V.case_neighbours(case, m_cond)
    cond_ref, grad_ref = V.case_reference(case, m_cond)
    cond, grad = V.vecchia_sum(V.model_cond, name, theta, X, y, noise, idx)
    assert np.abs(cond - cond_ref).max() <= TOL * max(1.0, np.abs(cond_ref).max())
    assert abs(cond.sum() - cond_ref.sum()) <= TOL * np.abs(cond_ref).sum()
    assert nerr(grad.sum(0), grad_ref.sum(0)) <= TOL
    if V.block_also(case):
        assert nerr(grad.sum(0)[:-1], grad_ref.sum(0)[:-1]) <= TOL


@pytest.mark.parametrize("case", V.CASES)
def test_the_float64_model_against_longdouble(case):
    """a few points per size, among them the largest models: float64 agrees with np.longdouble far inside TOL"""
    name, theta, X, y, noise = V.case(case)
    for m_cond in V.M_CONDS:
        idx, _ = V.case_neighbours(case, m_cond)
        for i in (0, 1, m_cond, 150, 299):
            nb = [j for j in idx[i] if j >= 0]
            c64, g64 = V.model_cond(name, theta, X, y, noise, nb, i)
            cl, gl = V.model_cond(name, theta, X, y, noise, nb, i, np.longdouble)
            assert abs(c64 - cl) <= 1e-12 * max(1.0, abs(cl))
            assert np.abs(g64 - gl).max() <= 1e-11 * max(1.0, np.abs(gl).max())


@pytest.mark.parametrize("case", V.CASES)
def test_the_reference_gradient_against_central_differences(case):
    name, theta, X, y, noise = V.case(case)
    m_cond = 17
    idx, _ = V.case_neighbours(case, m_cond)
    grad = V.case_reference(case, m_cond)[1].sum(0)

    def value(t, nz):
        return V.vecchia_sum(V.model_cond, name, t, X, y, nz, idx)[0].sum()      # frozen neighbours

    h = 1e-5
    for k in range(len(theta) + 1):
        tp, tm, np_, nm = theta.copy(), theta.copy(), noise, noise
        if k < len(theta):
            tp[k] += h * theta[k]
            tm[k] -= h * theta[k]
            step = 2 * h * theta[k]
        else:
            np_, nm, step = noise + h * noise, noise - h * noise, 2 * h * noise
        fd = (value(tp, np_) - value(tm, nm)) / step
        assert abs(fd - grad[k]) <= 1e-6 * max(1.0, np.abs(grad).max()), (k, fd, grad[k])


@pytest.mark.parametrize("case", V.CASES)
def test_every_predecessor_is_the_exact_likelihood(case):
    name, theta, X, y, noise = V.case(case, 100)
    cond, grad = V.case_reference(case, 127, 100)
    want, want_g = ard_grad_ref.logp_grad(name, theta, X, y, noise)
    assert abs(cond.sum() - want) <= TOL * np.abs(cond).sum()
    assert nerr(grad.sum(0), want_g) <= TOL


@pytest.mark.parametrize("scaled", [False, True], ids=["euclid", "scaled"])
@pytest.mark.parametrize("d", LR.KNN_DIMS)
def test_no_two_prefix_distances_of_the_search_inputs_are_nearly_tied(d, scaled):
    """queries against their own predecessors on local_ref.knn_data's master sets, the first m + 1 = 129 distances: the device's sums are
    within (d + 4) 2.3e-16 of the reference's, so with these gaps index equality is a fair demand"""
    gap = V.smallest_prefix_gap(V.before_reference(d, LR.N_MASTER, scaled)[1], 128)
    print(f"knn_before inputs d={d} scaled={scaled}: smallest relative gap {gap:.3e}")
    assert gap > 1e-12


@pytest.mark.parametrize("case", V.CASES)
def test_the_likelihood_cases_have_no_near_ties_either(case):
    name, theta, X, _, _ = V.case(case)
    gap = V.smallest_prefix_gap(V.knn_before_ref(X, 128, LR.metric_of(name, theta))[1], 127)
    assert gap > 1e-12
    name, theta, X, _, _ = V.case(case, 100)
    assert V.smallest_prefix_gap(V.knn_before_ref(X, 99, LR.metric_of(name, theta))[1], 99) > 1e-12


def test_knn_before_ref_on_a_case_small_enough_to_check_by_hand():
    X = np.array([[0.0, 1.0, 3.0, 1.0, 0.9]])
    idx, dist = V.knn_before_ref(X, 3)
    assert idx.tolist() == [[-1, -1, -1], [0, -1, -1], [1, 0, -1], [1, 0, 2], [1, 3, 0]]      # the tie of point 4 goes to the lower index
    assert np.isposinf(dist[0]).all() and dist[3, 0] == 0.0 and np.allclose(dist[4], [0.01, 0.01, 0.81])


def test_optimize_local_on_the_numpy_model():
    """n = 400, d = 2, m = 15, matern52_ard through value_and_grad: runs on the CPU, raises the value, returns the siblings' keys and its
    own, and prepares once per round"""
    X, y, _ = V.optimiser_data(400, seed=7)
    perm = L.vecchia_order(X, "random", seed=3)
    assert sorted(perm) == list(range(400)) and np.array_equal(L.vecchia_order(X, "given"), np.arange(400))
    assert np.array_equal(perm, L.vecchia_order(X, seed=3)) and not np.array_equal(perm, L.vecchia_order(X, seed=4))
    hook = V.ArdVecchia("matern52_ard", X[:, perm], y[perm], 15)
    start = np.array([1.0, 1.0])
    hook.prepare(start, 0.1)
    before = hook(start, 0.1)[0]
    hook.prepares = 0
    r = F.optimize_local(X, y, 0.1, "matern52_ard", start, m=15, order="random", seed=3, value_and_grad=hook)
    assert set(r) == {"par", "noise", "value", "counts", "convergence", "func", "m", "order", "rounds"}
    assert r["rounds"] == 2 and hook.prepares == 2 and r["m"] == 15 and r["order"] == "random"
    assert r["value"] > before + 1.0 and r["convergence"] in (0, 1) and len(r["par"]) == 2 and r["noise"] > 0
    assert r["func"].gprc_kernel[0] == V.kernel_id("matern52_ard")
    one = F.optimize_local(X, y, 0.1, "matern52_ard", start, m=15, order=perm, rounds=1, optimize_noise=False, value_and_grad=hook)
    assert one["rounds"] == 1 and hook.prepares == 3 and one["noise"] == 0.1 and one["order"] == "custom" and one["value"] > before
    assert F.optimize_local(X, y, 0.1, "matern52", [1.0], m=15, order="given", maxit=1,
                            value_and_grad=lambda t, nz: (0.0, np.zeros(2)))["rounds"] == 1          # an isotropic kernel: one pass


def test_a_failed_evaluation_is_never_accepted_below_the_sentinel():
    """an objective near -50 000 (n = 2^20 gives -3e5) whose first full step lands where the evaluation fails: the siblings' sentinel
    -10000 would look like an improvement there; optimize_local must step back instead and reach the maximum"""
    X, y, _ = V.optimiser_data(30, seed=2)
    calls = []

    def hook(theta, nz):
        z = np.log(np.concatenate([theta, [nz]]))
        calls.append(z)
        if np.abs(z).max() > 5:
            raise ArithmeticError("not positive definite")
        c = np.array([0.3, -0.2, -2.0])
        return -50000.0 - 1e4 * float(((z - c) ** 2).sum()), -2e4 * (z - c) / np.exp(z)

    r = F.optimize_local(X, y, 0.1, "matern52_ard", [1.0, 1.0], m=5, order="given", rounds=1, value_and_grad=hook)
    assert max(np.abs(z).max() for z in calls) > 5                                # the failing region was visited
    assert abs(r["value"] + 50000.0) < 1e-3 and np.allclose(np.log(r["par"]), [0.3, -0.2], atol=1e-4)


def test_argument_errors_of_the_python_layer():
    X, y, _ = V.optimiser_data(30, seed=1)
    hook = lambda t, nz: (0.0, np.zeros(3))   # noqa: E731
    for m in (0, 128, 2.5):
        with pytest.raises(ValueError):
            F.optimize_local(X, y, 0.1, "matern52_ard", m=m, value_and_grad=hook)
    with pytest.raises(ValueError):
        F.optimize_local(X, y, 0.1, "matern52_ard", rounds=0, value_and_grad=hook)
    with pytest.raises(ValueError):
        F.optimize_local(X, y, 0.1, "matern52_ard", order="maxmin", value_and_grad=hook)
    with pytest.raises(ValueError):
        F.optimize_local(X, y, 0.1, "matern52_ard", order=np.zeros(30, dtype=int), value_and_grad=hook)
    with pytest.raises(ValueError):
        F.optimize_local(X, y[:-1], 0.1, "matern52_ard", value_and_grad=hook)
    with pytest.raises(ValueError):
        F.optimize_local(X, y, 0.1, "matern52_ard", [1.0, -1.0], value_and_grad=hook)
    with pytest.raises(KeyError):
        F.optimize_local(X, y, 0.1, "linear", value_and_grad=hook)
    with pytest.raises(ValueError):
        L.vecchia_order(X, "maxmin")
    for kw in (dict(m=0), dict(m=129), dict(m=4, first=-1), dict(m=4, first=29, count=2), dict(m=4, scale=[1.0, -1.0])):
        with pytest.raises(ValueError):
            L.knn_before(X, **kw)
    for name in ("knn_before", "vecchia_order", "vecchia_logp_grad", "optimize_local"):
        import gprc_amd
        assert hasattr(gprc_amd, name) and name in gprc_amd.__all__
    for name in ("vecchia_prepare", "vecchia_logp_grad", "vecchia_neighbours", "vecchia_flagged"):
        assert hasattr(L.LocalGPR, name)
