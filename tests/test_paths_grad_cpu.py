"""The reference of the sample paths' gradients (tests/paths_grad_ref.py) and the maximiser (sampling.maximize_paths) judged on the
CPU.  No GPU.

1. The float64 reference of the gradient against its longdouble twin on the very inputs of tests/test_gpu_paths_grad.py (paths_ref's
   eight cases, the last test point a training point), gated at TOL / 100 as tests/test_paths_cpu.py gates the values; and the twin
   against central differences of the longdouble path.  The step: with u = 2^-64 the differences carry a rounding of about
   u |f| / h and a truncation of h^2 |f'''| / 6; the shortest scale of these problems is 0.5 (length scales, and frequencies of about
   1 / (2 pi l) cycles), so |f'''| is a few |f'| / 0.25 and h = 1e-6 puts both terms near 1e-12 |f'|: gated at 1e-10, two orders above
   that estimate for the constants it leaves out, and two orders below what h = 1e-9 in float64 would reach.
   Measured here: twin <= 3.9e-14 on all eight cases (the training point alone likewise); differences at h = 1e-6 <= 2.7e-11 (d = 20),
   <= 1.1e-11 for d <= 3.
2. The componentwise bounds of the two gradient products (tests/test_gpu_paths_grad.py derives them): numpy's own float64 product lies
   inside them against the twin.  Measured: worst ratio 0.019 over the six product problems.
3. maximize_paths on the numpy evaluator, the two problems of paths_grad_ref.MAXIMA, seeds 0-2: every path's best value reaches its
   maximum over the grid (20 001 points; 401 x 401) up to 1e-10 max|F|, the best points' projected-gradient norms are <= 1e-6, every
   candidate is inside the box, and a seed gives the same bits twice.  Measured: worst (grid max - best) / max|F| 1.6e-15 (in four of
   the six cases the ascent ends above the grid's best point); worst projected gradient of a best point 9.9e-9; 10-11 evaluations at
   d = 1, 51-84 at d = 2, every candidate converged to 1e-8.
"""
import functools

import numpy as np
import pytest

import paths_grad_ref as G
import paths_ref as R
from conftest import TOL
from gprc_amd.sampling import maximize_paths
from pred_grad_ref import nerr

LD = np.longdouble
H_DIFF = 1e-6
DIFF_TOL = 1e-10


@pytest.mark.parametrize("index", range(len(R.CASES)), ids=[R.case_id(i) for i in range(len(R.CASES))])
def test_float64_gradient_against_its_twin_and_central_differences(index):
    name, par, *_ = R.CASES[index]
    X, y, Xs, nu, phase, W, E = G.problem(index)
    F, dF, U = G.paths_grad(name, par, X, y, R.NOISE, nu, phase, W, E, Xs)
    Fl, dFl, Ul = G.paths_grad(name, par, X, y, R.NOISE, nu, phase, W, E, Xs, LD)
    assert dF.shape == (Xs.shape[1], W.shape[1], X.shape[0])
    et = nerr(dF.astype(LD), dFl)
    cd = G.central_differences(name, par, X, nu, phase, W, Ul, Xs, H_DIFF)
    ed = nerr(cd, dFl)
    at = nerr(dF[-1].astype(LD), dFl[-1])                            # the training point alone
    print("paths_grad_ref %s: twin %.2e, at the training point %.2e; differences at h = %g: %.2e" % (R.case_id(index), et, at, H_DIFF, ed))
    assert np.isfinite(dF).all()
    assert max(et, at) <= 0.01 * TOL
    assert ed <= DIFF_TOL


@pytest.mark.parametrize("index", range(len(R.PRODUCTS)), ids=["%d-%s" % (i, p[1] or p[0]) for i, p in enumerate(R.PRODUCTS)])
def test_float64_gradient_products_lie_inside_their_bounds(index):
    out, bound = G.product_grad_reference(index)
    twin, _ = G.product_grad_reference(index, LD)
    ratio = float((np.abs(out.astype(LD) - twin) / bound).max())
    print("gradient product %d %s: worst |float64 - longdouble| / bound %.3f" % (index, R.PRODUCTS[index][:2], ratio))
    assert ratio <= 1.0


@functools.lru_cache(maxsize=None)
def numpy_paths(which, seed):
    """(evaluator, grid maxima per path, max |F| on the grid) of a maximisation problem on the float64 reference; computed once"""
    m = G.MAXIMA[which]
    X, y, nu, phase, W, E = G.maxima_problem(which, seed)
    U = R.paths(m["name"], m["par"], X, y, m["noise"], nu, phase, W, E, X[:, :1])[1]

    def eval_grad(P):
        return G.values(m["name"], m["par"], X, nu, phase, W, U, P), G.grad(m["name"], m["par"], X, nu, phase, W, U, P)

    grid = G.maxima_grid(which)
    Fg = np.vstack([G.values(m["name"], m["par"], X, nu, phase, W, U, grid[:, i:i + 20000]) for i in range(0, grid.shape[1], 20000)])
    return eval_grad, Fg.max(axis=0), float(np.abs(Fg).max())


@pytest.mark.parametrize("seed", G.MAXIMA_SEEDS)
@pytest.mark.parametrize("which", range(len(G.MAXIMA)), ids=["d1-sqrexp", "d2-matern52_ard"])
def test_maximize_paths_reaches_the_grid_maximum_of_every_path(which, seed):
    m = G.MAXIMA[which]
    eval_grad, grid_max, fmax = numpy_paths(which, seed)
    lower, upper = np.full(m["d"], m["box"][0]), np.full(m["d"], m["box"][1])
    res = maximize_paths(eval_grad, lower, upper, m["S"], n_starts=m["starts"], rng=np.random.default_rng(seed))
    again = maximize_paths(eval_grad, lower, upper, m["S"], n_starts=m["starts"], rng=np.random.default_rng(seed))
    short, pg, inside = G.check_maxima(res, grid_max, fmax, lower, upper)
    print("maximize_paths %s seed %d: %d evaluations; worst (grid max - best) / max|F| %.2e; worst projected gradient of a best point %.2e; "
          "candidates converged %d of %d" % (m["name"], seed, res.n_evals, short, pg, int((res.pg <= 1e-8).sum()), res.pg.size))
    assert res.x_best.shape == (m["d"], m["S"]) and res.x.shape == (m["d"], m["S"] * m["starts"])
    assert short <= 1e-10
    assert pg <= 1e-6
    assert inside
    assert all(np.array_equal(a, b) for a, b in zip(res, again))


def test_maximize_paths_takes_given_starts_and_refuses_bad_boxes():
    eval_grad, _, _ = numpy_paths(0, 0)
    x0 = np.linspace(-2.5, 2.5, 16).reshape(1, 16)                   # two starts a path; outside the box: clipped
    res = maximize_paths(eval_grad, [-2.0], [2.0], 8, n_starts=2, x0=x0, max_iter=0)
    assert res.n_evals == 1 and np.array_equal(res.x, np.clip(x0, -2.0, 2.0))
    F = eval_grad(res.x)[0]
    assert np.array_equal(res.f, F[np.arange(16), np.arange(16) % 8])
    one = maximize_paths(lambda P: tuple(v[:, :1] for v in eval_grad(P)), [-2.0], [2.0], 1, n_starts=5, rng=np.random.default_rng(0))   # a single path
    assert one.x.shape == (1, 5) and one.x_best.shape == (1, 1) and one.f_best[0] == one.f.max() and (one.pg <= 1e-8).all()
    for lo, hi in (([0.0], [0.0]), ([0.0, 0.0], [1.0]), ([0.0], [np.inf])):
        with pytest.raises(ValueError):
            maximize_paths(eval_grad, lo, hi, 8)
