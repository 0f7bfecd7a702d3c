"""Records what the five optimisers of gprc_amd.fit (optimize, optimize_gpc, optimize_sparse, optimize_iterative,
optimize_multistart) do on closed-form objectives: every returned field except `func`, and the full sequence of points at
which the objective hook was called.  With a hook (`value_and_grad` / `value_and_grad_batch`) the optimisers never load
the native library, so the record is produced and checked without a GPU; tests/test_optimizers_cpu.py replays the same
cases and requires equality, every float bit for bit (they are stored as float.hex()).

Each objective is a smooth concave function of log(theta) -- c - sum_i a_i (log theta_i - m_i)^2, the noise and the
inducing points likewise -- with its analytic gradient; regions of the parameter space raise or flag what the native
objectives raise or flag, so that the sentinel and the raising paths are walked.

    python tests/golden/make_optimizer_record.py        # rewrites tests/golden/optimizer_iterates.json

The record is a statement about behaviour that refactors must keep: regenerate it only from a commit whose behaviour is
meant to be the new truth, and say from which.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

X = np.array([[0.0, 0.3, 0.5, 0.8, 1.0], [1.0, 0.2, 0.7, 0.1, 0.6]])   # d = 2; the hooks never look at the data
Y = np.array([0.1, -0.4, 0.3, 0.9, -0.2])
Z0 = np.array([[0.1, 0.5, 0.9], [0.2, 0.6, 0.4]])                       # m = 3 inducing points
Z_TARGET = np.array([[0.3, 0.4, 0.7], [0.1, 0.8, 0.5]])
STARTS = np.array([[1.0, 1.0], [0.5, 1.5], [2.0, 0.7], [0.3, 0.4]])     # S = 4


def enc(v):
    """JSON form of a result: floats as float.hex(), arrays and tuples as nested lists"""
    if v is None or isinstance(v, (str, bool)):
        return v
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return float(v).hex()
    if isinstance(v, np.ndarray):
        return enc(v.tolist())
    if isinstance(v, (list, tuple)):
        return [enc(t) for t in v]
    raise TypeError(type(v))


def quad(t, a, m):
    """(value, d value / d t) of -sum a (log t - m)^2"""
    t = np.asarray(t, dtype=np.float64)
    lt = np.log(t)
    return float(-np.sum(a * (lt - m) ** 2)), -2.0 * a * (lt - m) / t


class Objective:
    """c - sum_i a_i (log theta_i - m_i)^2 - a_n (log noise - m_n)^2 - b sum (Z - Z_TARGET)^2 with its gradient; `calls` is the
    sequence of arguments it was asked at.  fail(theta) -> an exception to raise (or, batched, an info > 0 to flag) or None."""

    def __init__(self, a, m, a_noise=1.5, m_noise=-1.0, b=2.0, fail=None, push=None):
        self.a, self.m = np.asarray(a, dtype=np.float64), np.asarray(m, dtype=np.float64)
        self.a_noise, self.m_noise, self.b, self.fail, self.push = a_noise, m_noise, b, fail, push
        self.calls = []

    def value_grad(self, theta, noise):
        v, g = quad(theta, self.a[:len(theta)], self.m[:len(theta)])
        if noise > 0:
            vn, gn = quad([noise], self.a_noise, self.m_noise)
        else:
            vn, gn = 0.0, np.zeros(1)
        return 3.0 + v + vn, np.concatenate([g, gn])

    def check(self, theta):
        err = self.fail(theta) if self.fail else None
        if isinstance(err, Exception):
            raise err
        return err

    def regression(self, theta, noise):            # optimize, optimize_iterative: (value, grad), noise last
        self.calls.append(enc([theta, noise]))
        self.check(theta)
        return self.value_grad(theta, noise)

    def with_se(self, theta, noise):               # optimize_iterative: (value, grad, se)
        val, g = self.regression(theta, noise)
        return val, g, 0.01 * abs(val) + 0.001

    def classification(self, theta):               # optimize_gpc: (value, grad), no noise
        self.calls.append(enc([theta]))
        self.check(theta)
        val, g = self.value_grad(theta, 0.0)
        return val, g[:-1]

    def sparse(self, theta, noise, Zc):            # optimize_sparse: (value, grad, dZ)
        self.calls.append(enc([theta, noise, Zc]))
        self.check(theta)
        val, g = self.value_grad(theta, noise)
        Zc = np.asarray(Zc, dtype=np.float64)
        if self.push is not None:                  # no curvature in Z, one coordinate pushed upwards by a (finite) slope
            dZ = np.zeros(Zc.shape)
            dZ[1, 2] = self.push
            return val, g, dZ
        return val - self.b * float(np.sum((Zc - Z_TARGET) ** 2)), g, -2.0 * self.b * (Zc - Z_TARGET)

    def batch(self, thetas, noises):               # optimize_multistart: (values, grads, infos)
        self.calls.append(enc([thetas, noises]))
        vals, grads, infos = np.full(len(thetas), np.nan), np.full((len(thetas), thetas.shape[1] + 1), np.nan), np.zeros(len(thetas), dtype=np.intc)
        for r, (theta, nz) in enumerate(zip(thetas, noises)):
            info = self.fail(theta) if self.fail else None
            if info:
                infos[r] = info
            else:
                vals[r], grads[r] = self.value_grad(theta, float(nz))
        return vals, grads, infos


def fields(r):
    """every returned field except func (and multistart's `all`, which the caller unfolds)"""
    return {k: enc(v) for k, v in r.items() if k not in ("func", "all")}


def run(call, objective):
    """the record of one optimiser call: its fields, or the exception that left it, and the objective's calls"""
    try:
        r = call()
        out = {"result": fields(r)}
        if "all" in r:
            out["all"] = [fields(q) for q in r["all"]]
    except Exception as e:   # noqa: BLE001  (the type and the text are what is recorded)
        out = {"raised": [type(e).__name__, str(e)]}
    out["calls"] = objective.calls
    return out


def far(bound):
    """the native objectives' failures, in the region theta_1 > bound (the first line-search step of the cases below enters it)"""
    from gprc_amd import NotPositiveDefinite
    return {"npd": lambda th: NotPositiveDefinite(3) if th[0] > bound else None,
            "arith": lambda th: ArithmeticError("the objective failed") if th[0] > bound else None,
            "info": lambda th: 3 if th[0] > bound else 0}


def cases():
    """name -> (call, objective), in a fixed order"""
    import gprc_amd  # noqa: F401  (alias loader)
    F = sys.modules["gprc_amd.fit"]
    a2, m2 = [2.0, 1.0], [1.0, -0.5]     # the first step from theta = (1, 1) goes to log theta_1 = 4: theta_1 = 54.6
    out = {}

    def add(name, make):
        out[name] = make

    def single(fn, kind, *args, fail=None, a=a2, m=m2, push=None, **kw):
        def make():
            ob = Objective(a, m, fail=fail, push=push)
            hook = getattr(ob, kind)
            return (lambda: fn(*args, value_and_grad=hook, **kw)), ob
        return make

    add("optimize/noise_on", single(F.optimize, "regression", X, Y, 0.1, "gammaexp", (1.0, 1.0)))
    add("optimize/noise_off", single(F.optimize, "regression", X, Y, 0.1, "gammaexp", (1.0, 1.0), optimize_noise=False))
    add("optimize/noise_zero", single(F.optimize, "regression", X, Y, 0, "gammaexp", (1.0, 1.0)))
    add("optimize/default_start", single(F.optimize, "regression", X, Y, 0.1, "rationalquadratic"))
    add("optimize/ard_start", single(F.optimize, "regression", X, Y, 0.1, "sqrexp_ard", [0.7, 1.3]))
    add("optimize/ard_default_start", single(F.optimize, "regression", X, Y, 0.1, "matern52_ard"))
    add("optimize/sentinel_not_positive_definite", single(F.optimize, "regression", X, Y, 0.1, "gammaexp", (1.0, 1.0), fail=far(20.0)["npd"]))
    add("optimize/sentinel_arithmetic_error", single(F.optimize, "regression", X, Y, 0.1, "gammaexp", (1.0, 1.0), fail=far(20.0)["arith"]))
    add("optimize/sentinel_exp_overflow", single(F.optimize, "regression", X, Y, 0.1, "gammaexp", (1.0, 1.0), a=[400.0, 1.0]))
    add("optimize/first_point_not_positive_definite", single(F.optimize, "regression", X, Y, 0.1, "gammaexp", (25.0, 1.0), fail=far(20.0)["npd"]))
    add("optimize/first_point_arithmetic_error", single(F.optimize, "regression", X, Y, 0.1, "gammaexp", (25.0, 1.0), fail=far(20.0)["arith"]))
    add("optimize/maxit_reached", single(F.optimize, "regression", X, Y, 0.1, "gammaexp", (1.0, 1.0), maxit=3))
    add("optimize/bad_start", single(F.optimize, "regression", X, Y, 0.1, "gammaexp", (1.0, -1.0)))

    add("optimize_gpc/plain", single(F.optimize_gpc, "classification", X, np.sign(Y), "gammaexp", (1.0, 1.0)))
    add("optimize_gpc/default_ard_start", single(F.optimize_gpc, "classification", X, np.sign(Y), "sqrexp_ard"))
    add("optimize_gpc/sentinel", single(F.optimize_gpc, "classification", X, np.sign(Y), "gammaexp", (1.0, 1.0), fail=far(20.0)["arith"]))
    add("optimize_gpc/bad_start", single(F.optimize_gpc, "classification", X, np.sign(Y), "gammaexp", (0.0, 1.0)))

    for oz in (True, False):
        for on in (True, False):
            add("optimize_sparse/Z_%s_noise_%s" % ("on" if oz else "off", "on" if on else "off"),
                single(F.optimize_sparse, "sparse", X, Y, 0.1, "gammaexp", Z0, (1.0, 1.0), optimize_Z=oz, optimize_noise=on))
    add("optimize_sparse/default_start_vector_Z", single(F.optimize_sparse, "sparse", X, Y, 0.1, "sqrexp", Z0.ravel(order="F")))
    add("optimize_sparse/sentinel", single(F.optimize_sparse, "sparse", X, Y, 0.1, "gammaexp", Z0, (1.0, 1.0), fail=far(20.0)["npd"]))
    Zfar = Z0.copy()
    Zfar[1, 2] = 1.5e308           # the first step adds the slope 1e308 to it: inf, the sentinel; the shorter ones stay finite
    add("optimize_sparse/inducing_point_not_finite", single(F.optimize_sparse, "sparse", X, Y, 0.1, "gammaexp", Zfar, (1.0, 1.0), push=1e308))
    add("optimize_sparse/bad_start", single(F.optimize_sparse, "sparse", X, Y, 0.1, "gammaexp", Z0, (np.inf, 1.0)))

    add("optimize_iterative/with_se", single(F.optimize_iterative, "with_se", X, Y, 0.1, "gammaexp", (1.0, 1.0)))
    add("optimize_iterative/without_se", single(F.optimize_iterative, "regression", X, Y, 0.1, "gammaexp", (1.0, 1.0)))
    add("optimize_iterative/noise_off_sentinel", single(F.optimize_iterative, "with_se", X, Y, 0.1, "matern32_ard", optimize_noise=False,
                                                        fail=far(20.0)["arith"], a=[2.0, 1.0], m=[1.0, -0.5]))
    add("optimize_iterative/bad_start", single(F.optimize_iterative, "regression", X, Y, 0.1, "gammaexp", (np.nan, 1.0)))

    def multi(*args, fail=None, a=a2, m=m2, **kw):
        def make():
            ob = Objective(a, m, fail=fail)
            return (lambda: F.optimize_multistart(*args, value_and_grad_batch=ob.batch, **kw)), ob
        return make

    add("optimize_multistart/explicit_starts", multi(X, Y, 0.1, "gammaexp", STARTS))
    add("optimize_multistart/default_starts", multi(X, Y, 0.1, "rationalquadratic", n_starts=4, rng=np.random.default_rng(11)))
    add("optimize_multistart/default_starts_ard_noise_off", multi([X] * 4, [Y] * 4, 0.1, "sqrexp_ard", n_starts=4, rng=np.random.default_rng(5),
                                                                   optimize_noise=False))
    add("optimize_multistart/noise_zero", multi(X, Y, 0, "gammaexp", STARTS))
    add("optimize_multistart/sentinel_for_one_instance", multi(X, Y, 0.1, "gammaexp", STARTS, fail=far(20.0)["info"]))
    add("optimize_multistart/first_point_not_positive_definite", multi(X, Y, 0.1, "gammaexp", np.vstack([STARTS[:2], [[25.0, 1.0]], STARTS[3:]]),
                                                                       fail=far(20.0)["info"]))
    # a = 400: the first step of three of the four starts is longer than 709, their exp(z) overflows: the sentinel for those rows
    add("optimize_multistart/exp_out_of_range_rows", multi(X, Y, 0.1, "gammaexp", STARTS, a=STEEP))
    # from theta_1 = 1e-300 the value is below -10000: the sentinel of the overflowing first step is ACCEPTED, and the gradient
    # vmmin then asks for at that point raises, as it does in `optimize`
    add("optimize_multistart/out_of_range_at_a_gradient", multi(X, Y, 0.1, "gammaexp", np.vstack([STARTS[:3], TINY]), a=[1.1, 1.0]))
    add("optimize_multistart/maxit_zero", multi(X, Y, 0.1, "gammaexp", STARTS, maxit=0))
    add("optimize_multistart/maxit_reached", multi(X, Y, 0.1, "gammaexp", STARTS, maxit=3))
    add("optimize_multistart/bad_start", multi(X, Y, 0.1, "gammaexp", [[1.0, 1.0], [1.0, -2.0]]))

    for variant, start, kw in promise_variants():
        fail = kw.pop("fail", None)
        add("promise/optimize/" + variant, single(F.optimize, "regression", X, Y, 0.1, "gammaexp", start, fail=fail and far(20.0)["npd"], **kw))
        add("promise/optimize_multistart/" + variant, multi(X, Y, 0.1, "gammaexp", [start], fail=fail and far(20.0)["info"], **kw))
    return out


STEEP = [400.0, 1.0]
TINY = np.array([[1e-300, 1.0]])


def promise_variants():
    """(name, start, keywords) of what optimize_multistart's docstring promises: one start runs exactly what `optimize` runs from it --
    the same fields, the same points in the same order.  Every start plain, with the failing region (an exception there, info > 0
    here) and with the overflowing steps; the start whose gradient call raises; the noise kept fixed."""
    for i, s in enumerate(STARTS):
        yield "start%d" % i, s, {}
        yield "start%d_failing_region" % i, s, {"fail": True}
        yield "start%d_overflow" % i, s, {"a": STEEP}
    yield "raises_at_a_gradient", TINY[0], {"a": [1.1, 1.0]}
    yield "first_point_fails", np.array([25.0, 1.0]), {"fail": True}
    yield "noise_off", STARTS[1], {"optimize_noise": False}
    yield "maxit_reached", STARTS[3], {"maxit": 3}


def record():
    out = {}
    for name, make in cases().items():
        call, ob = make()
        out[name] = run(call, ob)
    return out


if __name__ == "__main__":
    rec = record()
    with open(os.path.join(HERE, "optimizer_iterates.json"), "w") as f:
        json.dump({"floats": "float.hex()", "cases": rec}, f, indent=0, sort_keys=True)
    for name, r in rec.items():
        print(name, "->", r.get("raised") or {k: r["result"][k] for k in ("counts", "convergence") if k in r["result"]}, len(r["calls"]), "calls")
