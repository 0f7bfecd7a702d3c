"""SHA-256 digests of what the small-model family returns on fixed seeded inputs (numpy default_rng(515151)): the kernels that run one
model of at most 128 points per workgroup (csrc/small_model.h) and the iterative GPR's evidence gradient, which shares theta_terms.
  gprc_gpr_batch_logp_grad   the eight gradient kernels on one strided batch of five models, n_b = 1, 16, 17, 127, 128, d = 3; the ARD
                             kernels also at d = 17 and 33 (two and three chunks of their second pass); gammaexp on a model with two
                             identical points (the s = 0 skip); then the same call with grad_out NULL (the value alone: the kernel's
                             early return, W beside L in the slab) and alpha_out given: logp, info, alpha
  gprc_gpr_batch_fit         the same batches (W to the model's store): logp, info, alpha; then gprc_gpr_batch_predict and gprc_gpr_batch_predict_grad at
                             n* = 1 and 33 per model, all outputs and the mean alone; gprc_gpr_batch_loo on the fitted batch
  gprc_gpc_batch_fit         n_b = 1, 17, 128; sqrexp, gammaexp, matern52_ard (d = 8): logq, f_hat, iters, info, and the stored W
                             through one predict_latent (g has no getter: it enters through predict_latent's mean k*^T g)
  the Vecchia likelihood     n = 300, m = 0 (vecchia_prepare takes m >= 1: a data set of ONE point, whose conditional has p = 0), 15, 16, 31, 63, 127; sqrexp, gammaexp, rationalquadratic and
                             matern32_ard (d = 17): value, gradient, the conditionals; the value without the gradient
  LocalGPR / LocalGPC        n = 300, m = 17, 40 test points
  gprc_igpr_logp_grad        n = 300; sqrexp, gammaexp, rationalquadratic, sqrexp_ard (d = 17)
An error status is recorded as its text.  The library is the one GPRC_LIB_SUFFIX selects, so two builds are compared bit for bit by
running it once per build, each in its own process, and comparing the two files:
    GPRC_LIB_SUFFIX=_parent python tools/small_model_digests.py parent.json && python tools/small_model_digests.py change.json && cmp parent.json change.json
(the "lib" entry is left out of the file for that reason and only printed)."""
import hashlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gprc_amd import _native as nat
from gprc_amd import BatchGPR, BatchGPC, IterativeGPR, LocalGPR, LocalGPC
from gprc_amd.fit import _func_of, batch_layout, grad_dict, logp_grad_batch

out = {}
print("library:", os.path.basename(nat.LIB_PATH))
rng = np.random.default_rng(515151)


def h(*arrs):
    m = hashlib.sha256()
    for a in arrs:
        for part in (a if isinstance(a, (list, tuple)) else [a]):
            if part is not None:
                m.update(np.ascontiguousarray(np.asarray(part, dtype=np.float64)).tobytes())
    return m.hexdigest()[:24]


def record(key, f):
    try:
        out[key] = f()
    except Exception as e:   # the status is the output
        out[key] = "error: " + type(e).__name__ + " " + str(e)[:80]


def kfun(name, par):
    return _func_of(name, tuple(float(v) for v in np.atleast_1d(par)))


def points(d, n):
    X = np.asfortranarray(rng.uniform(-2, 2, (d, n)))
    return X, np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)


def theta_of(name, d):
    if name.endswith("_ard"):
        return rng.uniform(0.7, 2.0, d) * np.sqrt(d / 3.0)
    return {"sqrexp": [1.3], "gammaexp": [0.9, 1.5], "rationalquadratic": [1.1, 1.7], "matern32": [1.2], "matern52": [1.4]}[name]


GRAD_KERNELS = ("sqrexp", "gammaexp", "rationalquadratic", "sqrexp_ard", "matern32", "matern52", "matern32_ard", "matern52_ard")
SIZES = (1, 16, 17, 127, 128)

# ---- batched regression: evidence and gradient, fit, predict, predict_grad, LOO
for name in GRAD_KERNELS:
    for d in ((3, 17, 33) if name.endswith("_ard") else (3,)):
        sets = [points(d, n) for n in SIZES]
        Xl, yl = [s[0] for s in sets], [s[1] for s in sets]
        if name == "gammaexp":   # two identical points: the pair the theta sums skip
            Xl[2] = Xl[2].copy(); Xl[2][:, 5] = Xl[2][:, 11]
        thetas = np.array([np.asarray(theta_of(name, d)) * f for f in (1.0, 0.8, 1.25, 0.9, 1.1)])
        noises = np.array([0.05, 0.1, 0.02, 0.2, 0.07])
        tag = f"{name}/d{d}"
        record(f"batch_logp_grad/{tag}", lambda: h(*logp_grad_batch(Xl, yl, noises, name, thetas)))

        def value_alone():   # grad_out NULL, alpha_out given
            B, p = thetas.shape
            Xb, yb, dd, n_max, x_stride, y_stride, n_each = batch_layout(Xl, yl, B)
            logp, alpha, info = np.empty(B), np.zeros((B, 128)), np.zeros(B, dtype=np.intc)
            nat.check(nat.lib().gprc_gpr_batch_logp_grad(nat.default_context().handle, grad_dict[name].kernel_id, B, thetas.ctypes.data, p, p,
                                                         noises.ctypes.data, Xb.ctypes.data, dd, n_max, x_stride, yb.ctypes.data, y_stride,
                                                         n_each.ctypes.data, logp.ctypes.data, None, alpha.ctypes.data, info.ctypes.data))
            return h(logp, info, alpha)
        record(f"batch_logp_value_alone/{tag}", value_alone)

        def fitted():
            with BatchGPR(Xl, yl, noises, name, thetas) as bg:
                res = {"fit": h(bg.logp, bg.info, bg.alpha)}
                for ns in (1, 33):
                    Xs = [np.asfortranarray(rng.uniform(-2, 2, (d, ns))) for _ in SIZES]
                    Xs[1][:, 0] = Xl[1][:, 3]   # a test point equal to a training point: s = 0 exactly
                    res[f"predict/{ns}"] = h(*bg.predict(Xs)) + " " + h(*bg.predict(Xs, var=False))
                    res[f"predict_grad/{ns}"] = h(*bg.predict_grad(Xs)) + " " + h(*bg.predict_grad(Xs, var=False))
                res["loo"] = h(*bg.loo(), bg.loo_score)
                return res
        record(f"batch_fit/{tag}", fitted)

# ---- batched classification
for name, d in (("sqrexp", 3), ("gammaexp", 3), ("matern52_ard", 8)):
    sets = [points(d, n) for n in (1, 17, 128)]
    Xl = [s[0] for s in sets]
    yl = [np.where(s[1] + 0.3 * rng.normal(size=s[1].size) > 0, 1.0, -1.0) for s in sets]
    thetas = np.array([np.asarray(theta_of(name, d)) * f for f in (1.0, 0.8, 1.25)])

    def classified():
        with BatchGPC(Xl, yl, name, thetas) as bc:
            Xs = [np.asfortranarray(rng.uniform(-2, 2, (d, 9))) for _ in Xl]
            return h(bc.logq, bc.f_hat, bc.iters, bc.info, *bc.predict_latent(Xs), *bc.predict_class(Xs))
    record(f"gpc_batch_fit/{name}/d{d}", classified)

# ---- the Vecchia likelihood
for name, d in (("sqrexp", 3), ("gammaexp", 3), ("rationalquadratic", 3), ("matern32_ard", 17)):
    X, y = points(d, 300)
    theta = theta_of(name, d)
    for m in (0, 15, 16, 31, 63, 127):
        def vecchia():
            n = 1 if m == 0 else 300   # a model of one point conditions on nothing
            with LocalGPR(X[:, :n], y[:n], 0.05, kfun(name, theta), m=max(m, 1)) as model:
                used = model.vecchia_prepare(max(m, 1))
                v, g, c = model.vecchia_logp_grad(cond=True)
                v0, _ = model.vecchia_logp_grad(grad=False)
                return h([used, v, v0, model.vecchia_flagged], g, c)
        record(f"vecchia/{name}/d{d}/m{m}", vecchia)

# ---- the local front: the batch kernels' callers
X, y = points(3, 300)
Xs = np.asfortranarray(rng.uniform(-2, 2, (3, 40)))
yc = np.where(y > 0, 1.0, -1.0)
for name in ("sqrexp", "matern52_ard"):
    theta = theta_of(name, 3)

    def local_gpr():
        with LocalGPR(X, y, 0.05, kfun(name, theta), m=17) as model:
            return h(model.predict(Xs), model.info, model.predict(Xs, pointwise_var=False))

    def local_gpc():
        with LocalGPC(X, yc, kfun(name, theta), m=17) as model:
            return h(*model.predict_latent(Xs), model.predict_class(Xs), model.info)
    record(f"lgpr_predict/{name}", local_gpr)
    record(f"lgpc_predict/{name}", local_gpc)

# ---- the iterative GPR's evidence gradient
for name, d in (("sqrexp", 3), ("gammaexp", 3), ("rationalquadratic", 3), ("sqrexp_ard", 17)):
    X, y = points(d, 300)
    theta = theta_of(name, d)

    def evidence():
        with IterativeGPR(X, y, 0.1, kfun(name, theta), precond_rank=32) as model:
            est = model.logp_grad(7, rng=np.random.default_rng(7))
            return h([est.value, est.se], est.grad, est.terms)
    record(f"igpr_logp_grad/{name}/d{d}", evidence)

json.dump(out, open(sys.argv[1], "w"), indent=1, sort_keys=True)
print(json.dumps(out))
