"""SHA-256 digests of what the model pipelines of the host layer return on fixed seeded inputs (numpy default_rng(424242); n = 700,
d = 3 and n = 3000, d = 5): gprc_gpr_logp_grad and gprc_gpc_logq_grad on the four gradient kernels, gprc_gpr_log_marginal,
gprc_fit_gradient, gprc_gpc_fit with predict_latent / predict_class / L, GPR.add_data (m = 1, then m = 149), the full-covariance
predict, the jitter retry, gprc_kernel_matrix to a host array, gprc_mvn_sample / gprc_mvn_factor on the Cholesky and on the eigen
branch, gprc_sym_eigen.  An error status is recorded as its text.  The library is the one GPRC_LIB_SUFFIX selects, so two builds are
compared bit for bit by running it once per build and comparing the two files:
    GPRC_LIB_SUFFIX=_parent python tools/host_digests.py parent.json;  python tools/host_digests.py change.json;  cmp parent.json change.json
(the "lib" entry is left out of the file for that reason and only printed)."""
import hashlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gprc_amd
from gprc_amd import GPR, GPC, cov_func, sqrexp, _native as nat
from gprc_amd.fit import logp_grad, logq_grad, dens_deriv, dens
from gprc_amd.sampling import multivariate_normal, mvn_factor, sym_eigen

out = {}
print("library:", os.path.basename(nat.LIB_PATH))


def h(*arrs):
    m = hashlib.sha256()
    for a in arrs:
        m.update(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes())
    return m.hexdigest()[:24]


rng = np.random.default_rng(424242)
for n, d in ((700, 3), (3000, 5)):
    X = np.asfortranarray(rng.uniform(-2, 2, (d, n)))
    y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
    yc = np.sign(X[0] - 0.5 * X[-1] + 0.3 * rng.normal(size=n)); yc[yc == 0] = 1.0
    ell = rng.uniform(0.7, 2.0, d)
    cases = {"sqrexp": [1.3], "gammaexp": [0.9, 1.5], "rationalquadratic": [1.1, 1.7], "sqrexp_ard": ell}
    for name, v in cases.items():
        lp, g = logp_grad(X, y, 0.05, name, v)
        out[f"logp_grad/{name}/{n}"] = h([lp], g)
        lq, gq = logq_grad(X, yc, name, v)
        out[f"logq_grad/{name}/{n}"] = h([lq], gq)
    out[f"dens/{n}"] = h([dens(X, y, 0.05, "sqrexp", [1.3])])
    for name, v in (("sqrexp", [1.3]), ("gammaexp", [0.9, 1.5]), ("rationalquadratic", [0.3, 1.5]), ("polynomial", [1.0, 2.0])):
        try:
            out[f"fit_gradient/{name}/{n}"] = h(dens_deriv(X[:, :min(n, 900)], y[:min(n, 900)], name, v))
        except Exception as e:   # a noise-free K that is not positive definite: the status is the output
            out[f"fit_gradient/{name}/{n}"] = "error: " + type(e).__name__ + " " + str(e)[:80]
    Xs = np.asfortranarray(rng.uniform(-2, 2, (d, 333)))
    for rs in (True, False):
        try:
            gc = GPC(X, yc, cov_func(sqrexp, l=1.3), 1e-5, reference_stop=rs)
            fs, vf = gc.predict_latent(Xs)
            out[f"gpc_fit/{n}/stop{int(rs)}"] = h(gc.f_hat, [gc.logq, gc.iterations], fs, vf, gc.predict_class(Xs), gc._get_L())
        except Exception as e:
            out[f"gpc_fit/{n}/stop{int(rs)}"] = "error: " + type(e).__name__ + " " + str(e)[:80]
    g = GPR(X[:, :n - 150], y[:n - 150], 0.1, cov_func(sqrexp, l=1.0))
    p0 = g.predict(Xs)
    g.add_data(X[:, n - 150:n - 149], y[n - 150:n - 149])
    g.add_data(X[:, n - 149:], y[n - 149:])
    out[f"add_data/{n}"] = h(p0, g.alpha, [g.logp], g.predict(Xs), g._get_L())
    pf = g.predict(Xs, pointwise_var=False)
    out[f"predict_full/{n}"] = h(*pf) if isinstance(pf, (tuple, list)) else h(pf)
    try:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            gr = GPR(X, y, 0.0, cov_func(sqrexp, l=4.0))          # the jitter retry
        out[f"fit_retry/{n}"] = h(gr.alpha, [gr.logp, gr.noise])
    except Exception as e:
        out[f"fit_retry/{n}"] = "error: " + type(e).__name__ + " " + str(e)[:80]
    out[f"kernel_matrix/{n}"] = h(gprc_amd.covariance_matrix(X[:, :300], Xs, cov_func(sqrexp, l=1.3)))

m = 200
A = rng.normal(size=(m, m)); cov = A @ A.T + m * np.eye(m)
z = rng.standard_normal((m, 7))
out["mvn/chol"] = h(multivariate_normal(7, np.arange(m) * 0.01, cov, z=z), mvn_factor(cov)[0]) + " " + mvn_factor(cov)[1]
B = rng.normal(size=(m, 20)); cov2 = B @ B.T                      # rank 20: Cholesky fails, the eigen path
out["mvn/eigen"] = h(multivariate_normal(7, np.arange(m) * 0.01, cov2, z=z), mvn_factor(cov2)[0]) + " " + mvn_factor(cov2)[1]
ev = sym_eigen(cov)
out["sym_eigen"] = h(*ev) if isinstance(ev, (tuple, list)) else h(ev)
json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out))
