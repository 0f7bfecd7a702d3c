"""gprc_gpc_logq_grad (Laplace log evidence + exact gradient, one call) against the cost of the mode search alone, gprc_gpc_fit
(flags 0, the same epsilon): the only other way to the gradient is central differences, 2 p mode searches for p parameters.
d = 8, epsilon 1e-10, X ~ U[-1, 1], y = sign(x_0 - 0.5 x_7 + 0.3 N(0, 1)) (Philox seed 20261016), resident in device memory;
kernels: sqrexp (l = 1), sqrexp_ard and matern52_ard (l_k = 1 + k / 16).
    python tools/gpc_grad_bench.py                                   # n = 4096 8192 16384, writes profiles/gpc_logq_grad_bench.txt
    python tools/gpc_grad_bench.py 8192 --parent-lib PATH --out FILE  # gprc_gpc_fit also timed on another build of the library
    python tools/gpc_grad_bench.py --check-gpr FILE                   # dump of gprc_gpr_logp_grad on six fixed cases, nothing else
Per (n, kernel) one JSON line.  Times are host clocks around the synchronous C-ABI calls, medians of 5 after a warm-up; the calls of
a round alternate (fit, parent's fit, logq_grad) so that drift of the shared machine hits all of them alike.  stages_ms = one further
call under the in-library event profiler: mode_search (everything that is neither of the following, i.e. fills, factorisations and
the loop's vector work, WITH the gradient's vector stage), linv (the identity through the predict solve), inverse_gemm, contraction;
vector_stage_est = the gradient's share of the vector kinds (2 of the 2 iters + 2 vector solves, 1 of the 2 iters + 1 matvecs).
contraction_gbs = the bytes the contraction has to read (the stored triangle of -B^-1 once + X + four vectors) over its event time;
gpr_contraction_gbs = the same for gprc_gpr_logp_grad's contraction on the same n and kernel (one further call, noise 0.1).
The gate: at n = 8192, sqrexp, logq_grad_ms < 2 x the parent build's fit_ms (this build's fit_ms when no parent library is given).

--check-gpr: logp and gradient of gprc_gpr_logp_grad for the six cases of tests/test_gpu_ard_grad.py::test_gradient_against_the_
closed_form at n = 3000, as raw float64 bytes in FILE.  The library is the one GPRC_LIB_SUFFIX selects: two runs, two builds, and
`cmp` says whether the regression gradient changed in any bit."""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import gprc_amd  # noqa: F401
from gprc_amd import _native as nat
from gprc_amd.fit import logp_grad

SEED = 20261016
EPS = 1e-10
LINV = ("solve_left", "solve_panel", "solve_update_k512", "trsm_panel", "gemm_inner_k128")


def synth(n, d):
    rng = np.random.Generator(np.random.Philox(SEED))
    X = rng.uniform(-1.0, 1.0, size=(n, d))          # row i = point i (== d x n column-major)
    y = np.sign(X[:, 0] - 0.5 * X[:, d - 1] + 0.3 * rng.normal(size=n))
    y[y == 0] = 1.0
    return np.ascontiguousarray(X), y


def check_gpr(path):
    out = []
    for case, n, noise in (("sqrexp", 3000, 0.05), ("gammaexp1.5", 3000, 0.05), ("gammaexp1", 3000, 0.05), ("ratquad", 3000, 0.05),
                           ("ard3", 3000, 0.05), ("ard8", 3000, 0.05)):
        d = int(case[3:]) if case.startswith("ard") else 3
        rng = np.random.default_rng(1000 + n + d)
        X = rng.uniform(-2, 2, (d, n))
        y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
        ell = rng.uniform(0.7, 2.0, d)
        name, theta = ("sqrexp_ard", ell) if case.startswith("ard") else {
            "sqrexp": ("sqrexp", [1.3]), "gammaexp1.5": ("gammaexp", [0.9, 1.5]), "gammaexp1": ("gammaexp", [1.2, 1.0]),
            "ratquad": ("rationalquadratic", [1.1, 1.7])}[case]
        logp, grad = logp_grad(X, y, noise, name, theta)
        print(json.dumps(dict(check_gpr=case, n=n, lib=os.path.basename(nat.LIB_PATH), logp=logp, grad=[float(g) for g in grad])), flush=True)
        out.append(np.concatenate([[logp], grad]))
    np.concatenate(out).astype("<f8").tofile(path)


def bind(path):
    """another build of the library, beside the package's own: only what the fit timing needs"""
    lib = C.CDLL(path)
    for name in ("gprc_ctx_create", "gprc_gpc_fit", "gprc_model_free", "gprc_last_error"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = nat.PROTOTYPES[name]
    h = C.c_void_p()
    if lib.gprc_ctx_create(0, None, C.byref(h)) != 0:
        raise RuntimeError(lib.gprc_last_error())
    return lib, h


def main():
    args = sys.argv[1:]

    def opt(flag):
        if flag in args:
            i = args.index(flag)
            v = args[i + 1]
            del args[i:i + 2]
            return v
        return None
    dump = opt("--check-gpr")
    if dump:
        return check_gpr(dump)
    import torch
    parent_path = opt("--parent-lib")
    out_path = opt("--out") or os.path.join(ROOT, "profiles", "gpc_logq_grad_bench.txt")
    sizes = [int(a) for a in args] or [4096, 8192, 16384]
    lib = nat.lib()
    ctx = nat.default_context().handle
    parent = bind(parent_path) if parent_path else None
    d = 8
    dev = torch.device("cuda:0")
    kernels = [("sqrexp", nat.SQREXP, np.array([1.0])), ("sqrexp_ard", nat.SQREXP_ARD, 1.0 + np.arange(d) / 16.0),
               ("matern52_ard", nat.MATERN52_ARD, 1.0 + np.arange(d) / 16.0)]
    log = open(out_path, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()
    emit(dict(tool="gpc_grad_bench", sizes=sizes, d=d, epsilon=EPS, parent_lib=os.path.basename(parent_path) if parent_path else None))
    for n in sizes:
        Xh, yh = synth(n, d)
        X, y = torch.from_numpy(Xh).to(dev), torch.from_numpy(yh).to(dev)
        torch.cuda.synchronize()
        for name, kid, theta in kernels:
            _, pp, npar = nat.params_array(theta)
            lq, grad, iters = C.c_double(), np.empty(npar), C.c_int()

            def fit(l=lib, c=ctx):
                m, it = C.c_void_p(), C.c_int()
                rc = l.gprc_gpc_fit(c, kid, pp, npar, X.data_ptr(), d, n, y.data_ptr(), EPS, 0, 0, C.byref(m), C.byref(it))
                if rc != 0:
                    raise RuntimeError(f"gprc_gpc_fit: {rc}")
                l.gprc_model_free(m)
                return it.value

            def logq_grad():
                nat.check(lib.gprc_gpc_logq_grad(ctx, kid, pp, npar, X.data_ptr(), d, n, y.data_ptr(), EPS, 0, C.byref(lq),
                                                 grad.ctypes.data_as(C.POINTER(C.c_double)), C.byref(iters)))
            calls = {"fit": fit, "logq_grad": logq_grad}
            if parent:
                calls["parent_fit"] = lambda: fit(*parent)
            runs = {k: [] for k in calls}
            for f in calls.values():                     # warm-up: code objects, workspace, pool
                f()
            for _ in range(5):
                for k, f in calls.items():
                    t0 = time.perf_counter()
                    f()
                    runs[k].append((time.perf_counter() - t0) * 1e3)
            rec = dict(n=n, d=d, kernel=name, params=npar, iters=iters.value, logq=lq.value)
            for k, v in runs.items():
                rec[k + "_ms"], rec[k + "_runs"] = round(statistics.median(v), 2), [round(x, 2) for x in v]
            base = rec["parent_fit_ms"] if parent else rec["fit_ms"]
            rec["logq_grad_over_fit"] = round(rec["logq_grad_ms"] / base, 3)
            rec["fd_calls"] = 2 * npar
            rec["fd_over_logq_grad"] = round(2 * npar * base / rec["logq_grad_ms"], 2)
            if n == 8192 and name == "sqrexp":
                rec["gate_lt_2x_fit"] = bool(rec["logq_grad_ms"] < 2.0 * base)
            lib.gprc_prof_reset()
            lib.gprc_prof_enable(1)
            logq_grad()
            lib.gprc_prof_enable(0)
            prof = {k: v for k, v in nat.prof_summary().items() if v["count"]}
            lib.gprc_prof_reset()
            linv = sum(v["ms"] for k, v in prof.items() if k in LINV)
            rest = sum(v["ms"] for k, v in prof.items() if k not in LINV + ("inverse_gemm", "gpc_grad_contract"))
            it = iters.value
            vec = prof["trsv"]["ms"] * 2 / (2 * it + 2) + prof["row_reduce"]["ms"] / (2 * it + 1)
            con = prof["gpc_grad_contract"]
            rec["stages_ms"] = dict(mode_search=round(rest, 2), linv=round(linv, 2), inverse_gemm=round(prof["inverse_gemm"]["ms"], 2),
                                    vector_stage_est=round(vec, 3), contraction=round(con["ms"], 3))
            rec["inverse_gemm_tflops"] = round(prof["inverse_gemm"]["flops"] / prof["inverse_gemm"]["ms"] / 1e9, 1)
            rec["contraction_gbs"] = round(con["bytes"] / con["ms"] / 1e6, 1)
            lp, g2 = C.c_double(), np.empty(npar + 1)
            lib.gprc_prof_enable(1)
            rc = lib.gprc_gpr_logp_grad(ctx, kid, pp, npar, X.data_ptr(), d, n, y.data_ptr(), 0.1, C.byref(lp), g2.ctypes.data_as(C.POINTER(C.c_double)))
            lib.gprc_prof_enable(0)
            if rc == 0:
                gc = nat.prof_summary()["grad_contract"]
                rec["gpr_contraction_ms"] = round(gc["ms"], 3)
                rec["gpr_contraction_gbs"] = round(gc["bytes"] / gc["ms"] / 1e6, 1)
                rec["contraction_rate_over_gpr"] = round(rec["contraction_gbs"] / rec["gpr_contraction_gbs"], 3)
            lib.gprc_prof_reset()
            emit(rec)
        del X, y
        nat.check(lib.gprc_ctx_trim(ctx))
    log.close()


if __name__ == "__main__":
    main()
