"""gprc_gpr_predict_grad (mean, variance and both gradients with respect to the test points) against gprc_gpr_predict(pointwise = 1),
the call it extends: by flop count two m n^2 solves instead of one plus three bandwidth-bound passes.  d = 8, noise 0.1, n* = n,
bench.py's C4 inputs (X ~ U[-1, 1], y = 0.1 sum(x^3) + N(0, 0.1^2), Philox seed 20261004), everything resident in device memory;
kernels: sqrexp (l = 1), sqrexp_ard and matern52_ard (l_k = 1 + k / 16).
    python tools/predict_grad_bench.py                              # n = 4096 16384
    python tools/predict_grad_bench.py 16384 --parent-lib PATH      # gprc_gpr_predict also timed on another build of the library
    python tools/predict_grad_bench.py 4096 --out FILE              # where the JSON lines are appended (default profiles/predict_grad_bench.txt)
Per (n, kernel) one JSON line.  *_ms = median of 5 calls after a warm-up, host clock around the synchronous C-ABI call, the calls
interleaved; steady state: the reversed factor exists (the warm-up built it).  predict_grad_ms all four outputs, no_dvar_ms without
the variance's gradient (one solve), dmean_only_ms the mean's gradient alone (no solve, no chunk of K*).  The yardstick is predict on
the parent build when --parent-lib is given, else on this build: ratio = predict_grad_ms / that.  reversal: the one-off
gprc_dev_reverse_factor of the first call, from the in-library event profiler, with the GB/s of its read + write.  stages_ms: one
further steady-state call under the profiler -- fill, the solves (both), contraction -- and contraction_gbs = the solved chunk read
once over the contraction's event time; mean_only_contraction_ms the same kernel without the chunk."""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import gprc_amd  # noqa: F401
from gprc_amd import _native as nat

SEED = 20261004
SOLVE = ("solve_left", "solve_panel", "solve_update_k512", "trsm_panel", "gemm_inner_k128")


def synth(n, d):
    rng = np.random.Generator(np.random.Philox(SEED))
    X = rng.uniform(-1.0, 1.0, size=(n, d))          # row i = point i (== d x n column-major)
    y = 0.1 * (X ** 3).sum(1) + rng.normal(0.0, 0.1, size=n)
    Xs = rng.uniform(-1.0, 1.0, size=(n, d))
    return np.ascontiguousarray(X), y, np.ascontiguousarray(Xs)


def bind(path):
    """another build of the library, beside the package's own: only what the predict timing needs"""
    lib = C.CDLL(path)
    for name in ("gprc_ctx_create", "gprc_gpr_fit", "gprc_gpr_predict", "gprc_model_free", "gprc_last_error"):
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
    parent_path = opt("--parent-lib")
    out_path = opt("--out") or os.path.join(ROOT, "profiles", "predict_grad_bench.txt")
    sizes = [int(a) for a in args] or [4096, 16384]
    lib = nat.lib()
    ctx = nat.default_context().handle
    parent = bind(parent_path) if parent_path else None
    d, noise = 8, 0.1
    dev = torch.device("cuda:0")
    kernels = [("sqrexp", nat.SQREXP, np.array([1.0])), ("sqrexp_ard", nat.SQREXP_ARD, 1.0 + np.arange(d) / 16.0),
               ("matern52_ard", nat.MATERN52_ARD, 1.0 + np.arange(d) / 16.0)]
    log = open(out_path, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()
    emit(dict(tool="predict_grad_bench", sizes=sizes, d=d, parent_lib=os.path.basename(parent_path) if parent_path else None))
    for n in sizes:
        Xh, yh, Xsh = synth(n, d)
        X, y, Xs = torch.from_numpy(Xh).to(dev), torch.from_numpy(yh).to(dev), torch.from_numpy(Xsh).to(dev)
        mean, var = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
        dmean, dvar = torch.empty(n * d, dtype=torch.float64, device=dev), torch.empty(n * d, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        for name, kid, theta in kernels:
            _, pp, npar = nat.params_array(theta)

            def fit(l, c):
                m = C.c_void_p()
                rc = l.gprc_gpr_fit(c, kid, pp, npar, X.data_ptr(), d, n, y.data_ptr(), noise, C.byref(m))
                if rc != 0:
                    raise RuntimeError(f"gprc_gpr_fit: {rc}")
                return m
            model = fit(lib, ctx)
            pmodel = fit(*parent) if parent else None

            def predict(l=lib, m=model):
                if l.gprc_gpr_predict(m, Xs.data_ptr(), n, 1, mean.data_ptr(), var.data_ptr()) != 0:
                    raise RuntimeError("gprc_gpr_predict")

            def grad(a=mean, b=var, c=dmean, e=dvar):
                nat.check(lib.gprc_gpr_predict_grad(model, Xs.data_ptr(), n, *[t.data_ptr() if t is not None else None for t in (a, b, c, e)]))

            def profiled(f):
                lib.gprc_prof_reset()
                lib.gprc_prof_enable(1)
                f()
                lib.gprc_prof_enable(0)
                prof = {k: v for k, v in nat.prof_summary().items() if v["count"]}
                lib.gprc_prof_reset()
                return prof
            rec = dict(n=n, n_star=n, d=d, kernel=name)
            first = profiled(grad)                            # the first call: builds the reversed factor
            rv = first["reverse_factor"]
            rec["reversal"] = dict(ms=round(rv["ms"], 3), gbs=round(rv["bytes"] / rv["ms"] / 1e6, 1), mib=round(rv["bytes"] / 2 / 2 ** 20, 1))
            calls = {"predict": predict, "predict_grad": grad, "no_dvar": lambda: grad(e=None),
                     "dmean_only": lambda: grad(a=None, b=None, e=None)}
            if parent:
                calls["parent_predict"] = lambda: predict(parent[0], pmodel)
            runs = {k: [] for k in calls}
            for f in calls.values():                          # warm-up: code objects, workspace, pool
                f()
            for _ in range(5):
                for k, f in calls.items():
                    t0 = time.perf_counter()
                    f()
                    runs[k].append((time.perf_counter() - t0) * 1e3)
            for k, v in runs.items():
                rec[k + "_ms"], rec[k + "_runs"] = round(statistics.median(v), 2), [round(x, 2) for x in v]
            base = rec["parent_predict_ms"] if parent else rec["predict_ms"]
            rec["yardstick"] = "parent_predict" if parent else "predict"
            rec["ratio"] = round(rec["predict_grad_ms"] / base, 3)
            rec["no_dvar_ratio"] = round(rec["no_dvar_ms"] / base, 3)
            rec["dmean_only_ratio"] = round(rec["dmean_only_ms"] / base, 3)
            prof = profiled(grad)
            con = prof["pred_grad_contract"]
            rec["stages_ms"] = dict(fill=round(prof["fill"]["ms"], 3), solves=round(sum(v["ms"] for k, v in prof.items() if k in SOLVE), 2),
                                    contraction=round(con["ms"], 3), reversal_launches=prof.get("reverse_factor", {}).get("count", 0))
            rec["fill_gbs"] = round(prof["fill"]["bytes"] / prof["fill"]["ms"] / 1e6, 1)
            rec["contraction_gbs"] = round(con["bytes"] / con["ms"] / 1e6, 1)
            rec["contraction_gflops"] = round(con["flops"] / con["ms"] / 1e6, 1)
            rec["mean_only_contraction_ms"] = round(profiled(lambda: grad(a=None, b=None, e=None))["pred_grad_contract"]["ms"], 3)
            emit(rec)
            lib.gprc_model_free(model)
            if parent:
                parent[0].gprc_model_free(pmodel)
        del X, y, Xs, mean, var, dmean, dvar
        nat.check(lib.gprc_ctx_trim(ctx))
    log.close()


if __name__ == "__main__":
    main()
