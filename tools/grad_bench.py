"""gprc_gpr_logp_grad (value + exact gradient in one call) against the only other way to the same gradient, central differences of
gprc_gpr_log_marginal: 2 (p + 1) calls for p parameters and the noise.  d = 8, noise 0.1, bench.py's C4 inputs (X ~ U[-1, 1],
y = 0.1 sum(x^3) + N(0, 0.1^2), Philox seed 20261004), resident in device memory; kernels: sqrexp_ard and matern52_ard
(l_k = 1 + k / 16), sqrexp and matern52 (l = 1).
    python tools/grad_bench.py                         # n = 4096 8192 16384 32768
    python tools/grad_bench.py 16384 --once            # one logp_grad call per kernel, nothing else (the run to put under rocprofv3)
Per (n, kernel) one JSON line: logp_grad_ms = median of 5 calls after a warm-up (host clock around the synchronous C-ABI call);
marginal_ms likewise, fd_ms = 2 (p + 1) marginal_ms; stages_ms = one further call under the in-library event profiler, grouped into
fit / linv (the identity through the predict solve) / inverse_gemm / contraction; contraction_gbs = the bytes the contraction has to
read (the stored triangle of the inverse once + X + alpha) over its event time; fit_gradient_ms = the reference-form gradient
(diag(K^-1) only, noise-free K) on the same inputs, for context."""
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import gprc_amd  # noqa: F401
from gprc_amd import _native as nat

SEED = 20261004
LINV = ("solve_left", "solve_panel", "solve_update_k512", "trsm_panel", "gemm_inner_k128")


def synth(n, d):
    rng = np.random.Generator(np.random.Philox(SEED))
    X = rng.uniform(-1.0, 1.0, size=(n, d))          # row i = point i (== d x n column-major)
    y = 0.1 * (X ** 3).sum(1) + rng.normal(0.0, 0.1, size=n)
    return np.ascontiguousarray(X), y


def timed(f, reps):
    f()                                              # warm-up: code objects, workspace, pool
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    sizes = [int(a) for a in sys.argv[1:] if not a.startswith("--")] or [4096, 8192, 16384, 32768]
    once = "--once" in sys.argv
    lib = nat.lib()
    ctx = nat.default_context().handle
    d, noise = 8, 0.1
    dev = torch.device("cuda:0")
    kernels = [("sqrexp_ard", nat.SQREXP_ARD, 1.0 + np.arange(d) / 16.0), ("sqrexp", nat.SQREXP, np.array([1.0])),
               ("matern52_ard", nat.MATERN52_ARD, 1.0 + np.arange(d) / 16.0), ("matern52", nat.MATERN52, np.array([1.0]))]
    for n in sizes:
        Xh, yh = synth(n, d)
        X, y = torch.from_numpy(Xh).to(dev), torch.from_numpy(yh).to(dev)
        torch.cuda.synchronize()
        for name, kid, theta in kernels:
            _, pp, npar = nat.params_array(theta)
            lp, grad = C.c_double(), np.empty(npar + 1)

            def marginal():
                nat.check(lib.gprc_gpr_log_marginal(ctx, kid, pp, npar, X.data_ptr(), d, n, y.data_ptr(), noise, C.byref(lp)))

            def logp_grad():
                nat.check(lib.gprc_gpr_logp_grad(ctx, kid, pp, npar, X.data_ptr(), d, n, y.data_ptr(), noise, C.byref(lp),
                                                 grad.ctypes.data_as(C.POINTER(C.c_double))))
            if once:
                logp_grad()
                print(json.dumps(dict(n=n, kernel=name, logp=lp.value, grad=[float(f"{g:.6e}") for g in grad])), flush=True)
                continue
            rec = dict(n=n, d=d, kernel=name, params=npar)
            mm = timed(marginal, 5)
            rec["marginal_ms"], rec["marginal_runs"] = round(statistics.median(mm), 2), [round(v, 2) for v in mm]
            rec["fd_calls"] = 2 * (npar + 1)
            rec["fd_ms"] = round(rec["fd_calls"] * rec["marginal_ms"], 2)
            gg = timed(logp_grad, 5)
            rec["logp_grad_ms"], rec["logp_grad_runs"] = round(statistics.median(gg), 2), [round(v, 2) for v in gg]
            rec["fd_over_logp_grad"] = round(rec["fd_ms"] / rec["logp_grad_ms"], 2)
            lib.gprc_prof_reset()
            lib.gprc_prof_enable(1)
            logp_grad()
            lib.gprc_prof_enable(0)
            prof = {k: v for k, v in nat.prof_summary().items() if v["count"]}
            lib.gprc_prof_reset()
            linv = sum(v["ms"] for k, v in prof.items() if k in LINV)
            rest = sum(v["ms"] for k, v in prof.items() if k not in LINV + ("inverse_gemm", "grad_contract"))
            rec["stages_ms"] = dict(fit=round(rest, 2), linv=round(linv, 2), inverse_gemm=round(prof["inverse_gemm"]["ms"], 2),
                                    contraction=round(prof["grad_contract"]["ms"], 3))
            rec["inverse_gemm_tflops"] = round(prof["inverse_gemm"]["flops"] / prof["inverse_gemm"]["ms"] / 1e9, 1)
            rec["contraction_gbs"] = round(prof["grad_contract"]["bytes"] / prof["grad_contract"]["ms"] / 1e6, 1)
            if name == "sqrexp":
                g1 = np.empty(1)

                def fit_gradient():
                    nat.check(lib.gprc_fit_gradient(ctx, kid, pp, npar, X.data_ptr(), d, n, y.data_ptr(), g1.ctypes.data_as(C.POINTER(C.c_double))))
                try:
                    fg = timed(fit_gradient, 3)
                    rec["fit_gradient_ms"] = round(statistics.median(fg), 2)
                except nat.NotPositiveDefinite:
                    rec["fit_gradient_ms"] = None    # the reference form factors the NOISE-FREE K: not positive definite in fp64 at this n
            print(json.dumps(rec), flush=True)
        del X, y
        nat.check(lib.gprc_ctx_trim(ctx))


if __name__ == "__main__":
    main()
