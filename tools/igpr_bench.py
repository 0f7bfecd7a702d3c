"""Iterative exact GPR (gprc_igpr_*) at the sizes where the factor still fits and where it no longer does: iterations, seconds per
iteration, the product's share, the time beside gprc_gpr_fit and the distance from the exact model.  Records, not thresholds.
d = 8, noise 0.1, matern52_ard (l_k = 1 + k / 16), tools/grad_bench.py's inputs (X ~ U[-1, 1]^8, y = 0.1 sum(x^3) + N(0, 0.1^2), Philox
seed 20261004), preconditioner ranks 0 / 128 / 512, tolerance 1e-8; every array of the timed calls resident in device memory.
    python tools/igpr_bench.py                         # n = 65536 (with the exact leg) and 262144 (without); appends to profiles/igpr_bench.txt
    python tools/igpr_bench.py 65536 --reps 3          # the n's named; --reps R timed solves (default 3), --max-iter M (default 1000),
                                                       # --no-exact: skip gprc_gpr_fit (forced above n = 131072: no factor fits)
Per n and rank one JSON line.  The model is fitted on y = 0 (zero iterations), so `precond_ms` is the preconditioner alone -- pivoted
Cholesky, the r x r algebra, Q -- and the solve of y is timed by itself through gprc_igpr_solve, which reports its iterations and true
residual even when it runs into max_iter (gprc_igpr_fit would return no model):
  precond_ms        host clock around the synchronous fit of y = 0, after a warm-up fit: [median, min, max] of the reps
  rank              columns the pivoted Cholesky produced
  solve_ms          gprc_igpr_solve of y (device pointers): [median, min, max] of the reps after one warm-up solve capped at 3 iterations
  iterations, relres_true, status     of that solve (status -6: max_iter reached)
  s_per_iter        median solve_ms / (iterations + 1) / 1000: the + 1 is the true residual's product
  product_share     profiled once more with gprc_prof_enable: the generated-operand product's event time (kind 19) / that solve's wall time
  fit_ms            precond_ms + solve_ms medians: what gprc_igpr_fit of y costs;  exact_fit_ms: gprc_gpr_fit of the same run, once
  alpha_dist        max |alpha - alpha_exact| / max |alpha_exact|
  pred_dist         the same for the posterior mean at 1024 points of the same cloud, the iterative one as K(X*, X) alpha through
                    gprc_dev_kernel_gemm (the product gprc_igpr_predict's mean is), the exact one from gprc_gpr_predict
"""
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
from gprc_amd import GPR, cov_func, matern52_ard
from gprc_amd import _native as nat
from grad_bench import synth

RANKS = (0, 128, 512)
TOL = 1e-8
N_PRED = 1024
KIND_PRODUCT = 19


def spread(v):
    return [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)]


def option(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    skip = {sys.argv.index(o) + 1 for o in ("--reps", "--max-iter") if o in sys.argv}
    sizes = [int(a) for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and i not in skip] or [65536, 262144]
    reps, max_iter = option("--reps", 3), option("--max-iter", 1000)
    lib = nat.lib()
    ctx = nat.default_context()
    d, noise = 8, 0.1
    dev = torch.device("cuda:0")
    theta = 1.0 + np.arange(d) / 16.0
    _, pp, npar = nat.params_array(theta)
    k = cov_func(matern52_ard, l=theta)
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "igpr_bench.txt")
    for n in sizes:
        Xh, yh = synth(n, d)
        Xd, yd = torch.from_numpy(Xh).to(dev), torch.from_numpy(yh).to(dev)
        zero = torch.zeros(n, dtype=torch.float64, device=dev)
        Xs = torch.from_numpy(synth(n + N_PRED, d)[0][n:].copy()).to(dev)   # further points of the same stream
        torch.cuda.synchronize()
        exact = n <= 131072 and "--no-exact" not in sys.argv
        exact_fit_ms = alpha_exact = mean_exact = None
        if exact:
            t0 = time.perf_counter()
            g = GPR(Xh.T, yh, noise, k)
            exact_fit_ms = (time.perf_counter() - t0) * 1e3
            alpha_exact = g.alpha.copy()
            mean_exact = g.predict(np.asfortranarray(Xs.cpu().numpy().T))[:, 0]
            g.close()
            nat.check(lib.gprc_ctx_trim(ctx.handle))
        for rank in RANKS:
            h = C.c_void_p()

            def fit(cap):
                if h:
                    nat.check(lib.gprc_model_free(h))
                    h.value = None
                t = time.perf_counter()
                nat.check(lib.gprc_igpr_fit(ctx.handle, nat.MATERN52_ARD, pp, npar, Xd.data_ptr(), d, n, zero.data_ptr(), noise, TOL, cap, rank, C.byref(h)))
                return (time.perf_counter() - t) * 1e3

            fit(3)                                                   # warm-up: code objects, the pool's blocks, the chunk workspace
            precond = [fit(3) for _ in range(reps)]
            fit(max_iter)
            alpha = torch.empty(n, dtype=torch.float64, device=dev)
            its, res = C.c_int(), C.c_double()

            def solve(model):
                torch.cuda.synchronize()
                t = time.perf_counter()
                rc = lib.gprc_igpr_solve(model, yd.data_ptr(), n, 1, alpha.data_ptr(), n, C.byref(its), C.byref(res))
                ctx.synchronize()
                if rc not in (0, nat.ERR_MAXITER):
                    nat.check(rc)
                return (time.perf_counter() - t) * 1e3, rc

            hw = C.c_void_p()                                        # the warm-up solve: a model that stops after three iterations
            nat.check(lib.gprc_igpr_fit(ctx.handle, nat.MATERN52_ARD, pp, npar, Xd.data_ptr(), d, n, zero.data_ptr(), noise, TOL, 3, min(rank, 8), C.byref(hw)))
            solve(hw)
            nat.check(lib.gprc_model_free(hw))
            runs = [solve(h) for _ in range(reps)]
            ms, status = [r[0] for r in runs], runs[-1][1]
            lib.gprc_prof_reset()
            lib.gprc_prof_enable(1)
            prof_ms, _ = solve(h)
            lib.gprc_prof_enable(0)
            product_ms = nat.prof_summary()["pred_grad_contract"]["ms"]
            rk = C.c_int64()
            nat.check(lib.gprc_igpr_stats(h, None, None, None, C.byref(rk)))
            rec = dict(n=n, d=d, kernel="matern52_ard", noise=noise, tol=TOL, max_iter=max_iter, precond_rank=rank, rank=rk.value, reps=reps,
                       precond_ms=spread(precond), solve_ms=spread(ms), iterations=its.value, relres_true=res.value, status=status,
                       s_per_iter=round(statistics.median(ms) / (its.value + 1) / 1e3, 5), product_share=round(product_ms / prof_ms, 3),
                       fit_ms=round(statistics.median(precond) + statistics.median(ms), 1),
                       exact_fit_ms=round(exact_fit_ms, 1) if exact else None)
            if exact:
                a = alpha.cpu().numpy()
                rec["alpha_dist"] = float(np.abs(a - alpha_exact).max() / np.abs(alpha_exact).max())
                mean = torch.empty(N_PRED, dtype=torch.float64, device=dev)
                nat.check(lib.gprc_dev_kernel_gemm(ctx.handle, nat.MATERN52_ARD, pp, npar, Xs.data_ptr(), N_PRED, Xd.data_ptr(), n, d, alpha.data_ptr(), n, 1,
                                                   mean.data_ptr(), N_PRED))
                rec["pred_dist"] = float(np.abs(mean.cpu().numpy() - mean_exact).max() / np.abs(mean_exact).max())
            nat.check(lib.gprc_model_free(h))
            nat.check(lib.gprc_ctx_trim(ctx.handle))
            line = json.dumps(rec)
            print(line, flush=True)
            with open(path, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
