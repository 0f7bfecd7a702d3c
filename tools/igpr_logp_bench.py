"""The iterative GPR's stochastic log evidence (gprc_igpr_logp_grad) and its contraction (gprc_dev_lowrank_grad): where the time goes and
how far the estimate sits from the exact evidence.  Records, not thresholds.  tools/igpr_bench.py's problem: d = 8, noise 0.1, matern52_ard
(l_k = 1 + k / 16), tools/grad_bench.py's inputs, tolerance 1e-8; every array of the timed calls resident in device memory; the normals
from default_rng(20261020), G2 first.
    python tools/igpr_logp_bench.py                    # all three legs; appends JSON lines to profiles/igpr_logp_bench.txt
    python tools/igpr_logp_bench.py --n 65536 --n-exact 16384 --reps 3 --legs logp,contraction,exact
Legs, one JSON line each, medians of --reps timed calls after one warm-up call:
  logp          at n, ranks 128 and 512, T = 31 and 63: total_ms of gprc_igpr_logp_grad and its parts timed by themselves through the ABI --
                solve_ms: gprc_igpr_solve of the same T probes (the same loop without the history's stores); contraction_ms:
                gprc_dev_lowrank_grad with R = T + 1 columns; rest_ms = total - solve - contraction: the probes, P^-1 z, the column dots,
                the copies and the host's quadrature, which the ABI does not time by itself; iterations of the probes' solve
  contraction   at n, R = 32 and 64: ms and pairs per ns (n^2 / time), beside gprc_dev_kernel_gemm with S = 64 of the same run (the
                generated-operand product the solve's iterations consist of)
  exact         at n_exact: gprc_gpr_logp_grad of the same run beside the stochastic value and gradient (rank 128, T = 63) and the value's
                standard error
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
from gprc_amd import _native as nat
from gprc_amd.fit import logp_grad
from grad_bench import synth

TOL = 1e-8
SEED = 20261020


def option(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn, reps):
    fn()                                                             # warm-up: code objects, the pool's blocks
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(out), 2)


def main():
    n, n_exact, reps = option("--n", 65536), option("--n-exact", 16384), option("--reps", 3)
    legs = option("--legs", "logp,contraction,exact", str).split(",")
    lib, ctx = nat.lib(), nat.default_context()
    d, noise = 8, 0.1
    dev = torch.device("cuda:0")
    theta = 1.0 + np.arange(d) / 16.0
    _, pp, npar = nat.params_array(theta)
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "igpr_logp_bench.txt")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(path, "a") as f:
            f.write(line + "\n")

    def fit(Xd, yd, m, rank):
        h = C.c_void_p()
        nat.check(lib.gprc_igpr_fit(ctx.handle, nat.MATERN52_ARD, pp, npar, Xd.data_ptr(), d, m, yd.data_ptr(), noise, TOL, 1000, rank, C.byref(h)))
        rk = C.c_int64()
        nat.check(lib.gprc_igpr_stats(h, None, None, None, C.byref(rk)))
        return h, rk.value

    def normals(m, rank, T):
        rng = np.random.default_rng(SEED)
        g2 = torch.from_numpy(np.ascontiguousarray(rng.standard_normal((m, T)).T)).to(dev)      # T x m in C order = m x T column-major
        g1 = torch.from_numpy(np.ascontiguousarray(rng.standard_normal((max(rank, 1), T)).T)).to(dev)
        return g1, g2

    def evidence(h, g1, g2, m, rank, T):
        lp, se = C.c_double(), C.c_double()
        grad, terms = np.empty(npar + 1), np.empty(T)
        nat.check(lib.gprc_igpr_logp_grad(h, g1.data_ptr(), max(rank, 1), g2.data_ptr(), m, T, C.byref(lp), C.byref(se), grad.ctypes.data, terms.ctypes.data))
        return lp.value, se.value, grad

    Xh, yh = synth(n, d)
    Xd, yd = torch.from_numpy(Xh).to(dev), torch.from_numpy(yh).to(dev)
    torch.cuda.synchronize()

    if "logp" in legs:
        for precond_rank in (128, 512):
            h, rank = fit(Xd, yd, n, precond_rank)
            for T in (31, 63):
                g1, g2 = normals(n, rank, T)
                Z = torch.empty((T, n), dtype=torch.float64, device=dev)
                nat.check(lib.gprc_igpr_probes(h, g1.data_ptr(), max(rank, 1), g2.data_ptr(), n, T, Z.data_ptr(), n))
                U = torch.empty((T, n), dtype=torch.float64, device=dev)
                its = (C.c_int * T)()
                A = torch.randn((T + 1, n), dtype=torch.float64, device=dev)
                B = torch.randn((T + 1, n), dtype=torch.float64, device=dev)
                gout = np.empty(npar)
                total = timed(lambda: evidence(h, g1, g2, n, rank, T), reps)
                solve = timed(lambda: nat.check(lib.gprc_igpr_solve(h, Z.data_ptr(), n, T, U.data_ptr(), n, its, None)), reps)
                contraction = timed(lambda: nat.check(lib.gprc_dev_lowrank_grad(ctx.handle, nat.MATERN52_ARD, pp, npar, Xd.data_ptr(), d, n, A.data_ptr(), n,
                                                                                B.data_ptr(), n, T + 1, gout.ctypes.data)), reps)
                lp, se, grad = evidence(h, g1, g2, n, rank, T)
                emit(dict(leg="logp", MEASURED=True, n=n, d=d, kernel="matern52_ard", noise=noise, tol=TOL, precond_rank=precond_rank, rank=rank, T=T, reps=reps,
                          total_ms=total, solve_ms=solve, contraction_ms=contraction, rest_ms=round(total - solve - contraction, 2),
                          iterations=[min(its), max(its)], logp=lp, se=se))
            nat.check(lib.gprc_model_free(h))
            nat.check(lib.gprc_ctx_trim(ctx.handle))

    if "contraction" in legs:
        S = 64
        Ug = torch.randn((S, n), dtype=torch.float64, device=dev)
        out = torch.empty((S, n), dtype=torch.float64, device=dev)
        gemm = timed(lambda: nat.check(lib.gprc_dev_kernel_gemm(ctx.handle, nat.MATERN52_ARD, pp, npar, Xd.data_ptr(), n, Xd.data_ptr(), n, d, Ug.data_ptr(), n, S,
                                                                out.data_ptr(), n)), reps)
        for Rk in (32, 64):
            A = torch.randn((Rk, n), dtype=torch.float64, device=dev)
            B = torch.randn((Rk, n), dtype=torch.float64, device=dev)
            gout = np.empty(npar)
            ms = timed(lambda: nat.check(lib.gprc_dev_lowrank_grad(ctx.handle, nat.MATERN52_ARD, pp, npar, Xd.data_ptr(), d, n, A.data_ptr(), n, B.data_ptr(), n,
                                                                   Rk, gout.ctypes.data)), reps)
            emit(dict(leg="contraction", MEASURED=True, n=n, d=d, kernel="matern52_ard", R=Rk, reps=reps, ms=ms, pairs_per_ns=round(n * n / (ms * 1e6), 2),
                      kernel_gemm_S64_ms=gemm, kernel_gemm_pairs_per_ns=round(n * n / (gemm * 1e6), 2)))

    if "exact" in legs:
        m = n_exact
        Xe, ye = synth(m, d)
        t = time.perf_counter()
        exact_value, exact_grad = logp_grad(Xe.T, ye, noise, "matern52_ard", theta)
        exact_ms = (time.perf_counter() - t) * 1e3
        nat.check(lib.gprc_ctx_trim(ctx.handle))
        Xed, yed = torch.from_numpy(Xe).to(dev), torch.from_numpy(ye).to(dev)
        h, rank = fit(Xed, yed, m, 128)
        T = 63
        g1, g2 = normals(m, rank, T)
        ms = timed(lambda: evidence(h, g1, g2, m, rank, T), reps)
        lp, se, grad = evidence(h, g1, g2, m, rank, T)
        emit(dict(leg="exact", MEASURED=True, n=m, d=d, kernel="matern52_ard", precond_rank=128, rank=rank, T=T, exact_logp=exact_value, logp=lp, se=se,
                  exact_grad=[float(v) for v in exact_grad], grad=[float(v) for v in grad], exact_ms=round(exact_ms, 1), stochastic_ms=ms))
        nat.check(lib.gprc_model_free(h))


if __name__ == "__main__":
    main()
