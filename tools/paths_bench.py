"""Posterior sample paths (gprc_gpr_paths_create / _eval) at the sizes the project predicts at, the fused update term against the route it
replaces, and today's way to draw a sample.  d = 8, noise 0.1, matern52_ard (l_k = 1 + k / 16), D = 4096 features, S = 64 paths,
tools/grad_bench.py's inputs (X ~ U[-1, 1], y = 0.1 sum(x^3) + N(0, 0.1^2), Philox seed 20261004); the draws from Philox seed 20261019;
every array of the timed calls resident in device memory.
    python tools/paths_bench.py                  # n = 16384 65536; appends to profiles/paths_bench.txt
    python tools/paths_bench.py 16384            # the n's named
Per n one JSON line:
  fit_ms            the GPR fit (host clock around the synchronous call), once
  create_first_ms   the first gprc_gpr_paths_create: it also builds the model's reversed factor
  create_ms         median of 3 further calls (prior term at the training points, two row solves of S right-hand sides)
  eval_ms           per n* in 65536, 1024: median of REPS gprc_gpr_paths_eval calls after a warm-up (both terms, partials, tails)
  update_ms / yard_ms   per n*: the update term alone, gprc_dev_kernel_gemm (n* x n pairs generated in registers, S columns), against
                    gprc_dev_fill_cross + gprc_dev_gemm_nt on the same shapes (the n* x n chunk through HBM; gemm_nt pads S to 128), taken
                    in ALTERNATING rounds of one process, host clock around work that ends in a synchronise: median and (min, max) of
                    REPS rounds each.  update_gpairs: n* n_pad / update_ms in pairs per nanosecond
  max_abs_diff      per n*: max |fused update - yardstick| over the n* x S block (two orders of summation of the same products)
  today_ms          GPR.predict(pointwise_var=False) + multivariate_normal of S draws at n* = 2048 (host arrays, as that route takes
                    them), median of 3 after a warm-up
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
from gprc_amd import GPR, cov_func, matern52_ard, multivariate_normal, spectral_frequencies
from gprc_amd import _native as nat
from grad_bench import synth, timed

REPS = 5
D_FEATURES, S_PATHS = 4096, 64
N_STARS = (65536, 1024)
N_TODAY = 2048


def spread(v):
    return [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)]


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [16384, 65536]
    lib = nat.lib()
    ctx = nat.default_context()
    d, noise, D, S = 8, 0.1, D_FEATURES, S_PATHS
    dev = torch.device("cuda:0")
    theta = 1.0 + np.arange(d) / 16.0
    _, pp, npar = nat.params_array(theta)
    k = cov_func(matern52_ard, l=theta)
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "paths_bench.txt")
    Xsh, _ = synth(max(N_STARS), d)
    Xs = torch.from_numpy(Xsh[::-1].copy()).to(dev)                  # test points: the same cloud, other points than the training set's first
    for n in sizes:
        n_pad = int(lib.gprc_pad(n))
        Xh, yh = synth(n, d)
        rng = np.random.Generator(np.random.Philox(20261019))
        nu = torch.from_numpy(np.ascontiguousarray(spectral_frequencies(k, d, D, rng).T)).to(dev)
        phase = torch.from_numpy(rng.random(D)).to(dev)
        W = torch.from_numpy(rng.standard_normal((S, D))).to(dev)   # row s = column s of W (D x S, column-major)
        E = torch.from_numpy(rng.standard_normal((S, n))).to(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g = GPR(Xh.T, yh, noise, k)
        fit_ms = (time.perf_counter() - t0) * 1e3
        h = C.c_void_p()

        def create():
            if h:
                nat.check(lib.gprc_gpr_paths_free(h))
            nat.check(lib.gprc_gpr_paths_create(g._model, nu.data_ptr(), phase.data_ptr(), D, W.data_ptr(), E.data_ptr(), S, C.byref(h)))

        t0 = time.perf_counter()
        create()
        create_first_ms = (time.perf_counter() - t0) * 1e3
        create_ms = statistics.median(timed(create, 3))
        U = torch.empty((S, n), dtype=torch.float64, device=dev)
        nat.check(lib.gprc_gpr_paths_get_weights(h, U.data_ptr()))
        Xd = torch.from_numpy(Xh).to(dev)
        rec = dict(n=n, n_pad=n_pad, d=d, D=D, S=S, kernel="matern52_ard", fit_ms=round(fit_ms, 1), create_first_ms=round(create_first_ms, 1),
                   create_ms=round(create_ms, 1), eval_ms={}, update_ms={}, yard_ms={}, update_gpairs={}, max_abs_diff={})
        for ns in N_STARS:
            out = torch.empty((S, ns), dtype=torch.float64, device=dev)
            rec["eval_ms"][ns] = round(statistics.median(timed(lambda: nat.check(lib.gprc_gpr_paths_eval(h, Xs.data_ptr(), ns, out.data_ptr(), ns)), REPS)), 2)
            # the update term alone against fill + GEMM: Ut (128 x n_pad, column-major) holds U^T, zero in the padding; C = -K* Ut^T
            m_pad = -(-ns // 128) * 128
            ld = m_pad + 128
            vt = torch.empty(ld * n_pad, dtype=torch.float64, device=dev)
            Ut = torch.zeros((n_pad, 128), dtype=torch.float64, device=dev)
            Ut[:n, :S] = U.T
            Cm = torch.zeros((128, m_pad), dtype=torch.float64, device=dev)
            upd = torch.empty((S, ns), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()

            def fused():
                nat.check(lib.gprc_dev_kernel_gemm(ctx.handle, nat.MATERN52_ARD, pp, npar, Xs.data_ptr(), ns, Xd.data_ptr(), n, d, U.data_ptr(), n, S,
                                                   upd.data_ptr(), ns))
                ctx.synchronize()

            def yard():
                Cm.zero_()
                torch.cuda.synchronize()
                t = time.perf_counter()
                nat.check(lib.gprc_dev_fill_cross(ctx.handle, nat.MATERN52_ARD, pp, npar, Xs.data_ptr(), d, ns, m_pad, Xd.data_ptr(), n, n_pad, vt.data_ptr(), ld))
                nat.check(lib.gprc_dev_gemm_nt(ctx.handle, Cm.data_ptr(), m_pad, vt.data_ptr(), ld, Ut.data_ptr(), 128, m_pad, 128, n_pad, 0))
                ctx.synchronize()
                return (time.perf_counter() - t) * 1e3

            fused()
            yard()                                                   # warm-up of both
            fu, ya = [], []
            for _ in range(REPS):
                t = time.perf_counter()
                fused()
                fu.append((time.perf_counter() - t) * 1e3)
                ya.append(yard())
            rec["update_ms"][ns], rec["yard_ms"][ns] = spread(fu), spread(ya)
            rec["update_gpairs"][ns] = round(ns * n_pad / statistics.median(fu) / 1e6, 1)
            rec["max_abs_diff"][ns] = float((upd + Cm[:S, :ns]).abs().max())
            del vt, Ut, Cm, upd, out
            nat.check(lib.gprc_ctx_trim(ctx.handle))
        nat.check(lib.gprc_gpr_paths_free(h))
        Xt = np.asfortranarray(Xsh[:N_TODAY].T)
        z = rng.standard_normal((S, N_TODAY)).T

        def today():
            mean, cov = g.predict(Xt, pointwise_var=False)
            multivariate_normal(S, mean[:, 0], cov, z=z)

        rec["today_ms"] = round(statistics.median(timed(today, 3)), 1)
        rec["today_n_star"] = N_TODAY
        g.close()
        nat.check(lib.gprc_ctx_trim(ctx.handle))
        line = json.dumps(rec)
        print(line, flush=True)
        with open(path, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
