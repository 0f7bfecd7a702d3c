"""Gradients of the posterior sample paths (gprc_gpr_paths_eval_grad) against the only route there was, central differences through
gprc_gpr_paths_eval, and one Thompson-sampling batch.  The shapes of tools/paths_bench.py: d = 8, noise 0.1, matern52_ard
(l_k = 1 + k / 16), D = 4096 features, S = 64 paths, tools/grad_bench.py's inputs, the draws from Philox seed 20261019, every array of
the timed calls resident in device memory.
    python tools/paths_grad_bench.py             # n = 16384 65536; appends to profiles/paths_grad_bench.txt
    python tools/paths_grad_bench.py 16384       # the n's named
Per n one JSON line; per n* in 65536, 1024, in ALTERNATING rounds of one process (host clock around a synchronous call), median and
(min, max) of REPS rounds after a warm-up of each:
  eval_grad_ms      gprc_gpr_paths_eval_grad with values and gradients (n* x S and n* x S x d)
  eval_ms           gprc_gpr_paths_eval
  diff_ms           2 d gprc_gpr_paths_eval calls, what central differences cost (the shifted points are not formed: the same points 2 d times)
  speedup           median diff_ms / median eval_grad_ms: the gradient kernel has no reason to exist below 1
  grad_max_rel      at n* = 1024: max |eval_grad - central differences at h = 1e-5| / max |gradient| (a plausibility figure, not a gate)
and, at the largest n only, one GPR.thompson_batch(64, [-1, 1]^d, n_starts = 32) with 1024 features:
  thompson_ms, thompson_evals, thompson_ms_per_iter  (the evaluations from SamplePaths.maximize on the same draws)
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
from gprc_amd import GPR, cov_func, matern52_ard, spectral_frequencies
from gprc_amd import _native as nat
from grad_bench import synth

REPS = 5
D_FEATURES, S_PATHS = 4096, 64
N_STARS = (65536, 1024)
H_DIFF = 1e-5


def spread(v):
    return [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)]


def clock(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [16384, 65536]
    lib = nat.lib()
    ctx = nat.default_context()
    d, noise, D, S = 8, 0.1, D_FEATURES, S_PATHS
    dev = torch.device("cuda:0")
    theta = 1.0 + np.arange(d) / 16.0
    k = cov_func(matern52_ard, l=theta)
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "paths_grad_bench.txt")
    Xsh, _ = synth(max(N_STARS), d)
    Xs = torch.from_numpy(Xsh[::-1].copy()).to(dev)                  # test points: the same cloud, other points than the training set's first
    for n in sizes:
        Xh, yh = synth(n, d)
        rng = np.random.Generator(np.random.Philox(20261019))
        nu = torch.from_numpy(np.ascontiguousarray(spectral_frequencies(k, d, D, rng).T)).to(dev)
        phase = torch.from_numpy(rng.random(D)).to(dev)
        W = torch.from_numpy(rng.standard_normal((S, D))).to(dev)   # row s = column s of W (D x S, column-major)
        E = torch.from_numpy(rng.standard_normal((S, n))).to(dev)
        torch.cuda.synchronize()
        g = GPR(Xh.T, yh, noise, k)
        h = C.c_void_p()
        nat.check(lib.gprc_gpr_paths_create(g._model, nu.data_ptr(), phase.data_ptr(), D, W.data_ptr(), E.data_ptr(), S, C.byref(h)))
        rec = dict(n=n, d=d, D=D, S=S, kernel="matern52_ard", eval_grad_ms={}, eval_ms={}, diff_ms={}, speedup={})
        for ns in N_STARS:
            out = torch.empty((S, ns), dtype=torch.float64, device=dev)
            dout = torch.empty((d, S, ns), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()

            def eval_grad():
                nat.check(lib.gprc_gpr_paths_eval_grad(h, Xs.data_ptr(), ns, out.data_ptr(), ns, dout.data_ptr(), ns))

            def value(x=Xs):
                nat.check(lib.gprc_gpr_paths_eval(h, x.data_ptr(), ns, out.data_ptr(), ns))

            def differences():
                for _ in range(2 * d):
                    value()

            eval_grad()
            differences()                                            # warm-up of all three
            eg, ev, df = [], [], []
            for _ in range(REPS):
                eg.append(clock(eval_grad))
                ev.append(clock(value))
                df.append(clock(differences))
            rec["eval_grad_ms"][ns], rec["eval_ms"][ns], rec["diff_ms"][ns] = spread(eg), spread(ev), spread(df)
            rec["speedup"][ns] = round(statistics.median(df) / statistics.median(eg), 2)
            if ns == min(N_STARS):                                   # plausibility: real central differences at the small shape
                eval_grad()
                worst = 0.0
                for c in range(d):
                    step = torch.zeros_like(Xs[:ns])
                    step[:, c] = H_DIFF
                    value(Xs[:ns] + step)
                    hi = out.clone()
                    value(Xs[:ns] - step)
                    worst = max(worst, float(((hi - out) / (2.0 * H_DIFF) - dout[c]).abs().max()))
                rec["grad_max_rel"] = worst / float(dout.abs().max())
            del out, dout
            nat.check(lib.gprc_ctx_trim(ctx.handle))
        nat.check(lib.gprc_gpr_paths_free(h))
        if n == max(sizes):
            lower, upper = -np.ones(d), np.ones(d)
            t0 = time.perf_counter()
            batch = g.thompson_batch(64, lower, upper, n_starts=32, rng=np.random.default_rng(7))
            rec["thompson_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            r2 = np.random.default_rng(7)
            with g.sample_paths(64, 1024, rng=r2) as sp:
                t0 = time.perf_counter()
                res = sp.maximize(lower, upper, n_starts=32, rng=r2)
                ascent_ms = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(res.x_best, batch)
            rec["thompson_evals"] = res.n_evals
            rec["thompson_ms_per_iter"] = round(ascent_ms / res.n_evals, 2)
            rec["thompson_converged"] = "%d of %d" % (int((res.pg <= 1e-8).sum()), res.pg.size)
        g.close()
        nat.check(lib.gprc_ctx_trim(ctx.handle))
        line = json.dumps(rec)
        print(line, flush=True)
        with open(path, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
