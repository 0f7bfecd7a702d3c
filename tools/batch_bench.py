"""Small GPs in batches (gprc_gpr_batch_logp_grad): what one batched call costs beside the only route there was before it, B sequential
gprc_gpr_logp_grad calls on the same models, and optimize_multistart beside as many optimize calls.  Records, not thresholds.
    python tools/batch_bench.py                     # appends JSON lines to profiles/batch_bench.txt
    python tools/batch_bench.py --reps 9 --starts 32
matern52_ard, d = 8, noise 0.1, host arrays (what fit.py passes), one data set shared by the models of a batch, length scales
l_k = (1 + k / 16) times a factor per model, log-uniform in [1/2, 2] from default_rng(20261020).
  call       n in {32, 64, 128} x B in {1, 64, 256, 1024}: batch_ms of one batched call and seq_ms of B sequential single-model calls, each
             the median of --reps timed repeats after one warm-up of the same shape, the two alternating; min and max beside the median;
             the largest difference between the two routes' outputs
  multistart n = 128: one optimize_multistart of --starts starts beside --starts optimize calls from the same starts (once each, after a
             warm-up of both on two starts), with the number of device calls each made and the best value each found
"""
import importlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import gprc_amd  # noqa: F401
from gprc_amd import _native as nat

F = importlib.import_module("gprc_amd.fit")
NAME, D, NOISE, SEED = "matern52_ard", 8, 0.1, 20261020


def option(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def problem(n, B, rng):
    X = np.asfortranarray(rng.uniform(-2, 2, (D, n)))
    y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
    ell = 1.0 + np.arange(D) / 16.0
    return X, y, ell[None, :] * np.exp(rng.uniform(-np.log(2.0), np.log(2.0), (B, 1)))


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def stats(ms):
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))


def main():
    reps, starts = option("--reps", 7), option("--starts", 32)
    out_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "batch_bench.txt")
    rng = np.random.default_rng(SEED)
    ctx = nat.default_context()
    lines = []
    for n in (32, 64, 128):
        for B in (1, 64, 256, 1024):
            X, y, thetas = problem(n, B, rng)
            batched = lambda: F.logp_grad_batch(X, y, NOISE, NAME, thetas, ctx)                        # noqa: E731
            sequential = lambda: [F.logp_grad(X, y, NOISE, NAME, th, ctx) for th in thetas]            # noqa: E731
            _, (lp, g, info) = timed(batched)
            _, single = timed(sequential)
            tb, ts = [], []
            for _ in range(reps):
                tb.append(timed(batched)[0])
                ts.append(timed(sequential)[0])
            diff = max(max(abs(lp[b] - single[b][0]) / abs(single[b][0]), float(np.abs(g[b] - single[b][1]).max() / np.abs(single[b][1]).max()))
                       for b in range(B))
            rec = dict(leg="call", n=n, B=B, batch_ms=stats(tb), seq_ms=stats(ts), speedup=round(statistics.median(ts) / statistics.median(tb), 2),
                       per_model_us=round(1e3 * statistics.median(tb) / B, 2), max_rel_diff=float("%.2e" % diff), bad=int(np.count_nonzero(info)))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    # multi-start
    n = 128
    X, y, thetas = problem(n, starts, rng)
    calls = dict(batch=0, single=0)
    real_b, real_s = F.logp_grad_batch, F.logp_grad

    def count_b(*a, **k):
        calls["batch"] += 1
        return real_b(*a, **k)

    def count_s(*a, **k):
        calls["single"] += 1
        return real_s(*a, **k)

    F.logp_grad_batch, F.logp_grad = count_b, count_s
    try:
        F.optimize_multistart(X, y, NOISE, NAME, thetas[:2], ctx=ctx)
        [F.optimize(X, y, NOISE, NAME, th, ctx=ctx) for th in thetas[:2]]
        calls.update(batch=0, single=0)
        t_multi, r = timed(lambda: F.optimize_multistart(X, y, NOISE, NAME, thetas, ctx=ctx))
        t_seq, rs = timed(lambda: [F.optimize(X, y, NOISE, NAME, th, ctx=ctx) for th in thetas])
    finally:
        F.logp_grad_batch, F.logp_grad = real_b, real_s
    rec = dict(leg="multistart", n=n, starts=starts, multistart_ms=round(t_multi, 2), optimize_ms=round(t_seq, 2), speedup=round(t_seq / t_multi, 2),
               device_calls_multistart=calls["batch"], device_calls_optimize=calls["single"], best_multistart=r["value"],
               best_optimize=max(a["value"] for a in rs), same_results=all(a["value"] == b["value"] for a, b in zip(r["all"], rs)))
    print(json.dumps(rec), flush=True)
    lines.append(rec)
    with open(out_path, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
