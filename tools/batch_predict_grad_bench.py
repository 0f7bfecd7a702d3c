"""Prediction gradients and LOO of a fitted batch of small GPs (gprc_gpr_batch_predict_grad, gprc_gpr_batch_loo): what they cost beside
the only routes there were before, B times gprc_gpr_fit + gprc_gpr_predict_grad and B times gprc_gpr_loo on the same models, and beside
gprc_gpr_batch_predict of the same shape (the gradients' own cost).  Records, not thresholds.
    python tools/batch_predict_grad_bench.py                # appends JSON lines to profiles/batch_predict_grad_bench.txt
    python tools/batch_predict_grad_bench.py --reps 9
matern52_ard, d = 8, noise 0.1, host arrays, one data set and one set of test points shared by the models of a batch, length scales
l_k = (1 + k / 16) times a factor per model, log-uniform in [1/2, 2] from default_rng(20261020) (tools/batch_predict_bench.py's
models); the raw C-ABI calls on every route.
  n in {32, 128} x B in {1, 64, 256, 1024} x n* in {1, 64, 1024} test points a model:
    grad_ms        one gprc_gpr_batch_predict_grad (all four outputs) on a fitted batch
    grad_mean_ms   the same with var_out and dvar_out NULL (no product with L^-1 or L^-T)
    predict_ms     gprc_gpr_batch_predict (mean and variance) on the same batch and points
    seq_ms         B x (gprc_gpr_fit + gprc_gpr_predict_grad + the free)
    batch_ms       one gprc_gpr_batch_fit + one gprc_gpr_batch_predict_grad + the free, the route seq_ms stands beside
    loo_ms, seq_loo_ms   (at the first n* only: LOO has no test points) one gprc_gpr_batch_loo, all four outputs, beside B x
                   gprc_gpr_loo on single models fitted and freed outside the timed part
  each the median of --reps timed repeats after one warm-up of the same shape, the routes alternating; min and max beside the median;
  max_rel_diff: the largest normwise difference between the two routes' gradients.
Every (n, B, n*) runs in a process of its own under a time limit (--limit seconds); the first one that fails or runs out of time ends
the run, and nothing is started after it.
"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAME, D, NOISE, SEED = "matern52_ard", 8, 0.1, 20261020
SIZES, BATCHES, STARS = (32, 128), (1, 64, 256, 1024), (1, 64, 1024)


def option(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))


def one_shape(n, B, ns, reps):
    """the child: one (n, B, n*), a JSON line on stdout"""
    import numpy as np

    import gprc_amd  # noqa: F401
    from gprc_amd import _native as nat
    from gprc_amd.fit import grad_dict

    lib, ctx, kid = nat.lib(), nat.default_context(), grad_dict[NAME].kernel_id
    rng = np.random.default_rng(SEED + 1000 * n + B)
    X = np.asfortranarray(rng.uniform(-2, 2, (D, n)))
    y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
    thetas = np.ascontiguousarray((1.0 + np.arange(D) / 16.0)[None, :] * np.exp(rng.uniform(-np.log(2.0), np.log(2.0), (B, 1))))
    noises = np.full(B, NOISE)
    lp, info = np.empty(B), np.zeros(B, dtype=np.intc)
    dp = C.POINTER(C.c_double)
    Xs = np.asfortranarray(np.random.default_rng(SEED + ns).uniform(-2, 2, (D, ns)))
    mean, var, dmean, dvar = np.empty((B, ns)), np.empty((B, ns)), np.empty((B, D * ns)), np.empty((B, D * ns))
    smean, svar, sdmean, sdvar = np.empty((B, ns)), np.empty((B, ns)), np.empty((B, D * ns)), np.empty((B, D * ns))

    def fit_batch():
        h = C.c_void_p()
        nat.check(lib.gprc_gpr_batch_fit(ctx.handle, kid, B, thetas.ctypes.data, D, D, noises.ctypes.data, X.ctypes.data, D, n, 0, y.ctypes.data, 0, None,
                                         C.byref(h), lp.ctypes.data, info.ctypes.data))
        return h

    def fit_single(b):
        m = C.c_void_p()
        nat.check(lib.gprc_gpr_fit(ctx.handle, kid, thetas[b].ctypes.data_as(dp), D, X.ctypes.data, D, n, y.ctypes.data, NOISE, C.byref(m)))
        return m

    def grad(h, with_var=True):
        nat.check(lib.gprc_gpr_batch_predict_grad(h, Xs.ctypes.data, ns, 0, None, mean.ctypes.data, var.ctypes.data if with_var else None, ns,
                                                  dmean.ctypes.data, dvar.ctypes.data if with_var else None, D * ns))

    def predict(h):
        nat.check(lib.gprc_gpr_batch_predict(h, Xs.ctypes.data, ns, 0, None, mean.ctypes.data, var.ctypes.data, ns))

    def batched():
        h = fit_batch()
        grad(h)
        lib.gprc_batch_model_free(h)

    def sequential():
        for b in range(B):
            m = fit_single(b)
            nat.check(lib.gprc_gpr_predict_grad(m, Xs.ctypes.data, ns, smean[b].ctypes.data, svar[b].ctypes.data, sdmean[b].ctypes.data, sdvar[b].ctypes.data))
            lib.gprc_model_free(m)

    batched()
    sequential()
    tb, ts, tg, tm, tp = [], [], [], [], []
    for _ in range(reps):
        tb.append(timed(batched))
        ts.append(timed(sequential))
    diff = max(float(np.abs(dmean - sdmean).max() / np.abs(sdmean).max()), float(np.abs(dvar - sdvar).max() / np.abs(sdvar).max()))
    h = fit_batch()
    grad(h)
    grad(h, False)
    predict(h)
    for _ in range(reps):
        tg.append(timed(lambda: grad(h)))
        tm.append(timed(lambda: grad(h, False)))
        tp.append(timed(lambda: predict(h)))
    rec = dict(n=n, B=B, n_star=ns, grad_ms=stats(tg), grad_mean_ms=stats(tm), predict_ms=stats(tp), batch_ms=stats(tb), seq_ms=stats(ts),
               speedup=round(statistics.median(ts) / statistics.median(tb), 2), grad_over_predict=round(statistics.median(tg) / statistics.median(tp), 2),
               max_rel_diff=float("%.2e" % diff), bad=int(np.count_nonzero(info)))
    if ns == STARS[0]:
        lm, lv, ld, sc = np.empty((B, n)), np.empty((B, n)), np.empty((B, n)), np.empty(B)
        one = [np.empty(n) for _ in range(3)]
        score = C.c_double()

        def loo():
            nat.check(lib.gprc_gpr_batch_loo(h, lm.ctypes.data, lv.ctypes.data, ld.ctypes.data, n, sc.ctypes.data))

        def seq_loo():
            total = 0.0
            for b in range(B):
                m = fit_single(b)
                total += timed(lambda: nat.check(lib.gprc_gpr_loo(m, one[0].ctypes.data, one[1].ctypes.data, one[2].ctypes.data, C.byref(score))))
                lib.gprc_model_free(m)
            return total

        loo()
        seq_loo()
        tl, tsl = [], []
        for _ in range(reps):
            tl.append(timed(loo))
            tsl.append(seq_loo())
        rec.update(loo_ms=stats(tl), seq_loo_ms=stats(tsl), loo_speedup=round(statistics.median(tsl) / statistics.median(tl), 2))
    lib.gprc_batch_model_free(h)
    print(json.dumps(rec), flush=True)


def main():
    reps, limit = option("--reps", 7), option("--limit", 240)
    if "--shape" in sys.argv:
        i = sys.argv.index("--shape")
        return one_shape(int(sys.argv[i + 1]), int(sys.argv[i + 2]), int(sys.argv[i + 3]), reps)
    out_path = os.path.join(ROOT, "profiles", "batch_predict_grad_bench.txt")
    for n in SIZES:
        for B in BATCHES:
            for ns in STARS:
                cmd = [sys.executable, os.path.abspath(__file__), "--shape", str(n), str(B), str(ns), "--reps", str(reps)]
                try:
                    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit)
                except subprocess.TimeoutExpired:
                    sys.exit(f"n = {n}, B = {B}, n* = {ns}: no result after {limit} s; nothing more is started")
                if r.returncode != 0:
                    sys.exit(f"n = {n}, B = {B}, n* = {ns}: the step ended with status {r.returncode}; nothing more is started")
                sys.stdout.write(r.stdout)
                sys.stdout.flush()
                with open(out_path, "a") as f:
                    f.write(r.stdout)


if __name__ == "__main__":
    main()
