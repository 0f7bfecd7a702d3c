"""A fitted batch of small GPs (gprc_gpr_batch_fit + gprc_gpr_batch_predict): what fitting B models and predicting from all of them costs
beside the only route there was before, B times gprc_gpr_fit + gprc_gpr_predict on the same models.  Records, not thresholds.
    python tools/batch_predict_bench.py                     # appends JSON lines to profiles/batch_predict_bench.txt
    python tools/batch_predict_bench.py --reps 9
matern52_ard, d = 8, noise 0.1, host arrays, one data set and one set of test points shared by the models of a batch, length scales
l_k = (1 + k / 16) times a factor per model, log-uniform in [1/2, 2] from default_rng(20261020); the raw C-ABI calls on both routes.
  n in {32, 128} x B in {1, 64, 256, 1024} x n* in {1, 64, 1024} test points a model:
    batch_ms    one gprc_gpr_batch_fit + one gprc_gpr_batch_predict (mean and variance) + the free
    seq_ms      B x (gprc_gpr_fit + gprc_gpr_predict(pointwise = 1) + the free)
    predict_ms  gprc_gpr_batch_predict alone on a fitted batch; predict_mean_ms: the same without var_out
  each the median of --reps timed repeats after one warm-up of the same shape, the routes alternating; min and max beside the median;
  max_rel_diff: the largest difference between the two routes' outputs (mean normwise, variance per component).
Every (n, B) runs in a process of its own under a time limit (--limit seconds); the first one that fails or runs out of time ends the
run, and nothing is started after it.
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
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def stats(ms):
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))


def one_shape(n, B, reps):
    """the child: the three n* of one (n, B), a JSON line each on stdout"""
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

    def fit_batch():
        h = C.c_void_p()
        nat.check(lib.gprc_gpr_batch_fit(ctx.handle, kid, B, thetas.ctypes.data, D, D, noises.ctypes.data, X.ctypes.data, D, n, 0, y.ctypes.data, 0, None,
                                         C.byref(h), lp.ctypes.data, info.ctypes.data))
        return h

    for ns in STARS:
        Xs = np.asfortranarray(rng.uniform(-2, 2, (D, ns)))
        mean, var = np.empty((B, ns)), np.empty((B, ns))
        smean, svar = np.empty((B, ns)), np.empty((B, ns))

        def predict(h, with_var=True):
            nat.check(lib.gprc_gpr_batch_predict(h, Xs.ctypes.data, ns, 0, None, mean.ctypes.data, var.ctypes.data if with_var else None, ns))

        def batched():
            h = fit_batch()
            predict(h)
            lib.gprc_batch_model_free(h)

        def sequential():
            for b in range(B):
                m = C.c_void_p()
                nat.check(lib.gprc_gpr_fit(ctx.handle, kid, thetas[b].ctypes.data_as(dp), D, X.ctypes.data, D, n, y.ctypes.data, NOISE, C.byref(m)))
                nat.check(lib.gprc_gpr_predict(m, Xs.ctypes.data, ns, 1, smean[b].ctypes.data, svar[b].ctypes.data))
                lib.gprc_model_free(m)

        batched()
        sequential()
        tb, ts, tp, tm = [], [], [], []
        for _ in range(reps):
            tb.append(timed(batched)[0])
            ts.append(timed(sequential)[0])
        diff = max(float(np.abs(mean - smean).max() / np.abs(smean).max()), float((np.abs(var - svar) / np.abs(svar)).max()))
        h = fit_batch()
        predict(h)
        predict(h, False)
        for _ in range(reps):
            tp.append(timed(lambda: predict(h))[0])
            tm.append(timed(lambda: predict(h, False))[0])
        lib.gprc_batch_model_free(h)
        rec = dict(n=n, B=B, n_star=ns, batch_ms=stats(tb), seq_ms=stats(ts), speedup=round(statistics.median(ts) / statistics.median(tb), 2),
                   predict_ms=stats(tp), predict_mean_ms=stats(tm), per_model_us=round(1e3 * statistics.median(tb) / B, 2),
                   max_rel_diff=float("%.2e" % diff), bad=int(np.count_nonzero(info)))
        print(json.dumps(rec), flush=True)


def main():
    reps, limit = option("--reps", 7), option("--limit", 240)
    if "--shape" in sys.argv:
        i = sys.argv.index("--shape")
        return one_shape(int(sys.argv[i + 1]), int(sys.argv[i + 2]), reps)
    out_path = os.path.join(ROOT, "profiles", "batch_predict_bench.txt")
    for n in SIZES:
        for B in BATCHES:
            cmd = [sys.executable, os.path.abspath(__file__), "--shape", str(n), str(B), "--reps", str(reps)]
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit)
            except subprocess.TimeoutExpired:
                sys.exit(f"n = {n}, B = {B}: no result after {limit} s; nothing more is started")
            if r.returncode != 0:
                sys.exit(f"n = {n}, B = {B}: the step ended with status {r.returncode}; nothing more is started")
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            with open(out_path, "a") as f:
                f.write(r.stdout)


if __name__ == "__main__":
    main()
