"""The batched and the local classifier (gprc_gpc_batch_fit, gprc_gpc_batch_predict_latent, gprc_lgpc_predict): what one batched fit
costs beside the only route there was before it, B sequential gprc_gpc_fit calls on the same models, and what a local classification
costs with the search's share of it.  Records, and one floor: the batched fit of 256 models is at least 10 x faster than the 256 single
calls of the same run (the loop stayed on the CU), else the run ends with an error.
    python tools/batch_gpc_bench.py                      # appends JSON lines to profiles/batch_gpc_bench.txt
    python tools/batch_gpc_bench.py --out FILE --reps 9
matern52_ard, d = 8, l_c = 1 + c / 16, X uniform in [-1, 1]^d, labels as tests/gpu_calls.gpc_problem draws them
(sign(x_0 - x_7 / 2 + 0.3 N(0, 1))), from default_rng(20261021 + the shape); epsilon = 1e-10, host arrays.
  fit      B in {256, 1024} models of 128 points, a data set each: batch_ms of one gprc_gpc_batch_fit (free included) beside seq_ms of B
           gprc_gpc_fit calls (flags 0, the same epsilon; free included), the two alternating; fit_predict_ms: the batched fit and
           gprc_gpc_batch_predict_latent at 64 test points a model; the iterations the models took, the largest difference in logq
  local    gprc_lgpc_predict (latent mean, variance and class probability, host arrays) of n* in {1024, 65 536} points on a model of
           n in {65 536, 2^20} created once, m in {32, 64, 128}; knn_ms: gprc_lgpr_neighbours of the same points with device outputs,
           the search's share of it
  each time the median of --reps timed repeats after one warm-up of the same shape; min and max beside the median.
Every shape runs in a process of its own under a time limit (--limit seconds); the first one that fails or runs out of time ends the run,
and nothing is started after it.
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
NAME, D, EPSILON, SEED, N_B, NS_B = "matern52_ard", 8, 1e-10, 20261021, 128, 64
FIT_SHAPES = [(256,), (1024,)]
LOCAL_SHAPES = [(n, ns) for n in (65536, 1048576) for ns in (1024, 65536)]
MS = (32, 64, 128)
FLOOR = 10.0


def option(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def stats(ms):
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))


def labelled(rng, n):
    import numpy as np
    X = rng.uniform(-1, 1, (D, n))
    y = np.sign(X[0] - 0.5 * X[D - 1] + 0.3 * rng.normal(size=n))
    y[y == 0] = 1.0
    return np.asfortranarray(X), np.ascontiguousarray(y)


def fit_shape(B, reps):
    import numpy as np

    import gprc_amd  # noqa: F401
    from gprc_amd import _native as nat
    from gprc_amd.fit import grad_dict

    lib, ctx, kid = nat.lib(), nat.default_context(), grad_dict[NAME].kernel_id
    rng = np.random.default_rng(SEED + B)
    sets = [labelled(rng, N_B) for _ in range(B)]
    Xb = np.ascontiguousarray(np.stack([X.ravel(order="F") for X, _ in sets]))
    yb = np.ascontiguousarray(np.stack([y for _, y in sets]))
    Xs = np.ascontiguousarray(rng.uniform(-1, 1, (B, D * NS_B)))
    thetas = np.ascontiguousarray(np.tile(1.0 + np.arange(D) / 16.0, (B, 1)))
    dp = C.POINTER(C.c_double)
    logq, iters, info = np.empty(B), np.zeros(B, dtype=np.intc), np.zeros(B, dtype=np.intc)
    fs, vf = np.empty((B, NS_B)), np.empty((B, NS_B))
    single_logq = np.empty(B)

    def batched(predict=False):
        h = C.c_void_p()
        nat.check(lib.gprc_gpc_batch_fit(ctx.handle, kid, B, thetas.ctypes.data, D, D, Xb.ctypes.data, D, N_B, D * N_B, yb.ctypes.data, N_B, None, EPSILON, 0,
                                         C.byref(h), logq.ctypes.data, iters.ctypes.data, info.ctypes.data))
        if predict:
            nat.check(lib.gprc_gpc_batch_predict_latent(h, Xs.ctypes.data, NS_B, D * NS_B, None, fs.ctypes.data, vf.ctypes.data, NS_B))
        lib.gprc_batch_model_free(h)

    def sequential():
        for b in range(B):
            h, it = C.c_void_p(), C.c_int()
            nat.check(lib.gprc_gpc_fit(ctx.handle, kid, thetas[b].ctypes.data_as(dp), D, Xb[b].ctypes.data, D, N_B, yb[b].ctypes.data, EPSILON, 0, 0, C.byref(h),
                                       C.byref(it)))
            lib.gprc_model_free(h)

    def single_values():       # the evidence of every model by the single-model route, once, for the difference
        lq, it, g = C.c_double(), C.c_int(), np.empty(D)
        for b in range(B):
            nat.check(lib.gprc_gpc_logq_grad(ctx.handle, kid, thetas[b].ctypes.data_as(dp), D, Xb[b].ctypes.data, D, N_B, yb[b].ctypes.data, EPSILON, 0,
                                             C.byref(lq), g.ctypes.data_as(dp), C.byref(it)))
            single_logq[b] = lq.value

    batched()
    sequential()
    tb, ts = [], []
    for _ in range(reps):
        tb.append(timed(batched)[0])
        ts.append(timed(sequential)[0])
    batched(True)
    tp = [timed(lambda: batched(True))[0] for _ in range(reps)]
    single_values()
    speedup = statistics.median(ts) / statistics.median(tb)
    print(json.dumps(dict(kind="fit", d=D, n=N_B, B=B, batch_ms=stats(tb), seq_ms=stats(ts), speedup=round(speedup, 2),
                          per_model_us=round(1e3 * statistics.median(tb) / B, 2), fit_predict_ms=stats(tp), n_star_each=NS_B,
                          iters=[int(iters.min()), int(iters.max())], max_rel_diff_logq=float("%.2e" % np.abs((logq - single_logq) / single_logq).max()),
                          bad=int(np.count_nonzero(info)))), flush=True)
    if B == 256 and speedup < FLOOR:
        sys.exit(f"the batched fit of 256 models is {speedup:.1f} x faster than 256 single calls: below the floor of {FLOOR:.0f} x")


def local_shape(n, ns, reps):
    import numpy as np
    import torch

    import gprc_amd  # noqa: F401
    from gprc_amd import _native as nat
    from gprc_amd.fit import grad_dict

    lib, ctx, kid = nat.lib(), nat.default_context(), grad_dict[NAME].kernel_id
    rng = np.random.default_rng(SEED + n % 1000 + ns % 100)
    X, y = labelled(rng, n)
    Xs = np.asfortranarray(rng.uniform(-1, 1, (D, ns)))
    ell = 1.0 + np.arange(D) / 16.0
    dp = C.POINTER(C.c_double)
    fs, vf, prob = np.empty(ns), np.empty(ns), np.empty(ns)
    iters, info = np.zeros(ns, dtype=np.intc), np.zeros(ns, dtype=np.intc)
    for m in MS:
        h = C.c_void_p()
        nat.check(lib.gprc_lgpc_create(ctx.handle, kid, ell.ctypes.data_as(dp), D, X.ctypes.data, D, n, y.ctypes.data, m, EPSILON, 0, C.byref(h)))
        idx = torch.empty((ns, m), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def predict():
            nat.check(lib.gprc_lgpc_predict(h, Xs.ctypes.data, ns, fs.ctypes.data, vf.ctypes.data, prob.ctypes.data, iters.ctypes.data, info.ctypes.data))

        def search():
            nat.check(lib.gprc_lgpr_neighbours(h, Xs.ctypes.data, ns, idx.data_ptr(), None, m))

        predict()
        tp = [timed(predict)[0] for _ in range(reps)]
        search()
        tk = [timed(search)[0] for _ in range(reps)]
        lib.gprc_lgpr_free(h)
        print(json.dumps(dict(kind="local", d=D, n=n, n_star=ns, m=m, predict_ms=stats(tp), knn_ms=stats(tk),
                              per_point_us=round(1e3 * statistics.median(tp) / ns, 3), iters=[int(iters.min()), int(iters.max())],
                              bad=int(np.count_nonzero(info)))), flush=True)


def main():
    reps, limit = option("--reps", 7), option("--limit", 240)
    if "--shape" in sys.argv:
        a = sys.argv[sys.argv.index("--shape") + 1:]
        if a[0] == "fit":
            return fit_shape(int(a[1]), reps)
        return local_shape(int(a[1]), int(a[2]), reps)
    out_path = option("--out", os.path.join(ROOT, "profiles", "batch_gpc_bench.txt"), str)
    shapes = [("fit",) + s for s in FIT_SHAPES] + [("local",) + s for s in LOCAL_SHAPES]
    for shape in shapes:
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(reps), "--shape"] + [str(v) for v in shape]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"{shape}: no result after {limit} s; nothing more is started")
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        with open(out_path, "a") as f:
            f.write(r.stdout)
        if r.returncode != 0:
            sys.exit(f"{shape}: the step ended with status {r.returncode}; nothing more is started")


if __name__ == "__main__":
    main()
