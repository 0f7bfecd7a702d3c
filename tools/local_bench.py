"""The local GPR (gprc_dev_knn, gprc_lgpr_predict): what the neighbour search costs alone, what a local prediction costs, and how far it is
from the exact GP where both can run.  Records, not thresholds.
    python tools/local_bench.py                      # appends JSON lines to profiles/local_bench.txt
    python tools/local_bench.py --out FILE --reps 9
matern52_ard, d = 8 (the search also at d = 3), noise 0.1, X uniform in [-2, 2]^d, y = sin(sum x) + 0.1 N(0, 1), l_c = 1 + c / 16, from
default_rng(20261020 + the shape).
  knn      gprc_dev_knn alone, m = 64, device pointers for inputs and outputs (torch tensors), Euclidean and scaled:
           pairs_per_ns = n n* / time, beside the covariance fills' recorded 393 - 421 pairs per ns per coordinate group
           ("Sparse GPR gradient"; at d = 8, three groups): a comparison figure, not a target
  predict  gprc_lgpr_predict (mean and variance, host arrays) on a model created once, m in {32, 64, 128}; knn_ms: gprc_lgpr_neighbours of
           the same points with device outputs, the search's share of it
  exact    n = 16 384, n* = 1024, d = 8 and d = 2 (the same 16 384 points fill two dimensions far more densely than eight): the local
           prediction for m in {32, 64, 128} beside GPR(...).predict on the same data: both routes' times
           (the exact route's fit and predict apart) and the RMS and maximum difference of mean and variance
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
NAME, D, NOISE, SEED = "matern52_ard", 8, 0.1, 20261020
KNN_SHAPES = [(d, n, ns) for d in (3, 8) for n in (65536, 1048576) for ns in (1024, 65536)]
PREDICT_SHAPES = [(n, ns) for n in (65536, 1048576) for ns in (1024, 65536)]
MS = (32, 64, 128)
EXACT_DIMS = (8, 2)


def option(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def stats(ms):
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))


def repeat(f, reps):
    f()
    return [timed(f)[0] for _ in range(reps)]


def problem(d, n, ns, seed):
    import numpy as np
    rng = np.random.default_rng(SEED + seed)
    X = np.asfortranarray(rng.uniform(-2, 2, (d, n)))
    y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
    Xs = np.asfortranarray(rng.uniform(-2, 2, (d, ns)))
    return X, y, Xs, 1.0 + np.arange(d) / 16.0


def knn_shape(d, n, ns, reps):
    import numpy as np
    import torch

    import gprc_amd  # noqa: F401
    from gprc_amd import _native as nat

    lib, ctx, m = nat.lib(), nat.default_context(), 64
    X, _, Xs, ell = problem(d, n, ns, 7 * d + n % 1000 + ns % 100)
    xd, xsd = torch.from_numpy(X.ravel(order="F").copy()).cuda(), torch.from_numpy(Xs.ravel(order="F").copy()).cuda()
    idx = torch.empty((ns, m), dtype=torch.int32, device="cuda")
    dist = torch.empty((ns, m), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for scale in (None, np.ascontiguousarray(1.0 / ell)):
        def run():
            nat.check(lib.gprc_dev_knn(ctx.handle, xd.data_ptr(), d, n, xsd.data_ptr(), ns, None if scale is None else scale.ctypes.data, m,
                                       idx.data_ptr(), dist.data_ptr(), m))
        ms = repeat(run, reps)
        med = statistics.median(ms)
        print(json.dumps(dict(kind="knn", d=d, n=n, n_star=ns, m=m, scaled=scale is not None, ms=stats(ms),
                              pairs_per_ns=round(n * ns / (med * 1e6), 2), coord_pairs_per_ns=round(n * ns * d / (med * 1e6), 2))), flush=True)


def predict_shape(n, ns, reps):
    import numpy as np
    import torch

    import gprc_amd  # noqa: F401
    from gprc_amd import _native as nat
    from gprc_amd.fit import grad_dict

    lib, ctx, kid = nat.lib(), nat.default_context(), grad_dict[NAME].kernel_id
    X, y, Xs, ell = problem(D, n, ns, n % 1000 + ns % 100)
    dp = C.POINTER(C.c_double)
    mean, var, info = np.empty(ns), np.empty(ns), np.zeros(ns, dtype=np.intc)
    for m in MS:
        h = C.c_void_p()
        nat.check(lib.gprc_lgpr_create(ctx.handle, kid, ell.ctypes.data_as(dp), D, X.ctypes.data, D, n, y.ctypes.data, NOISE, m, C.byref(h)))
        idx = torch.empty((ns, m), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        tp = repeat(lambda: nat.check(lib.gprc_lgpr_predict(h, Xs.ctypes.data, ns, mean.ctypes.data, var.ctypes.data, info.ctypes.data)), reps)
        tk = repeat(lambda: nat.check(lib.gprc_lgpr_neighbours(h, Xs.ctypes.data, ns, idx.data_ptr(), None, m)), reps)
        lib.gprc_lgpr_free(h)
        print(json.dumps(dict(kind="predict", d=D, n=n, n_star=ns, m=m, predict_ms=stats(tp), knn_ms=stats(tk),
                              per_point_us=round(1e3 * statistics.median(tp) / ns, 3), bad=int(np.count_nonzero(info)))), flush=True)


def exact_shape(d, reps):
    import numpy as np

    import gprc_amd  # noqa: F401
    from gprc_amd import GPR, LocalGPR, cov_func, matern52_ard

    n, ns = 16384, 1024
    X, y, Xs, ell = problem(d, n, ns, 16384 + d)
    k = cov_func(matern52_ard, l=ell)
    fit_ms = repeat(lambda: GPR(X, y, NOISE, k), min(reps, 3))
    g = GPR(X, y, NOISE, k)
    want = g.predict(Xs)
    exact_ms = repeat(lambda: g.predict(Xs), reps)
    for m in MS:
        with LocalGPR(X, y, NOISE, k, m=m) as lg:
            got = lg.predict(Xs)
            local_ms = repeat(lambda: lg.predict(Xs), reps)
            bad = int(np.count_nonzero(lg.info))
        dm, dv = got[:, 0] - want[:, 0], got[:, 1] - want[:, 1]
        print(json.dumps(dict(kind="exact", d=d, n=n, n_star=ns, m=m, local_ms=stats(local_ms), exact_fit_ms=stats(fit_ms), exact_predict_ms=stats(exact_ms),
                              mean_rms_diff=float("%.3e" % np.sqrt(np.mean(dm * dm))), mean_max_diff=float("%.3e" % np.abs(dm).max()),
                              var_rms_diff=float("%.3e" % np.sqrt(np.mean(dv * dv))), var_max_diff=float("%.3e" % np.abs(dv).max()),
                              y_std=float("%.3e" % y.std()), exact_var_median=float("%.3e" % np.median(want[:, 1])), bad=bad)), flush=True)


def main():
    reps, limit = option("--reps", 7), option("--limit", 240)
    if "--shape" in sys.argv:
        a = sys.argv[sys.argv.index("--shape") + 1:]
        if a[0] == "knn":
            return knn_shape(int(a[1]), int(a[2]), int(a[3]), reps)
        if a[0] == "predict":
            return predict_shape(int(a[1]), int(a[2]), reps)
        return exact_shape(int(a[1]), reps)
    out_path = option("--out", os.path.join(ROOT, "profiles", "local_bench.txt"), str)
    shapes = [("knn",) + s for s in KNN_SHAPES] + [("predict",) + s for s in PREDICT_SHAPES] + [("exact", d) for d in EXACT_DIMS]
    for shape in shapes:
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(reps), "--shape"] + [str(v) for v in shape]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"{shape}: no result after {limit} s; nothing more is started")
        if r.returncode != 0:
            sys.exit(f"{shape}: the step ended with status {r.returncode}; nothing more is started")
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        with open(out_path, "a") as f:
            f.write(r.stdout)


if __name__ == "__main__":
    main()
