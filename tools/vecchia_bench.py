"""The Vecchia likelihood of the local GPR (gprc_lgpr_vecchia_prepare, gprc_lgpr_vecchia_logp_grad, fit.optimize_local): what one evaluation
costs beside the route the batched small models offer for the same number, what the predecessor-constrained search costs beside the
unconstrained one, and one optimisation at n = 2^20.  Records, not thresholds.
    python tools/vecchia_bench.py                      # appends JSON lines to profiles/vecchia_bench.txt
    python tools/vecchia_bench.py --out FILE --reps 7
matern52_ard, d = 8, noise 0.1, X uniform in [-2, 2]^d, y = sin(sum x) + 0.1 N(0, 1), l_c = 1 + c / 16, from default_rng(20261021 + the
shape); the columns are in random order as drawn.
  logp      n in {65 536, 2^20}, m in {15, 31, 63}: one gprc_lgpr_vecchia_logp_grad (value and gradient, host outputs) on prepared
            neighbours, beside the old route fed the SAME neighbour indices: per chunk of 16 384 points the neighbours' coordinates and
            targets gathered into strided slabs (a torch index on the device stands in for the library's gather kernel, which has no entry
            point of its own), gprc_gpr_batch_logp_grad on the (m + 1)-point models and again on their first m points, the difference summed.
            The old route runs over the points i >= m (the first m have smaller models); rel_diff is its value against the sum of the new
            route's cond_i over the same points.  speedup = old / new.
  prepare   gprc_lgpr_vecchia_prepare (m = 63) beside gprc_dev_knn of the same n with n* = n, m = 63, device pointers, scaled metric: about
            half the pair work is expected
  optimize  one fit.optimize_local at n = 2^20, m = 31: wall time, evaluations, result
  each time the median of --reps timed repeats after one warm-up of the same shape (three where a repeat takes seconds); min and max beside it.
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
NAME, D, NOISE, SEED = "matern52_ard", 8, 0.1, 20261021
NS = (65536, 1048576)
MS = (15, 31, 63)
OLD_CHUNK = 16384


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


def problem(n, seed):
    import numpy as np
    rng = np.random.default_rng(SEED + seed)
    X = np.asfortranarray(rng.uniform(-2, 2, (D, n)))
    y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
    return X, y, 1.0 + np.arange(D) / 16.0


def create(lib, ctx, kid, ell, X, y, m):
    h = C.c_void_p()
    from gprc_amd import _native as nat
    nat.check(lib.gprc_lgpr_create(ctx.handle, kid, ell.ctypes.data_as(C.POINTER(C.c_double)), D, X.ctypes.data, D, X.shape[1], y.ctypes.data, NOISE,
                                   min(m + 1, 128), C.byref(h)))
    return h


def logp_shape(n, m, reps):
    import numpy as np
    import torch

    import gprc_amd  # noqa: F401
    from gprc_amd import _native as nat
    from gprc_amd.fit import grad_dict

    lib, ctx, kid = nat.lib(), nat.default_context(), grad_dict[NAME].kernel_id
    X, y, ell = problem(n, n % 1000 + m)
    dp = C.POINTER(C.c_double)
    h = create(lib, ctx, kid, ell, X, y, m)
    nat.check(lib.gprc_lgpr_vecchia_prepare(h, m))
    out, g, cond, flagged = C.c_double(), np.empty(D + 1), np.empty(n), C.c_int64()

    def new():
        nat.check(lib.gprc_lgpr_vecchia_logp_grad(h, ell.ctypes.data_as(dp), D, NOISE, C.byref(out), g.ctypes.data, None, C.byref(flagged)))
    new_ms = repeat(new, reps)
    nat.check(lib.gprc_lgpr_vecchia_logp_grad(h, ell.ctypes.data_as(dp), D, NOISE, C.byref(out), g.ctypes.data, cond.ctypes.data, C.byref(flagged)))
    value_ms = repeat(lambda: nat.check(lib.gprc_lgpr_vecchia_logp_grad(h, ell.ctypes.data_as(dp), D, NOISE, C.byref(out), None, None, None)), reps)

    # the old route on the same indices
    idx = torch.empty((n, m), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    nat.check(lib.gprc_lgpr_vecchia_neighbours(h, idx.data_ptr(), m))
    lib.gprc_lgpr_free(h)
    xt, yt = torch.from_numpy(np.ascontiguousarray(X.T)).cuda(), torch.from_numpy(y).cuda()       # n x d, point-major
    B = OLD_CHUNK
    thetas, noises = np.ascontiguousarray(np.tile(ell, (B, 1))), np.full(B, NOISE)
    lp = [np.empty(B), np.empty(B)]
    gr = [np.empty((B, D + 1)), np.empty((B, D + 1))]
    info = np.zeros(B, dtype=np.intc)
    total = [0.0, np.zeros(D + 1)]

    def old():
        value, grad = 0.0, np.zeros(D + 1)
        for i0 in range(m, n, B):
            b = min(B, n - i0)
            pts = torch.cat([idx[i0:i0 + b].long(), torch.arange(i0, i0 + b, device="cuda")[:, None]], dim=1)     # b x (m + 1), the point last
            xg, yg = xt[pts].contiguous(), yt[pts].contiguous()
            torch.cuda.synchronize()
            for k, size in enumerate((m + 1, m)):
                nat.check(lib.gprc_gpr_batch_logp_grad(ctx.handle, kid, b, thetas.ctypes.data, D, D, noises.ctypes.data, xg.data_ptr(), D, size,
                                                       D * (m + 1), yg.data_ptr(), m + 1, None, lp[k].ctypes.data, gr[k].ctypes.data, None,
                                                       info.ctypes.data))
            value += float((lp[0][:b] - lp[1][:b]).sum())
            grad += (gr[0][:b] - gr[1][:b]).sum(0)
        total[0], total[1] = value, grad
    old_ms = repeat(old, min(reps, 3) if n > 100000 else reps)
    want = float(cond[m:].sum())
    med_new, med_old = statistics.median(new_ms), statistics.median(old_ms)
    print(json.dumps(dict(kind="logp", d=D, n=n, m=m, new_ms=stats(new_ms), value_only_ms=stats(value_ms), old_route_ms=stats(old_ms),
                          speedup=round(med_old / med_new, 2), per_point_us=round(1e3 * med_new / n, 4), flagged=int(flagged.value),
                          logp=out.value, rel_diff_old_route=float("%.3e" % (abs(total[0] - want) / abs(want))))), flush=True)


def prepare_shape(n, reps):
    import numpy as np
    import torch

    import gprc_amd  # noqa: F401
    from gprc_amd import _native as nat
    from gprc_amd.fit import grad_dict

    lib, ctx, kid, m = nat.lib(), nat.default_context(), grad_dict[NAME].kernel_id, 63
    X, y, ell = problem(n, n % 1000)
    reps = min(reps, 3) if n > 100000 else reps
    h = create(lib, ctx, kid, ell, X, y, m)
    prep_ms = repeat(lambda: nat.check(lib.gprc_lgpr_vecchia_prepare(h, m)), reps)
    lib.gprc_lgpr_free(h)
    xd = torch.from_numpy(X.ravel(order="F").copy()).cuda()
    idx = torch.empty((n, m), dtype=torch.int32, device="cuda")
    scale = np.ascontiguousarray(1.0 / ell)
    torch.cuda.synchronize()
    knn_ms = repeat(lambda: nat.check(lib.gprc_dev_knn(ctx.handle, xd.data_ptr(), D, n, xd.data_ptr(), n, scale.ctypes.data, m, idx.data_ptr(), None, m)),
                    reps)
    before_ms = repeat(lambda: nat.check(lib.gprc_dev_knn_before(ctx.handle, xd.data_ptr(), D, n, 0, n, scale.ctypes.data, m, idx.data_ptr(), None, m)),
                       reps)
    print(json.dumps(dict(kind="prepare", d=D, n=n, m=m, prepare_ms=stats(prep_ms), knn_before_ms=stats(before_ms), knn_all_ms=stats(knn_ms),
                          ratio=round(statistics.median(before_ms) / statistics.median(knn_ms), 3))), flush=True)


def optimize_shape(n, m):
    import gprc_amd  # noqa: F401
    from gprc_amd.fit import optimize_local

    X, y, ell = problem(n, 31337)
    ms, r = timed(lambda: optimize_local(X, y, NOISE, NAME, m=m, order="given"))
    print(json.dumps(dict(kind="optimize", d=D, n=n, m=m, seconds=round(ms / 1e3, 2), counts=r["counts"], rounds=r["rounds"], convergence=r["convergence"],
                          value=r["value"], par=[float("%.4g" % v) for v in r["par"]], noise=float("%.4g" % r["noise"]),
                          drawn_with=dict(l=[float(v) for v in ell], noise_sd=0.1))), flush=True)


def main():
    reps, limit = option("--reps", 7), option("--limit", 300)
    if "--shape" in sys.argv:
        a = sys.argv[sys.argv.index("--shape") + 1:]
        if a[0] == "logp":
            return logp_shape(int(a[1]), int(a[2]), reps)
        if a[0] == "prepare":
            return prepare_shape(int(a[1]), reps)
        return optimize_shape(int(a[1]), int(a[2]))
    out_path = option("--out", os.path.join(ROOT, "profiles", "vecchia_bench.txt"), str)
    shapes = [("logp", n, m) for n in NS for m in MS] + [("prepare", n) for n in NS] + [("optimize", NS[-1], 31)]
    if "--only" in sys.argv:
        shapes = [s for s in shapes if s[0] == sys.argv[sys.argv.index("--only") + 1]]
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
