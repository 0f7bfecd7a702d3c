#!/usr/bin/env python3
"""bench.py -- the GP predict step (fit + predict) on N MI355X GPUs of one node.

  python bench.py --gpus N --steps K --warmup W
      N = 1 runs in this process.  N > 1 without a launcher: this process (which never touches the GPU) starts
      `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...` as a CHILD, one
      rank per GPU over RCCL, and relays rank 0's JSON line.
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W          (the driver's own launch: used as is)

One "step" = one pass of the hot path over one synthetic problem: kernel fill of K + noise*I, blocked
fp64 Cholesky, alpha and logp (the reference's GPR$new, R/GPRclass.R:127-154) followed by the pointwise
GPR$predict (R/GPRclass.R:155-165) on the reference's own test grid (R/simulation.R:101-102).  Inputs are
resident in HBM when the timed region starts.  Default workload: BASELINE.json configs[3] (C4), n = 65536,
d = 8, sqexp, n* = 4^8 = 65536 -- the configuration the metric's target is quoted on; it fits one GPU and
is the same at every N (strong scaling).  `--workload c2|c3` select the other single-GPU configs.

Prints ONE JSON line on rank 0: `metric`, `value` (TFLOP/s of the timed steps), `unit`, `ms_per_step`,
`higher_is_better`, `dtype`, the configuration and the per-phase split of the timed steps.  A plain run does only
that: set up, warm up, time the --steps steps, write the outputs (--dump-outputs) and print the line.

--full adds the checks and side measurements, each of which costs runs of its own: a parity gate against the
oracle before timing, `kernels` / `roofline` (dominant kernel, HIP events recorded inside the native library on
the launching stream during the timed steps), `parity_timed_config_normwise_err` (the outputs of the LAST TIMED
step against an independent small-batch predict, the K alpha = y - noise alpha identity and -- mean AND variance --
a vendor-LAPACK fp64 reference that shares nothing with the library; the run FAILS above 1e-10) and, at N = 1,
`cpu_baseline` (three CPU lines on a bounded sample) and `abi_host_path` (the drop-in boundary as R's `.Call` would
use it: gprc_gpr_fit_retry + gprc_gpr_predict with HOST pointers on the timed workload, one cold call -- first-call
device allocations included -- and one warm call).  The --no-* switches leave out single legs of --full.

--dump-outputs DIR writes what the LAST TIMED step computed, as a caller of GPR$new + GPR$predict receives it, to
DIR/<name>.npy in float64: mean, var (all n* test points, every rank's slice), alpha, logp, L_diag (the diagonal
of the factor) and L_sample (entries L[i, j], i >= j, of the factor: the whole lower triangle when it is small,
else pairs drawn from a fixed seed).  An array longer than DUMP_MAX is replaced by a fixed, seeded sample of its
entries, which holds the dump under 64 MB.  The inputs depend only on the arguments, so two builds run with the
same arguments can be compared output for output.

GPRC_BENCH_BACKEND=gloo: ranks exchange through gloo and share cuda:(LOCAL_RANK mod device count) -- how
`pytest -m gpu` rehearses `--gpus 2` on a one-GPU box.  Default backend: nccl (= RCCL over xGMI).
"""
import argparse
import json
import math
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP64_MFMA_PEAK_TFLOPS = 78.6   # MI355X spec, fp64 matrix (dense); measured 77.5 by tools/microbench/mfma_f64.hip
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8 TB/s spec
PARITY_FAIL = 1e-10            # the north star's tolerance: the run fails when the timed outputs are further than this from
                               # the independent values (observed: 0.0 bitwise / 2e-13 / 1e-13)

WORKLOADS = {
    # name: (n, d, kernel name, params, n_star or None -> reference grid rule)
    "c1": (256, 1, "sqrexp", [1.0], None),
    "c2": (8192, 8, "sqrexp", [1.0], None),
    "c3": (32768, 8, "rationalquadratic", [1.0, 1.5], None),
    "c4": (65536, 8, "sqrexp", [1.0], None),
}
KERNEL_IDS = {"constant": 0, "linear": 1, "polynomial": 2, "sqrexp": 3, "gammaexp": 4, "rationalquadratic": 5}
SEED = 20261004
DUMP_MAX = 1 << 20             # doubles per dumped array (8 MB): five arrays + logp stay under 64 MB


def synth(n, d, n_star):
    """BASELINE.md inputs: X ~ U[-1,1]^(d x n), y = 0.1*sum(x^3) + N(0, 0.1^2); test grid = combine_all of
    ceil(10000^(1/d)) equispaced points per axis (R/simulation.R:101-102, 338-349), first axis slowest."""
    rng = np.random.Generator(np.random.Philox(SEED))
    X = rng.uniform(-1.0, 1.0, size=(n, d))                      # row i = point i  (== d x n column-major)
    y = 0.1 * (X ** 3).sum(1) + rng.normal(0.0, 0.1, size=n)
    if n_star is None:
        per = math.ceil(10000 ** (1.0 / d))   # R: seq(length.out = x) applies a bare ceiling()
        axes = [np.linspace(-1.0, 1.0, per)] * d
        Xs = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, d)
    else:
        Xs = rng.uniform(-1.0, 1.0, size=(n_star, d))
    return np.ascontiguousarray(X), y, np.ascontiguousarray(Xs)


def step_flops(n, ns):
    """end-to-end algorithmic flops of one predict step."""
    return n ** 3 / 3.0 + float(n) * n * ns + 2.0 * n * n + 4.0 * n * ns


# ---- CPU column ------------------------------------------------------------------------------------------------------
def usable_cpus():
    """(os.cpu_count() uncapped, CPUs this process may actually use: affinity mask and cgroup quota)."""
    host = os.cpu_count() or 1
    use = host
    try:
        use = min(use, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            use = min(use, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return host, max(1, use)


def cpu_baseline(kname, params, d, budget_1t_s=18.0):
    """Three CPU lines on the SAME inputs and the same n (= n*), the largest power of two whose 1-thread run fits the
    budget: the oracle's blocked port with all usable cores and with 1 thread (R's default BLAS/LAPACK is single
    threaded), and LAPACK dpotrf + dtrtrs through scipy/OpenBLAS when importable."""
    from oracle import oracle as orc
    host, cores = usable_cpus()
    kid = KERNEL_IDS[kname]

    def run_port(threads, n, ns):
        orc.set_threads(threads)
        X, y, Xs = synth(n, d, ns)
        t0 = time.perf_counter()
        r = orc.gpr_fit_predict_blocked(kid, params, X.T, y, 0.1, Xs.T)
        dt = time.perf_counter() - t0
        assert r["info"] == 0
        return dt, r

    t_cal, _ = run_port(1, 1024, 1024)
    rate1 = step_flops(1024, 1024) / t_cal
    n = 1024
    while n < 8192 and step_flops(2 * n, 2 * n) / rate1 < budget_1t_s:
        n *= 2
    fl = step_flops(n, n)
    lines = []
    dt_all, r_all = run_port(cores, n, n)
    lines.append({"name": "oracle_port_all_cores", "kind": "port", "threads": cores, "seconds": round(dt_all, 3),
                  "value": round(fl / dt_all * 1e-12, 5), "unit": "TFLOP/s"})
    dt_1, _ = run_port(1, n, n) if n > 1024 else (t_cal, None)
    lines.append({"name": "oracle_port_1_thread", "kind": "port", "threads": 1, "seconds": round(dt_1, 3),
                  "value": round(fl / dt_1 * 1e-12, 5), "unit": "TFLOP/s"})
    orc.set_threads(cores)
    try:   # LAPACK sanity line: numpy kernel fill (direct (x-y)^2 sums) + dpotrf + dpotrs + dtrtrs
        import scipy.linalg as sl
        X, y, Xs = synth(n, d, n)

        def kern(A, B):
            D = np.zeros((A.shape[0], B.shape[0]))
            for r in range(d):
                D += (A[:, r, None] - B[None, :, r]) ** 2
            return np.exp(-D / (2 * params[0] ** 2)) if kname == "sqrexp" else (1 + D / (2 * params[1] * params[0] ** 2)) ** (-params[1])

        def lapack_step():
            t0 = time.perf_counter()
            K = kern(X, X)
            K[np.diag_indices(n)] += 0.1
            L = sl.cholesky(K, lower=True, overwrite_a=True, check_finite=False)
            alpha = sl.cho_solve((L, True), y, check_finite=False)
            Ks = kern(X, Xs)
            mean = Ks.T @ alpha
            v = sl.solve_triangular(L, Ks, lower=True, overwrite_b=True, check_finite=False)
            var = 1.0 - np.einsum("ij,ij->j", v, v)
            return time.perf_counter() - t0, mean, var

        try:   # OpenBLAS sizes its pool from the HOST's core count (256 on the GPU node); hold it to what this job may use
            from threadpoolctl import threadpool_limits
            from threadpoolctl import threadpool_info
            with threadpool_limits(limits=cores, user_api="blas"):
                blas_threads = max([p_.get("num_threads", 1) for p_ in threadpool_info() if p_.get("user_api") == "blas"] or [1])
                dt_s, mean, var = lapack_step()
        except ImportError:
            blas_threads = None
            dt_s, mean, var = lapack_step()
        err = max(float(np.abs(mean - r_all["mean"]).max() / np.abs(r_all["mean"]).max()),
                  float(np.abs(var - r_all["var"]).max() / np.abs(r_all["var"]).max()))
        lines.append({"name": "scipy_openblas_dpotrf_dtrtrs", "kind": "lapack", "threads": blas_threads, "seconds": round(dt_s, 3),
                      "value": round(fl / dt_s * 1e-12, 5), "unit": "TFLOP/s", "normwise_diff_vs_port": err})
    except ImportError:
        pass
    # best of the three: all are CPU restatements of the reference algorithm ("port"); the LAPACK line is the closest to
    # what R itself executes (chol() = dpotrf), with a triangular solve where R runs dgesv
    best = max(lines, key=lambda ln: ln["value"])
    return {"value": best["value"], "unit": "TFLOP/s", "cores": best["threads"] or cores, "kind": "port",
            "host_cpu_count": host, "usable_cpus": cores,
            "sample": f"fit + pointwise predict on n={n}, n*={n}, d={d}, {kname} (same synthetic inputs for every line); best line: {best['name']} ({best['seconds']} s)",
            "lines": lines}


def parity_gate(eng_factory, comm):
    """Small fit+predict through the same engine against the oracle (normwise 1e-10) before timing."""
    from oracle import oracle as orc
    n, d, ns = 1536, 8, 512
    X, y, Xs = synth(n, d, ns)
    eng, ops, bufs = eng_factory(n, d, "sqrexp", [1.0], X, y, Xs)
    info = eng.fit(bufs["X"], bufs["y"])
    assert info == 0
    lo, hi = eng.slice_bounds(ns, comm.world)[comm.rank]
    eng.predict_local(bufs["X"], bufs["y"], bufs["Xs_local"], hi - lo, bufs["mean"], bufs["var"])
    mean = ops.to_host(bufs["mean"])[: hi - lo]
    var = ops.to_host(bufs["var"])[: hi - lo]
    ref = orc.gpr_fit(orc.SQREXP, [1.0], X.T, y, 0.1)
    mr, vr = orc.gpr_predict(orc.SQREXP, [1.0], X.T, ref["L"], ref["alpha"], Xs.T)
    e1 = np.abs(mean - mr[lo:hi]).max() / np.abs(mr).max() if hi > lo else 0.0
    e2 = np.abs(var - vr[lo:hi]).max() / np.abs(vr).max() if hi > lo else 0.0
    ops.close()
    assert e1 <= 1e-10 and e2 <= 1e-10, (e1, e2)
    return max(e1, e2)


def timed_config_parity(eng, ops, bufs, X, y, Xs, lo, hi, mean, var, noise=0.1, rows=512):
    """Independent values for the outputs of the LAST TIMED step (this rank's slice [lo, hi) of the grid):
      (a) `rows` strided rows predicted again in a separate small batch -- M = rows instead of M = hi - lo, so a
          different panel-group schedule of the solve (bit-identical by construction, compared normwise AND bitwise);
      (b) the size-independent identity K alpha = y - noise alpha read off a small-batch predict at `rows` TRAINING
          inputs (first, middle and last panels), which involves every panel of the timed factor, both triangular
          solves, the K*^T fill and the mean reduction, plus 0 < var < noise there.
    (a) ties the big-batch outputs to the small-batch path, (b) ties that path to the mathematics."""
    n = X.shape[0]
    m = hi - lo
    out = {"rows": 0, "bitwise_equal": True, "normwise_err": 0.0, "identity_err": 0.0, "var_bounds_ok": True}
    if m > 0:
        idx = np.unique(np.linspace(0, m - 1, min(rows, m)).astype(np.int64))
        sub = ops.from_host(Xs[lo:hi][idx])
        ms, vs = ops.zeros(idx.size), ops.zeros(idx.size)
        eng.predict_local(bufs["X"], bufs["y"], sub, idx.size, ms, vs)
        ms, vs = ops.to_host(ms), ops.to_host(vs)
        e = max(float(np.abs(mean[idx] - ms).max() / max(np.abs(ms).max(), 1e-300)),
                float(np.abs(var[idx] - vs).max() / max(np.abs(vs).max(), 1e-300)))
        out.update(rows=int(idx.size), normwise_err=e,
                   bitwise_equal=bool(np.array_equal(mean[idx], ms) and np.array_equal(var[idx], vs)))
    third = max(rows // 3, 1)
    tidx = np.unique(np.r_[0:min(third, n), max(n // 2 - third // 2, 0):min(n // 2 + third // 2, n), max(n - third, 0):n])
    sub = ops.from_host(X[tidx])
    mt, vt = ops.zeros(tidx.size), ops.zeros(tidx.size)
    eng.predict_local(bufs["X"], bufs["y"], sub, tidx.size, mt, vt)
    mt, vt = ops.to_host(mt), ops.to_host(vt)
    alpha = ops.to_host(eng.alpha)[:n]
    want = (y - noise * alpha)[tidx]
    out["identity_err"] = float(np.abs(mt - want).max() / max(np.abs(want).max(), 1e-300))
    out["var_bounds_ok"] = bool((vt > 0).all() and (vt < noise).all())
    return out


def vendor_parity(kname, X, y, Xs, lo, hi, mean, var, alpha, device, noise=0.1, rows=256):
    """The leg that is independent of the library, for mean AND variance: `rows` strided rows of this rank's slice of the
    LAST TIMED step's outputs against the predict step rebuilt from vendor LAPACK / BLAS on the same GPU
    (tools/vendor_reference.py: rocSOLVER potrf, rocBLAS trsm / gemm through torch.linalg; K in slabs with direct
    sum (x - y)^2).  Only the workloads' own kernels (sqrexp l = 1, rationalquadratic l = 1 alpha = 1.5)."""
    from tools.vendor_reference import lapack_reference_subset
    m = hi - lo
    if m <= 0 or kname not in ("sqrexp", "rationalquadratic"):
        return None
    idx = np.unique(np.linspace(0, m - 1, min(rows, m)).astype(np.int64))
    t0 = time.perf_counter()
    a_ref, m_ref, v_ref = lapack_reference_subset(kname, X.T, y, np.ascontiguousarray(Xs[lo:hi][idx].T), noise, device=device)
    nrm = lambda got, ref: float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))
    return {"rows": int(idx.size), "alpha_err": nrm(alpha, a_ref), "mean_err": nrm(mean[idx], m_ref), "var_err": nrm(var[idx], v_ref),
            "seconds": round(time.perf_counter() - t0, 2)}


def abi_host_path(device, kname, params, X, y, Xs, resident_ms):
    """The drop-in boundary as the reference's host would drive it (`.Call` hands REAL(x) pointers):
    gprc_gpr_fit_retry + gprc_gpr_predict with HOST arrays on the timed workload, on a fresh context.  Cold = the first
    call on that context (device allocations of the model -- 17 GB at C4 -- and of the predict chunk, H2D of X, y, X*,
    D2H of alpha / mean / var); warm = the same call again (blocks come back from the context's free-list)."""
    import ctypes as C
    from gprc_amd import _native as nat
    L = nat.lib()
    ctx = nat.Context(device, None)
    Xc, yc, Xsc = np.ascontiguousarray(X), np.ascontiguousarray(y), np.ascontiguousarray(Xs)   # row i = point i == d x n column-major
    n, d = Xc.shape
    ns = Xsc.shape[0]
    _, pp, npar = nat.params_array(params)
    mean, var = np.empty(ns), np.empty(ns)
    rec = {}
    try:
        for name in ("cold", "warm"):
            model, nu, att = C.c_void_p(), C.c_double(), C.c_int()
            t0 = time.perf_counter()
            nat.check(L.gprc_gpr_fit_retry(ctx.handle, KERNEL_IDS[kname], pp, npar, Xc.ctypes.data, d, n, yc.ctypes.data, 0.1, C.byref(model),
                                           C.byref(nu), C.byref(att)))
            t1 = time.perf_counter()
            nat.check(L.gprc_gpr_predict(model, Xsc.ctypes.data, ns, 1, mean.ctypes.data, var.ctypes.data))
            t2 = time.perf_counter()
            L.gprc_model_free(model)
            rec[name] = {"fit_ms": round((t1 - t0) * 1e3, 2), "predict_ms": round((t2 - t1) * 1e3, 2), "step_ms": round((t2 - t0) * 1e3, 2)}
    finally:
        ctx.close()
    rec["resident_step_ms"] = round(resident_ms, 2)
    rec["warm_minus_resident_ms"] = round(rec["warm"]["step_ms"] - resident_ms, 2)
    rec["cold_minus_resident_ms"] = round(rec["cold"]["step_ms"] - resident_ms, 2)
    rec["what"] = "gprc_gpr_fit_retry + gprc_gpr_predict(pointwise) with host pointers, fresh context; cold = first call (allocations included)"
    return rec, mean, var


# ---- --dump-outputs --------------------------------------------------------------------------------------------------
def factor_offsets(geom, n):
    """Offsets in the packed buffer of L_diag (L[j, j], j < n) and of L_sample (L[i, j], i >= j: the whole lower triangle
    in row-major order when it has at most DUMP_MAX entries, else DUMP_MAX pairs drawn from a fixed seed).  Panel p holds
    rows [p NB, n_pad) x columns [p NB, (p+1) NB), column-major with leading dimension n_pad - p NB (include/gprc_native.h),
    so every offset lies inside panel j // NB for i < n <= n_pad."""
    base = np.asarray(geom.offsets, dtype=np.int64)

    def offsets(i, j):
        p = j // geom.NB
        return base[p] + (j - p * geom.NB) * (geom.n_pad - p * geom.NB) + (i - p * geom.NB)

    diag = np.arange(n, dtype=np.int64)
    if n * (n + 1) // 2 <= DUMP_MAX:
        i, j = np.tril_indices(n)
    else:
        rng = np.random.Generator(np.random.Philox(SEED + 1))
        a, b = rng.integers(0, n, DUMP_MAX), rng.integers(0, n, DUMP_MAX)
        i, j = np.maximum(a, b), np.minimum(a, b)
    return offsets(diag, diag), offsets(i.astype(np.int64), j.astype(np.int64))


def write_outputs(path, arrays):
    """DIR/<name>.npy in float64; an array longer than DUMP_MAX is cut to DUMP_MAX entries at ascending indices drawn
    from a fixed seed (the same for every build)."""
    os.makedirs(path, exist_ok=True)
    for k, (name, a) in enumerate(arrays.items()):
        a = np.ascontiguousarray(a, dtype=np.float64).ravel()
        if a.size > DUMP_MAX:
            rng = np.random.Generator(np.random.Philox(SEED + 2 + k))
            a = a[np.sort(rng.choice(a.size, DUMP_MAX, replace=False))]
        np.save(os.path.join(path, name + ".npy"), a)


# ---- launching -------------------------------------------------------------------------------------------------------
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def spawn_ranks(args, argv):
    """--gpus N > 1 without a launcher: start the N ranks as fresh child processes.  THIS process has made no HIP call
    (torch is not even imported), and nothing is exec'd: the launcher is a child whose exit code we return."""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.abspath(__file__)] + argv
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in proc.stdout.splitlines():
        if ln.startswith("{") and '"metric"' in ln:
            line = ln
        else:
            print(ln, file=sys.stderr)
    if line is not None:
        print(line, flush=True)
    if proc.returncode != 0 or line is None:
        raise SystemExit(proc.returncode or 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="c4", choices=sorted(WORKLOADS))
    ap.add_argument("--ntrain", type=int, default=0, help="override n (not --n: ambiguous for torch.distributed.run)")
    ap.add_argument("--nstar", type=int, default=0, help="override n* (random test points instead of the grid)")
    ap.add_argument("--full", action="store_true", help="also the parity checks, per-kernel / roofline figures, the host-pointer "
                    "timing and the CPU baseline (off: set up, warm up, time the steps, dump, print the line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's outputs to DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-parity-gate", action="store_true", help="--full without the parity gate before timing")
    ap.add_argument("--no-abi-host-path", action="store_true", help="--full without the host-pointer (.Call-shaped) cold/warm timing at N = 1")
    ap.add_argument("--no-vendor-parity", action="store_true", help="--full without the vendor-LAPACK leg of the timed-output parity check")
    args = ap.parse_args()
    if args.gpus < 1 or args.steps < 1 or args.warmup < 0:
        raise SystemExit("bench.py: --gpus >= 1, --steps >= 1, --warmup >= 0")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return spawn_ranks(args, sys.argv[1:])       # before `import torch`: the parent never initialises the GPU
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: refusing to report a line for a different N")

    import torch
    import gprc_amd  # noqa: F401
    from gprc_amd import _native as nat
    from gprc_amd.distributed import DistributedGPR, HipOps, SingleComm, TorchComm

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the gprc native path has no CPU fallback")
    backend = os.environ.get("GPRC_BENCH_BACKEND", "nccl")
    if backend not in ("nccl", "gloo"):
        raise SystemExit("GPRC_BENCH_BACKEND must be nccl or gloo")
    ndev = torch.cuda.device_count()
    if backend == "nccl" and world > ndev:
        raise SystemExit(f"bench.py: {world} RCCL ranks need {world} GPUs, {ndev} visible (GPRC_BENCH_BACKEND=gloo shares one)")
    device = local_rank % ndev
    torch.cuda.set_device(device)
    use_dist = world > 1 or os.environ.get("GPRC_FORCE_DIST") == "1"   # FORCE_DIST: exercise the RCCL path with one rank
    if use_dist:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", device))
        else:
            dist.init_process_group("gloo")
        comm = TorchComm()
        # panel broadcast: RCCL's rooted broadcast vs scatter + all-gather, timed once on this node (GPRC_BCAST pins it)
        comm.calibrate(lambda c: torch.empty(c, dtype=torch.float64, device="cuda"), torch.cuda.synchronize)
    else:
        comm = SingleComm()

    n, d, kname, params, n_star = WORKLOADS[args.workload]
    if args.ntrain:
        n = args.ntrain
    if args.nstar:
        n_star = args.nstar

    def make_engine(n_, d_, kname_, params_, X, y, Xs):
        ops = HipOps(device, KERNEL_IDS[kname_], params_, d_, n_, 0.1)
        eng = DistributedGPR(ops, comm)
        g = ops.geom
        ypad = np.zeros(g.n_pad)
        ypad[:n_] = y
        ns_ = Xs.shape[0]
        lo, hi = eng.slice_bounds(ns_, comm.world)[comm.rank]
        width = max(hi - lo, 1)
        bufs = {"X": ops.from_host(X), "y": ops.from_host(ypad),
                "Xs_local": ops.from_host(Xs[lo:hi] if hi > lo else np.zeros((1, d_))),
                "mean": ops.zeros(width), "var": ops.zeros(width)}
        ops.synchronize()
        return eng, ops, bufs

    gate_err = None
    if args.full and not args.no_parity_gate:
        gate_err = parity_gate(make_engine, comm)

    X, y, Xs = synth(n, d, n_star)
    ns = Xs.shape[0]
    eng, ops, bufs = make_engine(n, d, kname, params, X, y, Xs)
    lo, hi = eng.slice_bounds(ns, world)[rank]

    marks = []   # (start, fitted, predicted) events on the library's main stream: phase split F1-F3 / P1-P3

    def mark():
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(ops.main_stream)
        return ev

    def step():
        e0 = mark()
        info = eng.fit(bufs["X"], bufs["y"])
        if info != 0:
            raise RuntimeError(f"K + noise*I not positive definite (info={info})")
        e1 = mark()
        eng.predict_local(bufs["X"], bufs["y"], bufs["Xs_local"], hi - lo, bufs["mean"], bufs["var"])
        marks.append((e0, e1, mark()))

    def fence():
        ops.synchronize()
        comm.barrier()
        torch.cuda.synchronize()

    def all_max(values):
        if not use_dist:
            return values
        t = torch.tensor(values, dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        return [float(v) for v in t.cpu()]

    def all_gather_rows(values):
        """values (a short list of floats) of every rank -> [[rank 0's], [rank 1's], ...]"""
        if not use_dist:
            return [list(values)]
        t = torch.tensor(values, dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        outs = [torch.empty_like(t) for _ in range(world)]
        torch.distributed.all_gather(outs, t)
        return [[float(v) for v in o.cpu()] for o in outs]

    def all_gather_concat(a):
        """this rank's slice of the test points -> all n* of them, in order (every rank takes part)"""
        if not use_dist:
            return a
        t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda" if backend == "nccl" else "cpu")
        return comm.gather_concat(t, [h - l for l, h in eng.slice_bounds(ns, world)]).cpu().numpy()

    for _ in range(args.warmup):
        step()
    if args.full:
        nat.lib().gprc_prof_reset()
        nat.lib().gprc_prof_enable(1 if rank == 0 else 0)
    fence()
    marks.clear()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    elapsed = time.perf_counter() - t0
    if args.full:
        nat.lib().gprc_prof_enable(0)
    elapsed = all_max([elapsed])[0]

    if args.full or args.dump_outputs:
        mean = ops.to_host(bufs["mean"])[: hi - lo]
        var = ops.to_host(bufs["var"])[: hi - lo]
    if args.dump_outputs:   # the last timed step's outputs, before any check runs on the engine
        outputs = {"mean": all_gather_concat(mean), "var": all_gather_concat(var)}
        if rank == 0:
            d_off, s_off = factor_offsets(eng.geom, n)
            idx = ops.from_host(np.concatenate([d_off, s_off]))
            with ops.on(False):
                picked = eng.packed.index_select(0, idx)
            picked = ops.to_host(picked)
            outputs.update(alpha=ops.to_host(eng.alpha)[:n], logp=ops.to_host(eng.scal)[:1], L_diag=picked[:n], L_sample=picked[n:])
            write_outputs(args.dump_outputs, outputs)

    parity_ok = True
    if args.full:
        sane = bool(np.isfinite(mean).all() and np.isfinite(var).all() and (var > -1e-8).all())
        tp = timed_config_parity(eng, ops, bufs, X, y, Xs, lo, hi, mean, var)
        vp = None
        if rank == 0 and not args.no_vendor_parity:   # rank 0's slice against vendor LAPACK: independent of the library, mean AND variance
            vp = vendor_parity(kname, X, y, Xs, lo, hi, mean, var, ops.to_host(eng.alpha)[:n], device)
        vend_err = max(vp["alpha_err"], vp["mean_err"], vp["var_err"]) if vp else 0.0
        par_err, id_err, bad, vend_err = all_max([tp["normwise_err"], tp["identity_err"],
                                                  0.0 if (sane and tp["var_bounds_ok"] and tp["bitwise_equal"]) else 1.0, vend_err])
        parity_ok = bool(par_err <= PARITY_FAIL and id_err <= PARITY_FAIL and vend_err <= PARITY_FAIL and bad == 0.0)

    phases = all_gather_rows([sum(a.elapsed_time(b) for a, b, _ in marks) / len(marks), sum(b.elapsed_time(c) for _, b, c in marks) / len(marks)])

    if rank == 0:
        ms = elapsed / args.steps * 1e3
        flops = step_flops(n, ns)
        out = {
            "metric": "GPR predict-step achieved fp64 TFLOP/s (kernel fill + Cholesky + solves + mean/variance), n x n sqexp",
            "value": round(flops / (elapsed / args.steps) * 1e-12, 4),
            "unit": "TFLOP/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms, 3),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": f"{args.workload}: n={n} d={d} {kname} GPR fit+predict, n*={ns} (reference test-grid rule), noise=0.1",
                       "n": n, "d": d, "n_star": ns, "kernel": kname, "kernel_params": params, "backend": backend if use_dist else None,
                       "parallelism": f"1-D block-cyclic 512-column panels over {world} GPU(s), test points sliced"},
            "phases_ms": {"fit_F1_F3": round(max(p[0] for p in phases), 3), "predict_P1_P3": round(max(p[1] for p in phases), 3),
                          "per_rank": [{"rank": r, "fit_F1_F3": round(p[0], 3), "predict_P1_P3": round(p[1], 3)} for r, p in enumerate(phases)]},
            "panel_broadcast": getattr(comm, "calibration", None) or {"choice": getattr(comm, "choice", None)},
        }
    if rank == 0 and args.full:
        prof = nat.prof_summary()
        kernels = {}
        for name, r in prof.items():
            if r["count"] == 0:
                continue
            kernels[name] = {"launches": r["count"], "ms_total": round(r["ms"], 3), "avg_ms": round(r["ms"] / r["count"], 4),
                             "tflops": round(r["flops"] / r["ms"] * 1e-9, 3) if r["ms"] > 0 else None,
                             "gbs": round(r["bytes"] / r["ms"] * 1e-6, 1) if r["ms"] > 0 else None}
        dom_name = max(("solve_left", "solve_update_k512", "trailing_update", "trailing_left"), key=lambda k: prof[k]["ms"])
        dom = prof[dom_name]
        achieved = dom["flops"] / dom["ms"] * 1e-9 if dom["ms"] > 0 else 0.0
        symbol = {"solve_left": "solve_left_kernel", "solve_update_k512": "gemm_nt_kernel<5>", "trailing_update": "trailing_kernel",
                  "trailing_left": "trailing_range_kernel"}[dom_name]
        # HBM traffic of the dominant kernel: PMC counters cannot be read from inside this process, so the figure
        # comes from the separate rocprofv3 --pmc passes of the same command stored under profiles/ (see the JSON's
        # `source`), per launch and corrected as MI355X_MICROARCH.md prescribes; null when no matching profile.
        traffic, traffic_src = None, None
        for cand in ("r03_c4_pmc_traffic.json", "r02_c4_pmc_traffic.json", "r01_c4_pmc_traffic.json"):
            try:
                pm = json.load(open(os.path.join(ROOT, "profiles", cand)))
                if pm["kernel"] == symbol and pm["workload"] == args.workload and pm["n_gpus"] == world and not args.ntrain and not args.nstar:
                    traffic, traffic_src = pm["traffic_bytes_per_launch"], "profiles/" + cand
                    break
            except (OSError, KeyError, ValueError):
                pass
        out.update({
            "roofline": {"bound": "mfma", "kernel": symbol, "achieved": round(achieved, 3), "peak": FP64_MFMA_PEAK_TFLOPS,
                         "unit": "TFLOP/s", "frac": round(achieved / FP64_MFMA_PEAK_TFLOPS, 4), "traffic": traffic,
                         "traffic_unit": "bytes per launch (PMC, separate pass)", "traffic_source": traffic_src,
                         "algorithmic_bytes_per_launch": round(dom["bytes"] / max(dom["count"], 1)),
                         "launches": dom["count"], "avg_launch_ms": round(dom["ms"] / max(dom["count"], 1), 4)},
            "kernels": kernels,
            "frac_of_fp64_peak_end_to_end": round(flops / (elapsed / args.steps) * 1e-12 / (FP64_MFMA_PEAK_TFLOPS * world), 4),
            "parity_gate_normwise_err": gate_err,
            "parity_timed_config_normwise_err": par_err,
            "parity_timed_config": {"rows_rank0": tp["rows"], "bitwise_equal_to_small_batch": bad == 0.0 or tp["bitwise_equal"],
                                    "identity_K_alpha_normwise_err": id_err, "vendor_lapack": vp, "fail_above": PARITY_FAIL, "ok": parity_ok},
            "outputs_sane": sane,
        })
        if world == 1 and not args.no_abi_host_path and parity_ok:
            # the resident engine's buffers go first: the cold call must find the device as R's first call would
            ops.close()
            del eng, bufs
            torch.cuda.empty_cache()
            rec, hmean, hvar = abi_host_path(device, kname, params, X, y, Xs, ms)
            rec["bitwise_equal_to_resident_path"] = bool(np.array_equal(hmean[lo:hi], mean) and np.array_equal(hvar[lo:hi], var))
            out["abi_host_path"] = rec
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(kname, params, d)
    if rank == 0:
        if parity_ok:
            print(json.dumps(out), flush=True)
        else:   # a fast step with wrong outputs is not a measurement: no JSON line on stdout
            print("bench.py: PARITY FAILURE of the timed configuration: " + json.dumps(out["parity_timed_config"]) +
                  f" normwise_err={par_err}", file=sys.stderr, flush=True)
    if not ops.closed:
        ops.close()
    if use_dist:
        torch.distributed.destroy_process_group()
    if not parity_ok:
        raise SystemExit(3)


if __name__ == "__main__":
    main()
