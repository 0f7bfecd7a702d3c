"""The real multi-rank HIP path on ONE GPU: two (and three) ranks share cuda:0 and exchange panels through
torch.distributed's gloo backend (RCCL needs one device per rank; the 8-GPU RCCL run is the driver's).  This
exercises what the CPU gloo test cannot: native kernels on the two streams, the look-ahead event ordering and
the broadcast of packed panels between device buffers."""
import os
import socket
import sys

import numpy as np
import pytest

from conftest import ROOT, TOL, nerr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _problem(n, d, ns, seed=21):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (n, d))
    y = 0.1 * (X ** 3).sum(1) + rng.normal(0, 0.1, n)
    Xs = rng.uniform(-1, 1, (ns, d))
    return X, y, Xs


def _worker(rank, world, port, n, d, ns, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    import gprc_amd  # noqa: F401
    from gprc_amd import _native as nat
    from gprc_amd.distributed import DistributedGPR, HipOps, TorchComm
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        X, y, Xs = _problem(n, d, ns)
        ops = HipOps(0, nat.SQREXP, [1.0], d, n, 0.1)
        comm = TorchComm()
        eng = DistributedGPR(ops, comm)          # world > 1 -> look-ahead on
        g = ops.geom
        ypad = np.zeros(g.n_pad)
        ypad[:n] = y
        Xd, yd = ops.from_host(X), ops.from_host(ypad)
        lo, hi = eng.slice_bounds(ns, world)[rank]
        Xsd = ops.from_host(Xs[lo:hi] if hi > lo else np.zeros((1, d)))
        mean, var = ops.zeros(max(hi - lo, 1)), ops.zeros(max(hi - lo, 1))
        for _ in range(2):                        # twice: buffers and streams are reused across steps
            info = eng.fit(Xd, yd)
            eng.predict_local(Xd, yd, Xsd, hi - lo, mean, var)
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), info=info, alpha=ops.to_host(eng.alpha)[:n],
                 packed=ops.to_host(eng.packed), logp=float(ops.to_host(eng.scal)[0]), lo=lo, hi=hi,
                 mean=ops.to_host(mean)[: hi - lo], var=ops.to_host(var)[: hi - lo])
        ops.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n", [(2, 2300), (3, 1800)])
def test_two_ranks_one_gpu_gloo(tmp_path, world, n):
    import torch.multiprocessing as mp
    from gprc_amd import GPR, cov_func, sqrexp
    d, ns = 4, 301
    try:
        mp.spawn(_worker, args=(world, _free_port(), n, d, ns, str(tmp_path)), nprocs=world, join=True)
    except Exception as e:  # gloo without device-tensor support on this build: not a product failure
        if "gloo" in str(e).lower() and ("cuda" in str(e).lower() or "device" in str(e).lower()):
            pytest.skip(f"gloo cannot move device tensors here: {e}")
        raise
    X, y, Xs = _problem(n, d, ns)
    g = GPR(X.T, y, 0.1, cov_func(sqrexp, l=1.0))   # single-GPU host path
    ref = g.predict(Xs.T)
    outs = [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(world)]
    for o in outs:
        assert int(o["info"]) == 0
        assert np.array_equal(o["alpha"], g.alpha)              # same arithmetic, same order: bitwise
        assert abs(float(o["logp"]) - g.logp) <= 1e-12 * abs(g.logp)
        lo, hi = int(o["lo"]), int(o["hi"])
        assert np.array_equal(o["mean"], ref[lo:hi, 0]) and np.array_equal(o["var"], ref[lo:hi, 1])
    for o in outs[1:]:
        assert np.array_equal(o["packed"], outs[0]["packed"])   # the factor is replicated on every rank


def test_bench_gpus2_spawns_its_own_ranks(tmp_path, orc):
    """`python bench.py --gpus 2` with no launcher: the parent (which never touches the GPU) starts two rank processes
    and relays rank 0's JSON line.  GPRC_BENCH_BACKEND=gloo lets both ranks share cuda:0 on a one-GPU box (RCCL wants a
    device per rank; the 2/4/8-device RCCL runs are the driver's).  The line must be an N = 2 line, carry the panel
    exchange record, per-rank phases and the parity of the timed outputs."""
    import json
    import subprocess
    env = dict(os.environ, GPRC_BENCH_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--workload", "c2",
                        "--ntrain", "2300", "--nstar", "1100", "--no-cpu-baseline", "--full", "--dump-outputs", str(tmp_path)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["backend"] == "gloo" and out["scaling"] == "strong"
    assert out["panel_broadcast"]["choice"] in ("broadcast", "scatter_allgather")
    assert [p["rank"] for p in out["phases_ms"]["per_rank"]] == [0, 1]
    assert out["parity_timed_config"]["ok"] and out["parity_timed_config_normwise_err"] <= TOL
    assert out["parity_gate_normwise_err"] <= TOL and out["value"] > 0
    import bench                                                  # --dump-outputs: both ranks' slices of the test points, in order
    X, y, Xs = bench.synth(2300, 8, 1100)
    ref = orc.gpr_fit(orc.SQREXP, [1.0], X.T, y, 0.1)
    mref, vref = orc.gpr_predict(orc.SQREXP, [1.0], X.T, ref["L"], ref["alpha"], Xs.T)
    mean, var = np.load(tmp_path / "mean.npy"), np.load(tmp_path / "var.npy")
    assert mean.shape == (1100,) and nerr(mean, mref) <= TOL and nerr(var, vref) <= TOL
    assert nerr(np.load(tmp_path / "alpha.npy"), ref["alpha"]) <= TOL


def test_bench_c1_workload_has_a_line():
    """BASELINE.json configs[0] (n = 256, d = 1, sqexp, n* = 10000 grid: the reference's own CPU-runnable case) through bench.py:
    the plumbing configuration has a line, with the parity of its timed outputs."""
    import json
    import subprocess
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c1", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline",
                        "--no-abi-host-path"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert out["config"]["n"] == 256 and out["config"]["d"] == 1 and out["config"]["n_star"] == 10000
    assert out["parity_timed_config"]["ok"] and out["parity_timed_config_normwise_err"] <= TOL and out["parity_gate_normwise_err"] <= TOL


def test_bench_plain_run_dumps_the_last_timed_step(tmp_path, orc):
    """A plain `bench.py` run (no --full) prints the headline line without the checks of --full, and --dump-outputs writes
    what its last timed step computed -- mean, var, alpha, logp and the factor (diagonal + the whole lower triangle at
    n = 256) -- in float64; every array agrees with the CPU oracle on the same synthetic inputs."""
    import json
    import subprocess
    import bench
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0 and out["dtype"] == "f64" and out["unit"] == "TFLOP/s"
    assert not {"roofline", "kernels", "parity_timed_config", "cpu_baseline", "abi_host_path"} & set(out)
    got = {k: np.load(tmp_path / f"{k}.npy") for k in ("mean", "var", "alpha", "logp", "L_diag", "L_sample")}
    assert all(a.dtype == np.float64 for a in got.values())
    X, y, Xs = bench.synth(256, 1, None)
    ref = orc.gpr_fit(orc.SQREXP, [1.0], X.T, y, 0.1)
    mref, vref = orc.gpr_predict(orc.SQREXP, [1.0], X.T, ref["L"], ref["alpha"], Xs.T)
    assert got["mean"].shape == (10000,) and nerr(got["mean"], mref) <= TOL and nerr(got["var"], vref) <= TOL
    assert nerr(got["alpha"], ref["alpha"]) <= TOL and nerr(got["logp"], [ref["logp"]]) <= TOL
    assert nerr(got["L_diag"], np.diag(ref["L"])) <= TOL and nerr(got["L_sample"], ref["L"][np.tril_indices(256)]) <= TOL


def test_bench_gpus4_gloo_rehearsal_n16384():
    """The torch.distributed driver at a panel count where every rank owns eight panels (n = 16384: 32 panels on 4 ranks sharing
    cuda:0 over gloo): quarter-panel pipelined broadcast, look-ahead, batched far updates, the forward solve inside the sweep,
    calibrate().  Four ranks, not eight: a GPU box admits six processes on its card (pytest itself is one); the 8-owner
    protocol runs with virtual ranks (test_config4_eight_rank_protocol_with_virtual_ranks) and on CPU over gloo."""
    import json
    import subprocess
    env = dict(os.environ, GPRC_BENCH_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "1", "--warmup", "1", "--workload", "c2",
                        "--ntrain", "16384", "--nstar", "8192", "--full", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert out["n_gpus"] == 4 and out["config"]["n"] == 16384 and [p["rank"] for p in out["phases_ms"]["per_rank"]] == [0, 1, 2, 3]
    assert out["parity_timed_config"]["ok"] and out["parity_timed_config_normwise_err"] <= TOL


@pytest.mark.parametrize("devices,rccl", [([0, 0], False), ([0, 0, 0], False), ([0], True)])
def test_gpr_over_virtual_ranks_from_one_process(devices, rccl):
    """GPR(..., devices=[...]): the reference's GPR$new / $predict over several ranks driven by THIS process through
    gprc_mgpu_* (what the R binding's options(gprc.devices=) selects).  Virtual ranks share cuda:0; the RCCL exchange is
    exercised with the one rank a one-GPU box allows.  Bitwise equal to the single-GPU object, including the full
    posterior covariance and $L served by rank 0's replica."""
    from gprc_amd import GPR, cov_func, rationalquadratic
    X, y, Xs = _problem(2300, 4, 301)
    k = cov_func(rationalquadratic, l=0.9, alpha=1.5)
    ref = GPR(X.T, y, 0.1, k)
    g = GPR(X.T, y, 0.1, k, devices=devices, rccl=rccl)
    assert np.array_equal(g.alpha, ref.alpha) and g.logp == ref.logp and g.noise == ref.noise
    assert np.array_equal(g.predict(Xs.T), ref.predict(Xs.T))
    m1, c1 = g.predict(Xs.T[:, :40], pointwise_var=False)
    m0, c0 = ref.predict(Xs.T[:, :40], pointwise_var=False)
    assert np.array_equal(m1, m0) and np.array_equal(c1, c0)
    assert np.array_equal(g.L, ref.L)
    g.close()
    ref.close()
