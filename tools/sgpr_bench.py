"""Sparse GPR (gprc_sgpr_fit / gprc_sgpr_predict) at sizes no exact entry point reaches, and its one new MFMA kernel against its
yardstick of the same run.  d = 8, noise 0.1, jitter 1e-6, sqrexp_ard (l_k = 1 + k / 16), tools/grad_bench.py's inputs (X ~ U[-1, 1],
y = 0.1 sum(x^3) + N(0, 0.1^2), Philox seed 20261004) resident in device memory; Z = m distinct columns of X.
    python tools/sgpr_bench.py                         # n = 1048576, m = 2048 8192 16384; appends to profiles/sgpr_bench.txt
    python tools/sgpr_bench.py 262144 2048 8192        # n, then the m's named
Per m one JSON line:
  fit_ms          median of 2 gprc_sgpr_fit calls after a warm-up (host clock around the synchronous call); elbo, trace of the fit
  stages_ms       one further fit under the in-library event profiler: fill / solve (the row solve with L_u) / gram (kind 8) / rest
                  (fit_ms of that call less the three: the two factorisations, the column reduction, staging, host sums)
  gram_fit_tflops the Gram launches of that fit: rows m_pad (m_pad + 128) flop per call over their event time; gram_calls, gram_rows
                  (mean rows per call)
  predict_ms      median of 3 gprc_sgpr_predict calls (mean and variance) for 65536 test points after a warm-up
  gram_tflops / nt_tflops   gprc_dev_gram_rows and gprc_dev_gemm_nt (lower = 1) ALONE on one random buffer, M = N = m_pad, K = gram_rows
                  rounded to 256 (alone_K), the same tiles and the same flop count for both, both pitches off the powers of two;
                  median of REPS launches each, timed by the in-library event profiler, and the (min, max) of each: the yardstick is the
                  NT launch of this run, and a gap counts when it exceeds the NT launch's own spread
Gradient mode, the same inputs and sizes:
    python tools/sgpr_bench.py grad                    # appends to profiles/sgpr_grad_bench.txt
    python tools/sgpr_bench.py grad 262144 2048        # n, then the m's named
Per m one JSON line:
  elbo_ms / grad_ms / grad_noz_ms   median of 2 calls after a warm-up of gprc_sgpr_elbo, gprc_sgpr_elbo_grad with dZ and without, of the SAME
                  run; ratio = grad_ms / elbo_ms (the flop count says 2 to 3: written down as an expectation, not a gate)
  contract_ms, contract_gpairs      the contraction launches of one further gprc_sgpr_elbo_grad under the in-library event profiler (kind
                  16, shared with the exact gradient's contraction: nothing else of this call counts there) and the point pairs per
                  nanosecond they weigh -- (n + m_pad) m_pad pairs per coordinate group of 3, ceil(d / 3) groups
  fill_ms, fill_gpairs              the fills of the same call (K_uu's panels and the cross fill of both passes) and their pairs per nanosecond:
                  the contraction's yardstick, one exp per pair on both sides
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
from gprc_amd import _native as nat
from grad_bench import LINV, synth, timed

REPS = 5
N_STAR = 65536


def alone(lib, ctx, m_pad, K):
    """(gram launch times, NT launch times) in ms on one random buffer read both ways: K x m_pad with the rows contiguous (gram), m_pad x K
    with the columns contiguous (NT)"""
    dev = torch.device("cuda:0")
    ldg, lda = K + 16, m_pad + 128                                  # both pitches off the powers of two
    buf = (torch.rand(max(ldg * m_pad, lda * K), dtype=torch.float64, device=dev) - 0.5) * 0.02
    packed = torch.zeros(int(lib.gprc_packed_size(m_pad)), dtype=torch.float64, device=dev)
    dense = torch.zeros(m_pad * m_pad, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()

    def launches(f):
        """event times of REPS single launches after a warm-up, from the in-library profiler (both launchers count under kind 8)"""
        out = []
        lib.gprc_prof_enable(1)
        for it in range(REPS + 1):
            lib.gprc_prof_reset()
            nat.check(f())
            ctx.synchronize()
            if it:
                out.append(nat.prof_summary()["cov_syrk"]["ms"])
        lib.gprc_prof_enable(0)
        return out

    gram = launches(lambda: lib.gprc_dev_gram_rows(ctx.handle, buf.data_ptr(), ldg, K, m_pad, packed.data_ptr()))
    nt = launches(lambda: lib.gprc_dev_gemm_nt(ctx.handle, dense.data_ptr(), m_pad, buf.data_ptr(), lda, buf.data_ptr(), lda, m_pad, m_pad, K, 1))
    return gram, nt


def grad_main(args):
    n = args[0] if args else 1 << 20
    ms = args[1:] or [2048, 8192, 16384]
    lib = nat.lib()
    ctx = nat.Context(0)
    d, noise, jitter = 8, 0.1, 1e-6
    dev = torch.device("cuda:0")
    theta = 1.0 + np.arange(d) / 16.0
    _, pp, npar = nat.params_array(theta)
    Xh, yh = synth(n, d)
    X, y = torch.from_numpy(Xh).to(dev), torch.from_numpy(yh).to(dev)
    torch.cuda.synchronize()
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sgpr_grad_bench.txt")
    for m in ms:
        m_pad = int(lib.gprc_pad(m))
        idx = np.sort(np.random.default_rng(m).choice(n, size=m, replace=False))
        Z = torch.from_numpy(np.ascontiguousarray(Xh[idx])).to(dev)
        dZ = torch.empty((m, d), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        e, g = C.c_double(), np.empty(npar + 1)
        common = (ctx.handle, nat.SQREXP_ARD, pp, npar, X.data_ptr(), d, n, y.data_ptr(), noise, Z.data_ptr(), m, jitter, C.byref(e))

        def elbo():
            nat.check(lib.gprc_sgpr_elbo(*common, None))

        def grad(with_z=True):
            nat.check(lib.gprc_sgpr_elbo_grad(*common, g.ctypes.data, dZ.data_ptr() if with_z else None))

        elbo_ms = statistics.median(timed(elbo, 2))
        grad_ms = statistics.median(timed(grad, 2))
        noz_ms = statistics.median(timed(lambda: grad(False), 2))
        lib.gprc_prof_enable(1)
        lib.gprc_prof_reset()
        grad()
        prof = nat.prof_summary()
        lib.gprc_prof_enable(0)
        groups = -(-d // 3)
        pairs_c, pairs_f = (n + m_pad) * m_pad * groups, (2 * n + m_pad) * m_pad
        c_ms, f_ms = prof["grad_contract"]["ms"], prof["fill"]["ms"]
        rec = dict(mode="grad", n=n, m=m, m_pad=m_pad, d=d, elbo_ms=round(elbo_ms, 2), grad_ms=round(grad_ms, 2), grad_noz_ms=round(noz_ms, 2),
                   ratio=round(grad_ms / elbo_ms, 2), expected_ratio="2 to 3", elbo=e.value, contract_ms=round(c_ms, 2),
                   contract_launches=prof["grad_contract"]["count"], contract_gpairs=round(pairs_c / c_ms / 1e6, 2), fill_ms=round(f_ms, 2),
                   fill_gpairs=round(pairs_f / f_ms / 1e6, 2), grad_abs_max=float(np.abs(g).max()), dZ_abs_max=float(dZ.abs().max()))
        line = json.dumps(rec)
        print(line, flush=True)
        with open(path, "a") as f:
            f.write(line + "\n")
        nat.check(lib.gprc_ctx_trim(ctx.handle))


def main():
    if sys.argv[1:2] == ["grad"]:
        return grad_main([int(a) for a in sys.argv[2:]])
    args = [int(a) for a in sys.argv[1:]]
    n = args[0] if args else 1 << 20
    ms = args[1:] or [2048, 8192, 16384]
    lib = nat.lib()
    ctx = nat.Context(0)
    d, noise, jitter = 8, 0.1, 1e-6
    dev = torch.device("cuda:0")
    theta = 1.0 + np.arange(d) / 16.0
    _, pp, npar = nat.params_array(theta)
    Xh, yh = synth(n, d)
    Xsh, _ = synth(N_STAR, d)
    X, y, Xs = torch.from_numpy(Xh).to(dev), torch.from_numpy(yh).to(dev), torch.from_numpy(Xsh[::-1].copy()).to(dev)
    out = torch.empty((2, N_STAR), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sgpr_bench.txt")
    for m in ms:
        m_pad = int(lib.gprc_pad(m))
        idx = np.sort(np.random.default_rng(m).choice(n, size=m, replace=False))
        Z = torch.from_numpy(np.ascontiguousarray(Xh[idx])).to(dev)
        torch.cuda.synchronize()
        model = C.c_void_p()

        def fit():
            if model:
                nat.check(lib.gprc_model_free(model))
            nat.check(lib.gprc_sgpr_fit(ctx.handle, nat.SQREXP_ARD, pp, npar, X.data_ptr(), d, n, y.data_ptr(), noise, Z.data_ptr(), m, jitter,
                                        C.byref(model)))

        def predict():
            nat.check(lib.gprc_sgpr_predict(model, Xs.data_ptr(), N_STAR, out[0].data_ptr(), out[1].data_ptr()))

        fit_ms = statistics.median(timed(fit, 2))
        lib.gprc_prof_enable(1)
        lib.gprc_prof_reset()
        t0 = time.perf_counter()
        fit()
        prof_ms = (time.perf_counter() - t0) * 1e3
        prof = nat.prof_summary()
        lib.gprc_prof_enable(0)
        stages = dict(fill=prof["fill"]["ms"], solve=sum(prof[k]["ms"] for k in LINV), gram=prof["cov_syrk"]["ms"])
        stages["rest"] = prof_ms - sum(stages.values())
        g = prof["cov_syrk"]
        e, t = C.c_double(), C.c_double()
        nat.check(lib.gprc_sgpr_get_elbo(model, C.byref(e), C.byref(t)))
        predict_ms = statistics.median(timed(predict, 3))
        gram_rows = g["flops"] / g["count"] / (m_pad * (m_pad + 128.0))
        nat.check(lib.gprc_model_free(model))
        nat.check(lib.gprc_ctx_trim(ctx.handle))                     # the chunk workspace goes back before the stand-alone buffers come
        K = max(256, int(round(gram_rows / 256.0)) * 256)
        gram, nt = alone(lib, ctx, m_pad, K)
        flop = K * m_pad * (m_pad + 128.0)
        rec = dict(n=n, m=m, m_pad=m_pad, d=d, fit_ms=round(fit_ms, 2), elbo=e.value, trace=t.value,
                   stages_ms={k: round(v, 2) for k, v in stages.items()}, gram_calls=g["count"], gram_rows=round(gram_rows),
                   gram_fit_tflops=round(g["flops"] / g["ms"] / 1e9, 2), predict_ms=round(predict_ms, 2), n_star=N_STAR, alone_K=K,
                   gram_tflops=round(flop / statistics.median(gram) / 1e9, 2), gram_tflops_range=[round(flop / max(gram) / 1e9, 2), round(flop / min(gram) / 1e9, 2)],
                   nt_tflops=round(flop / statistics.median(nt) / 1e9, 2), nt_tflops_range=[round(flop / max(nt) / 1e9, 2), round(flop / min(nt) / 1e9, 2)],
                   tiles=(m_pad // 128) * (m_pad // 128 + 1) // 2)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(path, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
