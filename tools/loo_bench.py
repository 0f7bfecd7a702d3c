"""Leave-one-out cross-validation against its two yardsticks, on tools/grad_bench.py's inputs and conventions: d = 8, noise 0.1, bench.py's
C4 inputs (X ~ U[-1, 1], y = 0.1 sum(x^3) + N(0, 0.1^2), Philox seed 20261004) resident in device memory; kernels sqrexp_ard and
matern52_ard (l_k = 1 + k / 16).
    python tools/loo_bench.py                          # n = 4096 8192 16384 32768
    python tools/loo_bench.py 16384                    # the sizes named
Per (n, kernel) one JSON line, every time the median of 5 calls after a warm-up (host clock around the synchronous C-ABI call):
  loo_grad_ms beside logp_grad_ms of the same run, and their ratio (2 n^3 against n^3 flop says about 2 at large n);
  loo_model_ms = gprc_gpr_loo with all four outputs on a resident model, beside fit_ms = gprc_gpr_fit of that model;
  stages_ms = one further gprc_gpr_loo_grad under the in-library event profiler, grouped into fit / linv (the identity through the predict
  solve) / inverse_gemm / q_build (kind 18, shared with the reversed factor: none is built in this call) / syrk (kind 8) / contraction
  (kind 17) / trsv (the fit's two vector solves and u's two);
  syrk_tflops = the SYRK's algorithmic flops (the lower triangle, n_pad^3) over its event time; q_build_gbs = 2 n_pad^2 doubles (read
  once, written once) over the builder's event time.
Per n one further line: reverse_factor_ms / reverse_factor_gbs, launch_reverse_factor (gprc_dev_reverse_factor) on buffers of the same
n_pad under the same profiler, mean of 5 launches after a warm-up -- the builder's yardstick, measured in the same run."""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import gprc_amd  # noqa: F401
from gprc_amd import _native as nat
from grad_bench import LINV, synth, timed


def main():
    sizes = [int(a) for a in sys.argv[1:] if not a.startswith("--")] or [4096, 8192, 16384, 32768]
    lib = nat.lib()
    ctx = nat.default_context().handle
    d, noise = 8, 0.1
    dev = torch.device("cuda:0")
    kernels = [("sqrexp_ard", nat.SQREXP_ARD, 1.0 + np.arange(d) / 16.0), ("matern52_ard", nat.MATERN52_ARD, 1.0 + np.arange(d) / 16.0)]
    for n in sizes:
        Xh, yh = synth(n, d)
        X, y = torch.from_numpy(Xh).to(dev), torch.from_numpy(yh).to(dev)
        outs = torch.empty((3, n), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        for name, kid, theta in kernels:
            _, pp, npar = nat.params_array(theta)
            val, grad, score = C.c_double(), np.empty(npar + 1), C.c_double()
            gp = grad.ctypes.data_as(C.POINTER(C.c_double))
            model = C.c_void_p()

            def logp_grad():
                nat.check(lib.gprc_gpr_logp_grad(ctx, kid, pp, npar, X.data_ptr(), d, n, y.data_ptr(), noise, C.byref(val), gp))

            def loo_grad():
                nat.check(lib.gprc_gpr_loo_grad(ctx, kid, pp, npar, X.data_ptr(), d, n, y.data_ptr(), noise, C.byref(val), gp))

            def fit():
                if model:
                    nat.check(lib.gprc_model_free(model))
                nat.check(lib.gprc_gpr_fit(ctx, kid, pp, npar, X.data_ptr(), d, n, y.data_ptr(), noise, C.byref(model)))

            def loo_model():
                nat.check(lib.gprc_gpr_loo(model, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), C.byref(score)))

            rec = dict(n=n, d=d, kernel=name, params=npar)
            for key, f in (("logp_grad", logp_grad), ("loo_grad", loo_grad), ("fit", fit), ("loo_model", loo_model)):
                runs = timed(f, 5)
                rec[key + "_ms"], rec[key + "_runs"] = round(statistics.median(runs), 2), [round(v, 2) for v in runs]
            rec["loo_grad_over_logp_grad"] = round(rec["loo_grad_ms"] / rec["logp_grad_ms"], 2)
            rec["loo_model_over_fit"] = round(rec["loo_model_ms"] / rec["fit_ms"], 2)
            rec["loo"], rec["loo_model_score"] = val.value, score.value
            nat.check(lib.gprc_model_free(model))
            lib.gprc_prof_reset()
            lib.gprc_prof_enable(1)
            loo_grad()
            lib.gprc_prof_enable(0)
            prof = {k: v for k, v in nat.prof_summary().items() if v["count"]}
            lib.gprc_prof_reset()
            named = ("inverse_gemm", "reverse_factor", "cov_syrk", "gpc_grad_contract", "trsv")
            linv = sum(v["ms"] for k, v in prof.items() if k in LINV)
            rest = sum(v["ms"] for k, v in prof.items() if k not in LINV + named)
            rec["stages_ms"] = dict(fit=round(rest, 2), linv=round(linv, 2), inverse_gemm=round(prof["inverse_gemm"]["ms"], 2),
                                    q_build=round(prof["reverse_factor"]["ms"], 3), syrk=round(prof["cov_syrk"]["ms"], 2),
                                    contraction=round(prof["gpc_grad_contract"]["ms"], 3), trsv=round(prof["trsv"]["ms"], 3))
            rec["syrk_tflops"] = round(prof["cov_syrk"]["flops"] / prof["cov_syrk"]["ms"] / 1e9, 1)
            rec["q_build_gbs"] = round(prof["reverse_factor"]["bytes"] / prof["reverse_factor"]["ms"] / 1e6, 1)
            print(json.dumps(rec), flush=True)
        # the builder's yardstick in the same run: launch_reverse_factor on buffers of this n_pad (data movement: the contents do not matter)
        n_pad = lib.gprc_pad(n)
        bufs = [torch.zeros(lib.gprc_packed_size(n_pad), dtype=torch.float64, device=dev) for _ in range(2)]
        winvs = [torch.zeros(lib.gprc_winv_size(n_pad), dtype=torch.float64, device=dev) for _ in range(2)]
        torch.cuda.synchronize()

        def reverse():
            nat.check(lib.gprc_dev_reverse_factor(ctx, bufs[0].data_ptr(), winvs[0].data_ptr(), n_pad, bufs[1].data_ptr(), winvs[1].data_ptr()))
            nat.check(lib.gprc_ctx_synchronize(ctx))
        reverse()
        lib.gprc_prof_reset()
        lib.gprc_prof_enable(1)
        for _ in range(5):
            reverse()
        lib.gprc_prof_enable(0)
        rv = nat.prof_summary()["reverse_factor"]
        lib.gprc_prof_reset()
        print(json.dumps(dict(n=n, n_pad=n_pad, reverse_factor_ms=round(rv["ms"] / rv["count"], 3),
                              reverse_factor_gbs=round(rv["bytes"] / rv["ms"] / 1e6, 1))), flush=True)
        del X, y, outs, bufs, winvs
        nat.check(lib.gprc_ctx_trim(ctx))


if __name__ == "__main__":
    main()
