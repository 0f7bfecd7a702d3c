"""gprc_gpr_extend against a fresh fit of the concatenated data: sqrexp (l = 1), d = 8, noise 0.1, bench.py's C4 inputs
(X ~ U[-1, 1], y = 0.1 sum(x^3) + N(0, 0.1^2), Philox seed 20261004) for n + m points; the base model is the first n.
    python tools/extend_bench.py                       # the default cases
    python tools/extend_bench.py 65536:1024 8192:1     # n:m pairs
    python tools/extend_bench.py --prof ...            # + one extend under the in-library event profiler, per stage
extend: median of 5 runs, each on a freshly fitted base model (the fit is not timed); fit: median of 3 after one warm-up.
Both are wall times of the one C-ABI call, inputs in host memory (64 KB at m = 1024)."""
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import gprc_amd  # noqa: F401
from gprc_amd import _native as nat

SEED = 20261004
DEFAULT = [(65536, 1), (65536, 64), (65536, 1024), (8192, 1), (8192, 512), (16384, 1), (16384, 512)]


def synth(n, d):
    rng = np.random.Generator(np.random.Philox(SEED))
    X = rng.uniform(-1.0, 1.0, size=(n, d))          # row i = point i (== d x n column-major)
    y = 0.1 * (X ** 3).sum(1) + rng.normal(0.0, 0.1, size=n)
    return np.ascontiguousarray(X), y


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    prof = "--prof" in sys.argv
    cases = [tuple(int(v) for v in a.split(":")) for a in args] or DEFAULT
    lib = nat.lib()
    ctx = nat.default_context().handle
    d, noise = 8, 0.1
    _, pp, npar = nat.params_array([1.0])

    def fit(X, y, n):
        m = C.c_void_p()
        nat.check(lib.gprc_gpr_fit(ctx, nat.SQREXP, pp, npar, X.ctypes.data, d, n, y.ctypes.data, noise, C.byref(m)))
        return m

    for n, m in cases:
        X, y = synth(n + m, d)
        Xn, yn = np.ascontiguousarray(X[n:]), np.ascontiguousarray(y[n:])
        fit_ms = []
        for rep in range(4):
            t0 = time.perf_counter()
            h = fit(X, y, n + m)
            fit_ms.append((time.perf_counter() - t0) * 1e3)
            if rep == 0:
                a_ref, lp_ref = np.empty(n + m), C.c_double()
                nat.check(lib.gprc_gpr_get_alpha(h, a_ref.ctypes.data))
                nat.check(lib.gprc_gpr_get_logp(h, C.byref(lp_ref)))
            lib.gprc_model_free(h)
        ext_ms = []
        for rep in range(7 if prof else 6):   # 0: warm-up + accuracy check, 1..5 timed, 6: profiled
            h = fit(X, y, n)
            nat.check(lib.gprc_ctx_synchronize(ctx))
            if rep == 6:
                lib.gprc_prof_reset()
                lib.gprc_prof_enable(1)
            t0 = time.perf_counter()
            nat.check(lib.gprc_gpr_extend(h, Xn.ctypes.data, m, yn.ctypes.data))
            dt = (time.perf_counter() - t0) * 1e3
            if rep == 6:
                lib.gprc_prof_enable(0)
                stages = {k: round(v["ms"], 3) for k, v in nat.prof_summary().items() if v["count"]}
            elif rep > 0:
                ext_ms.append(dt)
            if rep == 0:
                a, lp = np.empty(n + m), C.c_double()
                nat.check(lib.gprc_gpr_get_alpha(h, a.ctypes.data))
                nat.check(lib.gprc_gpr_get_logp(h, C.byref(lp)))
                err = float(np.abs(a - a_ref).max() / np.abs(a_ref).max())
                lp_err = abs(lp.value - lp_ref.value) / abs(lp_ref.value)
            lib.gprc_model_free(h)
        rec = dict(n=n, m=m, n_new=n + m, extend_ms=round(statistics.median(ext_ms), 2), extend_runs=[round(v, 2) for v in ext_ms],
                   fit_ms=round(statistics.median(fit_ms[1:]), 2), fit_runs=[round(v, 2) for v in fit_ms[1:]])
        rec["ratio"] = round(rec["extend_ms"] / rec["fit_ms"], 4)
        rec["alpha_nerr_vs_fit"], rec["logp_rel_vs_fit"] = float(f"{err:.3e}"), float(f"{lp_err:.3e}")
        if prof:
            rec["profiled_stages_ms"] = stages
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
