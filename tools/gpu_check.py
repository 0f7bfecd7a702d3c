"""Bring-up diagnostics on a real MI355X: every native stage against the CPU oracle, stage by stage,
so a failure is localised to one kernel.  (The judged parity tests are tests/test_gpu_*.py; this
script is the verbose developer version of them.)"""
import ctypes as C
import importlib.util
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gprc_amd  # noqa: E402
from gprc_amd import _native as nat  # noqa: E402
from oracle import oracle as orc  # noqa: E402

import torch  # noqa: E402

FAILS = []


def report(name, got, ref, tol=1e-10):
    got, ref = np.asarray(got), np.asarray(ref)
    scale = max(np.abs(ref).max(), 1e-300)
    err = np.abs(got - ref).max() / scale if got.shape == ref.shape else float("inf")
    ok = bool(err <= tol) and np.isfinite(got).all()
    print(f"{'OK  ' if ok else 'FAIL'} {name:58s} normwise err {err:.3e}", flush=True)
    if not ok:
        FAILS.append(name)
    return ok


def main():
    L = nat.lib()
    print("devices:", nat.device_count())
    ctx = nat.default_context(0)
    rng = np.random.default_rng(20261004)
    kernels = [("constant", orc.CONSTANT, [1.7]), ("linear", orc.LINEAR, [0.7]), ("linear_vec", orc.LINEAR, None),
               ("polynomial", orc.POLYNOMIAL, [0.5, 3.0]), ("sqrexp", orc.SQREXP, [1.3]),
               ("gammaexp", orc.GAMMAEXP, [0.9, 1.5]), ("ratquad", orc.RATQUAD, [1.1, 1.5])]
    # ---- 1. kernel fill ------------------------------------------------------------------------
    for d, nA, nB in [(1, 5, 3), (2, 130, 67), (8, 257, 300), (20, 64, 129)]:
        A = np.asfortranarray(rng.uniform(-1, 1, (d, nA)))
        B = np.asfortranarray(rng.uniform(-1, 1, (d, nB)))
        for name, kid, par in kernels:
            if par is None:
                par = list(rng.uniform(0.2, 1.5, d))
            out = np.empty((nA, nB), order="F")
            p, pp, npar = nat.params_array(par)
            nat.check(L.gprc_kernel_matrix(ctx.handle, kid, pp, npar, A.ctypes.data, d, nA, B.ctypes.data, nB, out.ctypes.data, nA))
            report(f"kernel_matrix {name} d={d} {nA}x{nB}", out, orc.kernel_matrix(kid, par, A, B), 1e-13)
    # ---- 2. staged factorisation on device buffers ------------------------------------------------
    # (the asserted form of this stage, on arbitrary matrices against an 80-bit reference: tests/test_gpu_blocks.py)
    dev = torch.device("cuda:0")
    for n in (300, 1000, 1500):
        d = 8
        X = np.asfortranarray(rng.uniform(-1, 1, (d, n)))
        par = [1.0]
        noise = 0.1
        n_pad = L.gprc_pad(n)
        P = L.gprc_panel_count(n_pad)
        NB = L.gprc_panel_width()
        Kref = orc.kernel_matrix(orc.SQREXP, par, X, X) + noise * np.eye(n)
        Kpad = np.eye(n_pad)
        Kpad[:n, :n] = Kref
        Xd = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)  # memory = point-major, same bytes as F-order d x n
        packed = torch.zeros(L.gprc_packed_size(n_pad), dtype=torch.float64, device=dev)
        winv = torch.zeros(L.gprc_winv_size(n_pad), dtype=torch.float64, device=dev)
        info = torch.zeros(4, dtype=torch.int32, device=dev)
        p, pp, npar = nat.params_array(par)
        torch.cuda.synchronize()

        def panel_np(pk, q):
            off = L.gprc_panel_offset(n_pad, q)
            ld = n_pad - q * NB
            return pk[off:off + ld * NB].reshape(NB, ld).T  # (ld, NB) view in matrix orientation

        for q in range(P):
            nat.check(L.gprc_dev_fill_panel(ctx.handle, orc.SQREXP, pp, npar, Xd.data_ptr(), d, n, n_pad, noise, packed.data_ptr(), q))
        ctx.synchronize()
        pk = packed.cpu().numpy()
        for q in range(P):
            report(f"fill_panel n={n} panel {q}", panel_np(pk, q), Kpad[q * NB:, q * NB:(q + 1) * NB], 1e-13)
        Lref = np.linalg.cholesky(Kpad)
        Awork = Kpad.copy()
        for q in range(P):
            nat.check(L.gprc_dev_factor_panel(ctx.handle, packed.data_ptr(), n_pad, q, winv.data_ptr(), info.data_ptr()))
            ctx.synchronize()
            pk = packed.cpu().numpy()
            got = np.tril(panel_np(pk, q), 0) if True else None
            ref = Lref[q * NB:, q * NB:(q + 1) * NB]
            # only the lower part of the diagonal block is defined
            g = panel_np(pk, q).copy()
            g[:NB, :NB] = np.tril(g[:NB, :NB])
            report(f"factor_panel n={n} panel {q}", g, ref, 1e-11)
            wv = winv.cpu().numpy()
            for j in range(NB // 128):
                blk = q * (NB // 128) + j
                W = wv[blk * 16384:(blk + 1) * 16384].reshape(128, 128).T
                c = q * NB + j * 128
                report(f"  winv n={n} block {blk}", W, np.linalg.inv(Lref[c:c + 128, c:c + 128]), 1e-10)
            if q + 1 < P:
                nat.check(L.gprc_dev_update_trailing(ctx.handle, packed.data_ptr(), n_pad, q, q + 1, P, 1))
                ctx.synchronize()
                pk = packed.cpu().numpy()
                Lq = Lref[(q + 1) * NB:, q * NB:(q + 1) * NB]
                Awork[(q + 1) * NB:, (q + 1) * NB:] -= Lq @ Lq.T
                for r in range(q + 1, P):
                    g = panel_np(pk, r).copy()
                    refp = Awork[r * NB:, r * NB:(r + 1) * NB].copy()
                    g[:NB, :NB] = np.tril(g[:NB, :NB])
                    refp[:NB, :NB] = np.tril(refp[:NB, :NB])
                    report(f"  trailing n={n} after {q}: panel {r}", g, refp, 1e-11)
        print("info:", info.cpu().numpy()[0])
        # trsv
        y = rng.normal(size=n)
        ypad = np.zeros(n_pad)
        ypad[:n] = y
        b = torch.from_numpy(ypad.copy()).to(dev)
        work = torch.zeros(L.gprc_trsv_work_size(n_pad), dtype=torch.float64, device=dev)
        inv = torch.zeros(L.gprc_solve_inv_size(n_pad), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        nat.check(L.gprc_dev_solve_prepare(ctx.handle, packed.data_ptr(), winv.data_ptr(), n_pad, inv.data_ptr(), 0, P))
        nat.check(L.gprc_dev_trsv(ctx.handle, packed.data_ptr(), inv.data_ptr(), n_pad, b.data_ptr(), 0, work.data_ptr()))
        ctx.synchronize()
        import scipy.linalg as sl
        z = sl.solve_triangular(Lref, ypad, lower=True)
        report(f"trsv forward n={n}", b.cpu().numpy(), z, 1e-11)
        nat.check(L.gprc_dev_trsv(ctx.handle, packed.data_ptr(), inv.data_ptr(), n_pad, b.data_ptr(), 1, work.data_ptr()))
        ctx.synchronize()
        report(f"trsv backward n={n}", b.cpu().numpy(), sl.solve_triangular(Lref.T, z, lower=False), 1e-11)
        # cross fill + solve_rows + reductions
        m = 200
        Xs = np.asfortranarray(rng.uniform(-1, 1, (d, m)))
        m_pad = 256
        Xsd = torch.from_numpy(np.ascontiguousarray(Xs.T)).to(dev)
        vt = torch.zeros(m_pad * n_pad, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        nat.check(L.gprc_dev_fill_cross(ctx.handle, orc.SQREXP, pp, npar, Xsd.data_ptr(), d, m, m_pad, Xd.data_ptr(), n, n_pad, vt.data_ptr(), m_pad))
        ctx.synchronize()
        Kst = np.zeros((m_pad, n_pad))
        Kst[:m, :n] = orc.kernel_matrix(orc.SQREXP, par, Xs, X)
        report(f"fill_cross n={n}", vt.cpu().numpy().reshape(n_pad, m_pad).T, Kst, 1e-13)
        w = torch.from_numpy(rng.normal(size=n_pad)).to(dev)
        out = torch.zeros(m_pad, dtype=torch.float64, device=dev)
        rwork = torch.zeros(m_pad * L.gprc_rowreduce_splits(n_pad), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        nat.check(L.gprc_dev_row_reduce(ctx.handle, vt.data_ptr(), m_pad, m_pad, n_pad, w.data_ptr(), out.data_ptr(), rwork.data_ptr()))
        ctx.synchronize()
        report(f"row_reduce dot n={n}", out.cpu().numpy(), Kst @ w.cpu().numpy(), 1e-12)
        nat.check(L.gprc_dev_solve_rows(ctx.handle, packed.data_ptr(), winv.data_ptr(), n_pad, vt.data_ptr(), m_pad, m_pad))
        ctx.synchronize()
        Vref = sl.solve_triangular(Lref, Kst.T, lower=True).T
        report(f"solve_rows n={n}", vt.cpu().numpy().reshape(n_pad, m_pad).T, Vref, 1e-11)
        nat.check(L.gprc_dev_row_reduce(ctx.handle, vt.data_ptr(), m_pad, m_pad, n_pad, 0, out.data_ptr(), rwork.data_ptr()))
        ctx.synchronize()
        report(f"row_reduce sumsq n={n}", out.cpu().numpy(), (Vref * Vref).sum(1), 1e-11)

    # ---- 3. high level ----------------------------------------------------------------------------
    from gprc_amd import GPR, GPC, cov_func, sqrexp, rationalquadratic
    for n, d, ns in [(2, 1, 1), (17, 2, 5), (300, 8, 77), (1100, 8, 300)]:
        X = np.asfortranarray(rng.uniform(-1, 1, (d, n)))
        y = 0.1 * (X ** 3).sum(0) + rng.normal(0, 0.1, n)
        Xs = np.asfortranarray(rng.uniform(-1, 1, (d, ns)))
        for kname, kf, kid, par in [("sqrexp", cov_func(sqrexp, l=1.0), orc.SQREXP, [1.0]),
                                    ("ratquad", cov_func(rationalquadratic, l=1.0, alpha=1.5), orc.RATQUAD, [1.0, 1.5])]:
            g = GPR(X, y, 0.1, kf)
            f = orc.gpr_fit(kid, par, X, y, 0.1)
            report(f"GPR {kname} n={n} L", g.L, f["L"], 1e-10)
            report(f"GPR {kname} n={n} alpha", g.alpha, f["alpha"], 1e-10)
            report(f"GPR {kname} n={n} logp", [g.logp], [f["logp"]], 1e-10)
            pr = g.predict(Xs)
            mr, vr = orc.gpr_predict(kid, par, X, f["L"], f["alpha"], Xs)
            report(f"GPR {kname} n={n} mean", pr[:, 0], mr, 1e-10)
            report(f"GPR {kname} n={n} var", pr[:, 1], vr, 1e-10)
            mean2, cov2 = g.predict(Xs, pointwise_var=False)
            mr2, cr2 = orc.gpr_predict(kid, par, X, f["L"], f["alpha"], Xs, pointwise=False)
            report(f"GPR {kname} n={n} cov", cov2, cr2, 1e-10)
    # non-PD + jitter
    Xdup = np.zeros((1, 6))
    Xdup[0] = [0.0, 0.0, 1.0, 1.0, 2.0, 3.0]
    import warnings
    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter("always")
        g = GPR(Xdup, np.arange(6.0), 0.0, cov_func(sqrexp, l=1.0))
        f = orc.gpr_fit(orc.SQREXP, [1.0], Xdup, np.arange(6.0), 0.0)
        print("jitter: noise", g.noise, "oracle", f["noise"], "attempts", f["attempts"], "warnings", [str(w.message) for w in wl])
        report("jitter L", g.L, f["L"], 1e-9)
    # GPC
    Xc = np.linspace(-1, 1, 21).reshape(1, -1)
    yc = 2.0 * (Xc[0] > 0) - 1
    kc = cov_func(sqrexp, l=math.sqrt(1 / 6))
    gc = GPC(Xc, yc, kc, 1e-5)
    oc = orc.gpc_fit(orc.SQREXP, [math.sqrt(1 / 6)], Xc, yc, 1e-5)
    print("GPC iters", gc.iterations, oc["iters"])
    report("GPC f_hat", gc.f_hat, oc["f_hat"], 1e-9)
    report("GPC logq", [gc.logq], [oc["logq"]], 1e-9)
    report("GPC L", gc.L, oc["L"], 1e-9)
    xs = np.array([[-0.2, 0.2, 0.5]])
    fs, vf = gc.predict_latent(xs)
    ofs, ovf = orc.gpc_predict_latent(orc.SQREXP, [math.sqrt(1 / 6)], Xc, yc, oc["f_hat"], oc["L"], xs)
    report("GPC fs_bar", fs, ofs, 1e-9)
    report("GPC Vfs", vf, ovf, 1e-9)
    print("GPC predict_class", gc.predict_class(xs))

    # ---- 4. first timing --------------------------------------------------------------------------
    for n, ns in [(8192, 8192), (16384, 16384)]:
        d = 8
        X = np.asfortranarray(rng.uniform(-1, 1, (d, n)))
        y = 0.1 * (X ** 3).sum(0) + rng.normal(0, 0.1, n)
        Xs = np.asfortranarray(rng.uniform(-1, 1, (d, ns)))
        kf = cov_func(sqrexp, l=1.0)
        g = GPR(X, y, 0.1, kf)
        t0 = time.perf_counter(); g = GPR(X, y, 0.1, kf); t1 = time.perf_counter()
        pr = g.predict(Xs); t2 = time.perf_counter()
        print(f"n={n} ns={ns}: fit {1e3*(t1-t0):.1f} ms ({n**3/3/(t1-t0)*1e-12:.2f} TF)  predict {1e3*(t2-t1):.1f} ms ({n*n*ns/(t2-t1)*1e-12:.2f} TF)", flush=True)
    print("FAILED:", FAILS if FAILS else "none")
    return 1 if FAILS else 0


if __name__ == "__main__":
    sys.exit(main())
