"""Accuracy of the device-level building blocks (gprc_dev_*) on ARBITRARY matrices, against the 80-bit reference of
tests/packed_ref.py: factor, block inverses, trailing updates, vector and row solves, row reductions, logp, the cross fill, and
LAPACK's info under every schedule.  Independent of "the same bits as another schedule" (tests/test_gpu_device_level.py) and of the
kernel matrices at noise 0.1 that the parity tests factor.  tests/test_packed_ref_cpu.py runs the same matrices and bounds through
LAPACK, which stays inside all of them.

Bounds (u = 2^-53, gamma_k = k u / (1 - k u)):
  * products, reductions, logp: the derived bounds stated at each test, valid for any summation order;
  * stages that multiply by an explicit inverse (factor: 128 x 128 blocks; trsv, solve_rows: ceiling taken over the 512 x 512 blocks):
        omega <= gamma_{n_pad+1} kappa_blk,   kappa_blk = the largest kappa_inf among the diagonal blocks of the device's factor;
  * and a second, sharper one: omega <= RATIO[stage] * max(omega_LAPACK, u) on the same input (numpy.linalg.cholesky,
    scipy.linalg.solve_triangular; u, one rounding, is the floor below which an omega carries no information: n = 1 has omega = 0).
    RATIO = the next power of two at or above twice the worst ratio measured per stage, at least 4 -- LAPACK's own omega moves by more
    than a factor 2 between rungs and seeds (7.9 u .. 29 u on the ladder).  Measured figures: profiles/blocks_accuracy.txt.

        stage        worst measured omega_gpu / omega_LAPACK                    RATIO
        factor       3.58  (n 1100, cond 1e2: 27.6 u against 7.7 u)               8
        trsv         2.14  (n 1100, cond 1e10, b = L @ ones, L: 3.6 u / 1.7 u)    8
        solve_rows   1.46  (n 1100, cond 1e2, m_pad 128, ld 128: 6.3 u / 4.3 u)   4

With GPRC_BLOCKS_PROFILE=<path> in the environment the measured omegas and ratios are also written to <path>.
"""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.linalg as sl

torch = pytest.importorskip("torch")
import gprc_amd  # noqa: E402,F401
from gprc_amd import _native as nat  # noqa: E402
from conftest import nerr  # noqa: E402
import packed_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

RATIO = {"factor": 8.0, "trsv": 8.0, "solve_rows": 4.0}
U, gamma = R.U, R.gamma
_RECORD = []                                             # (stage, case, omega_gpu, omega_lapack)
_FACTORS = {}                                            # key -> device factor and its host copies, shared by the tests below


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("GPRC_BLOCKS_PROFILE")
    if path and _RECORD:
        with open(path, "w") as f:
            f.write("%-11s %-52s %12s %12s %8s\n" % ("stage", "case", "omega_gpu/u", "omega_lap/u", "ratio"))
            for stage, case, wg, wl in _RECORD:
                f.write("%-11s %-52s %12.3f %12.3f %8.3f\n" % (stage, case, wg / U, wl / U, wg / max(wl, U)))
            for stage in RATIO:
                worst = max((wg / max(wl, U) for s, _, wg, wl in _RECORD if s == stage), default=0.0)
                f.write("worst %-11s %.3f\n" % (stage, worst))


@pytest.fixture
def ctx():
    c = nat.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c
    torch.cuda.synchronize()
    c.close()


def dev(a, dtype=torch.float64):
    """a host array on the device, complete before the library's stream can touch it"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()
    torch.cuda.synchronize()
    return t


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def workspace(g, with_inv=True):
    w = torch.zeros(g.winv_size, dtype=torch.float64, device="cuda")
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    inv = torch.full((int(nat.lib().gprc_solve_inv_size(g.n_pad)),), float("nan"), dtype=torch.float64, device="cuda") if with_inv else None
    torch.cuda.synchronize()
    return w, info, inv


# ---- the schedules: each factors the packed device buffer a in place and returns info ----------------------------------------------
def factor_all(ctx, g, a, w, info, inv=None):
    nat.check(nat.lib().gprc_dev_factor_all(ctx.handle, a.data_ptr(), g.n_pad, w.data_ptr(), info.data_ptr(), inv.data_ptr() if inv is not None else None))
    torch.cuda.synchronize()
    return int(info[0])


def factor_panel_loop(ctx, g, a, w, info, inv=None):
    L = nat.lib()
    for p in range(g.P):
        nat.check(L.gprc_dev_factor_panel(ctx.handle, a.data_ptr(), g.n_pad, p, w.data_ptr(), info.data_ptr()))
        if p + 1 < g.P:
            nat.check(L.gprc_dev_update_trailing(ctx.handle, a.data_ptr(), g.n_pad, p, p + 1, g.P, 1))
    torch.cuda.synchronize()
    return int(info[0])


def factor_quarters(ctx, g, a, w, info, inv=None):
    L = nat.lib()
    for p in range(g.P):
        for j in range(4):
            for part in (1, 2):
                nat.check(L.gprc_dev_factor_subpanel(ctx.handle, a.data_ptr(), g.n_pad, p, j, part, w.data_ptr(), info.data_ptr()))
        if p + 1 < g.P:
            nat.check(L.gprc_dev_update_trailing(ctx.handle, a.data_ptr(), g.n_pad, p, p + 1, g.P, 1))
    torch.cuda.synchronize()
    return int(info[0])


def matrix_of(key):
    if key[0] == "spd":
        _, n, cond, grade = key
        return R.spd(n, cond, R.SEED, grade)
    return key[1] * R.spd(513, 1e2, R.SEED)              # ("scaled", scale)


def factored(ctx, key, schedule=factor_all):
    """K, its device factor under `schedule` (device tensors and host copies) and omega_chol of it; computed once per (key, schedule)"""
    ck = (key, schedule.__name__)
    if ck not in _FACTORS:
        K = matrix_of(key)
        n = K.shape[0]
        g = R.geometry(n)
        a = dev(R.pack(K, n))
        w, info, inv = workspace(g)
        rc = schedule(ctx, g, a, w, info, inv)
        Lp = R.unpack_lower(host(a), g.n_pad)
        f = dict(K=K, n=n, g=g, a=a, w=w, inv=inv, info=rc, Lp=Lp, L=Lp[:n, :n])
        f["omega"] = R.omega_chol(K, f["L"]) if rc == 0 and np.isfinite(Lp).all() else float("inf")
        _FACTORS[ck] = f
    return _FACTORS[ck]


def check_factor(f, stage_case):
    """the assertions of section a on a factor: info, finite, identity padding, omega_chol under both bounds"""
    n, g, Lp, K = f["n"], f["g"], f["Lp"], f["K"]
    assert f["info"] == 0
    assert np.isfinite(Lp).all()
    assert np.array_equal(Lp[n:, n:], np.eye(g.n_pad - n)) and not Lp[n:, :n].any()
    w_lap = R.omega_chol(K, np.linalg.cholesky(K))
    kap = R.kappa_blk(Lp, 128)
    _RECORD.append(("factor", stage_case, f["omega"], w_lap))
    print("factor %s: omega_gpu %.2f u, omega_lapack %.2f u, kappa_blk %.3g, ceiling %.3g u" % (stage_case, f["omega"] / U, w_lap / U, kap,
                                                                                                gamma(g.n_pad + 1) * kap / U))
    assert f["omega"] <= gamma(g.n_pad + 1) * kap, (f["omega"] / U, kap)
    assert f["omega"] <= RATIO["factor"] * max(w_lap, U), (f["omega"] / U, w_lap / U)


# ---- a. factor on arbitrary matrices ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.FACTOR_CASES, ids=R.case_id)
def test_factor_all_on_arbitrary_matrices(ctx, case):
    check_factor(factored(ctx, ("spd",) + case), R.case_id(case))


@pytest.mark.parametrize("scale", R.PIVOT_SCALES)
def test_factor_all_at_the_pivot_extremes(ctx, scale):
    """pivots near 1e-280 and 1e280: sqrt_rsqrt (v_rsq_f64 + Newton steps) and the inverses far from 1"""
    check_factor(factored(ctx, ("scaled", scale)), "n513-cond1e+02-scaled%.0e" % scale)


@pytest.mark.parametrize("schedule", [factor_panel_loop, factor_quarters], ids=["panel-loop", "subpanel-quarters"])
def test_other_schedules_on_the_cond_1e10_matrix(ctx, schedule):
    check_factor(factored(ctx, ("spd", 1100, 1e10, 0), schedule), "n1100-cond1e+10-grade0 " + schedule.__name__)


def test_mvn_factor_on_an_arbitrary_matrix(ctx):
    n, cond, grade = 513, 1e6, 0
    K = np.asfortranarray(R.spd(n, cond, R.SEED, grade))
    Lout = np.empty((n, n), order="F")
    method = C.c_int()
    torch.cuda.synchronize()
    nat.check(nat.lib().gprc_mvn_factor(ctx.handle, K.ctypes.data, n, n, 1e-6, Lout.ctypes.data, C.byref(method)))
    assert method.value == 1
    assert not np.triu(Lout, 1).any()
    g = R.geometry(n)
    f = dict(K=K, n=n, g=g, info=0, Lp=R.pad_identity(Lout, g.n_pad), L=Lout, omega=R.omega_chol(K, Lout) if np.isfinite(Lout).all() else float("inf"))
    check_factor(f, "n513-cond1e+06-grade0 mvn_factor")


# ---- b. block inverses -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cond", [1e2, 1e10])
def test_block_inverses_invert_the_factors_own_diagonal_blocks(ctx, cond):
    """max |T L_bb - I| <= gamma_{b+1} kappa_inf(L_bb) for every 128-block of winv and every 512-block of inv, the latter from
    solve_prepare and from factor_all's inv argument; residual in longdouble, kappa on the host."""
    f = factored(ctx, ("spd", 1100, cond, 0))
    g, Lp = f["g"], f["Lp"]
    assert f["info"] == 0
    winv = host(f["w"])
    for j in range(g.n_pad // 128):
        Lbb = Lp[128 * j:128 * (j + 1), 128 * j:128 * (j + 1)]
        W = R.winv_block(winv, j)
        assert not np.triu(W, 1).any()
        err = float(np.abs(R.tri_times(W, Lbb) - np.eye(128)).max())
        assert err <= gamma(129) * R.kappa_inf_lower(Lbb), (j, err)
    inv_prep = torch.full_like(f["inv"], float("nan"))
    torch.cuda.synchronize()
    nat.check(nat.lib().gprc_dev_solve_prepare(ctx.handle, f["a"].data_ptr(), f["w"].data_ptr(), g.n_pad, inv_prep.data_ptr(), 0, g.P))
    for name, inv in (("factor_all", host(f["inv"])), ("solve_prepare", host(inv_prep))):
        for p in range(g.P):
            Lpp = Lp[512 * p:512 * (p + 1), 512 * p:512 * (p + 1)]
            T, written = R.inv_block(inv, p)
            assert np.isfinite(T[written]).all(), (name, p)
            T = np.tril(np.where(written, T, 0.0))
            err = float(np.abs(R.tri_times(T, Lpp) - np.eye(512)).max())
            assert err <= gamma(513) * R.kappa_inf_lower(Lpp), (name, p, err)


# ---- c. trailing updates alone -----------------------------------------------------------------------------------------------------------
def run_update(ctx, g, packed, sources, targets):
    a = dev(packed)
    L = nat.lib()
    if sources[1] - sources[0] == 1:
        nat.check(L.gprc_dev_update_trailing(ctx.handle, a.data_ptr(), g.n_pad, sources[0], *targets))
    else:
        nat.check(L.gprc_dev_update_range(ctx.handle, a.data_ptr(), g.n_pad, sources[0], sources[1], *targets))
    return host(a)


@pytest.mark.parametrize("call", R.UPDATE_CALLS, ids=[c[0] for c in R.UPDATE_CALLS])
def test_trailing_updates_on_a_buffer_that_is_no_factor(ctx, call):
    """Exact case: small integers, every partial sum an integer below 2^53 -- zero tolerance, any summation order; a missing, doubled
    or misplaced tile shows.  Rounded case: N(0,1), |c_gpu - c_blas| <= 2 gamma_{K+1} (|C| + |A| |B^T|), K = 512 per source panel (both
    sides round, each within gamma_{K+1} of the exact value in any order).  On and below the diagonal of each target; the source panels and
    the targets the stride skips bit-unchanged."""
    name, n_pad, sources, targets = call
    g = R.geometry(n_pad)
    K = g.NB * (sources[1] - sources[0])
    for kind in ("exact", "rounded"):
        packed = (R.small_ints(g.packed_size, R.UPDATE_BITS, R.SEED) if kind == "exact"
                  else np.random.default_rng(R.SEED).normal(size=g.packed_size))
        want, mag = R.update_expected(packed, g, sources, targets)
        got = run_update(ctx, g, packed, sources, targets)
        touched = set(range(*targets))
        for q in range(g.P):
            Cq = R.panel_view(got, g, q)
            if q not in touched:
                assert np.array_equal(Cq, R.panel_view(packed, g, q)), (name, kind, q)      # sources and skipped targets: untouched
                continue
            low = R.lower_mask(g, q)
            if kind == "exact":
                assert np.array_equal(Cq[low], want[q][low]), (name, q, int((Cq[low] != want[q][low]).sum()))
            else:
                assert np.all(np.abs(Cq - want[q])[low] <= 2 * gamma(K + 1) * mag[q][low]), (name, q)


# ---- d. vector solves --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cond", R.SOLVE_CONDS)
def test_trsv_backward_error(ctx, cond):
    f = factored(ctx, ("spd", 1100, cond, 0))
    n, g, L = f["n"], f["g"], f["L"]
    assert f["info"] == 0
    kap = R.kappa_blk(f["Lp"], 512)
    rng = np.random.default_rng(R.SEED + 1)
    work = torch.zeros(g.trsv_work, dtype=torch.float64, device="cuda")
    for rhs, b in (("N(0,1)", rng.normal(size=n)), ("L @ ones", L @ np.ones(n))):
        for transpose in (0, 1):
            x = dev(np.concatenate([b, np.zeros(g.n_pad - n)]))
            nat.check(nat.lib().gprc_dev_trsv(ctx.handle, f["a"].data_ptr(), f["inv"].data_ptr(), g.n_pad, x.data_ptr(), transpose, work.data_ptr()))
            x = host(x)
            assert np.isfinite(x).all() and not x[n:].any()
            wg = R.omega_tri(L, x[:n], b, bool(transpose))
            wl = R.omega_tri(L, sl.solve_triangular(L, b, lower=True, trans=transpose), b, bool(transpose))
            case = "n1100-cond%.0e %s %s" % (cond, rhs, "L^T" if transpose else "L")
            _RECORD.append(("trsv", case, wg, wl))
            print("trsv %s: omega_gpu %.2f u, omega_lapack %.2f u, kappa_blk %.3g" % (case, wg / U, wl / U, kap))
            assert wg <= gamma(g.n_pad + 1) * kap, (case, wg / U)
            assert wg <= RATIO["trsv"] * max(wl, U), (case, wg / U, wl / U)


# ---- e. solve_rows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SOLVE_ROWS_SHAPES, ids=lambda s: "m%d-ld%d" % s)
@pytest.mark.parametrize("cond", R.SOLVE_CONDS)
def test_solve_rows_backward_error(ctx, cond, shape):
    """vt := vt L^-T on an m_pad x n_pad block with leading dimension ld: residual vt_in - V L^T, the zero padding columns stay zero,
    the ld - m_pad rows between the columns are not touched."""
    m_pad, ld = shape
    f = factored(ctx, ("spd", 1100, cond, 0))
    n, g, L = f["n"], f["g"], f["L"]
    assert f["info"] == 0
    kap = R.kappa_blk(f["Lp"], 512)
    rng = np.random.default_rng(R.SEED + 3)
    buf = rng.normal(size=(g.n_pad, ld))                 # [column j of vt, row i]: element (i, j) at i + j ld
    buf[n:, :m_pad] = 0.0
    vt = dev(buf)
    nat.check(nat.lib().gprc_dev_solve_rows(ctx.handle, f["a"].data_ptr(), f["w"].data_ptr(), g.n_pad, vt.data_ptr(), ld, m_pad))
    out = host(vt).reshape(g.n_pad, ld)
    assert np.isfinite(out).all()
    assert np.array_equal(out[:, m_pad:], buf[:, m_pad:])
    assert not out[n:, :m_pad].any()
    B, X = buf[:n, :m_pad], out[:n, :m_pad]              # columns = right-hand sides: L X = B
    wg = R.omega_tri(L, X, B)
    wl = R.omega_tri(L, sl.solve_triangular(L, B, lower=True), B)
    case = "n1100-cond%.0e m_pad %d ld %d" % (cond, m_pad, ld)
    _RECORD.append(("solve_rows", case, wg, wl))
    print("solve_rows %s: omega_gpu %.2f u, omega_lapack %.2f u, kappa_blk %.3g" % (case, wg / U, wl / U, kap))
    assert wg <= gamma(g.n_pad + 1) * kap, (case, wg / U)
    assert wg <= RATIO["solve_rows"] * max(wl, U), (case, wg / U, wl / U)


# ---- f. row_reduce -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gap", [0, 128])
@pytest.mark.parametrize("rows", R.REDUCE_ROWS)
def test_row_reduce_column_tails(ctx, rows, gap):
    """out[i] = sum_j vt[i + j ld] w[j] (w NULL: sum of squares) at column counts around the 4-column unrolling and the 512-column
    splits.  Exact: integers of 20 bits, sums below 2^53.  Rounded: N(0,1), error <= gamma_cols sum |v| |w| (any order, fma or not)."""
    L = nat.lib()
    ld = rows + gap
    for cols in R.REDUCE_COLS:
        work = torch.zeros(rows * int(L.gprc_rowreduce_splits(cols)), dtype=torch.float64, device="cuda")
        for kind in ("exact", "rounded"):
            if kind == "exact":
                buf, w = R.small_ints((cols, ld), R.REDUCE_BITS, cols), R.small_ints(cols, R.REDUCE_BITS, cols + 1)
            else:
                rng = np.random.default_rng(cols)
                buf, w = rng.normal(size=(cols, ld)), rng.normal(size=cols)
            V = buf[:, :rows].T                          # rows x cols; the gap rows hold data that must not enter
            vt, wd = dev(buf), dev(w)
            for mode in ("dot", "sumsq"):
                out = torch.full((rows,), float("nan"), dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()
                nat.check(L.gprc_dev_row_reduce(ctx.handle, vt.data_ptr(), ld, rows, cols, wd.data_ptr() if mode == "dot" else None,
                                                out.data_ptr(), work.data_ptr()))
                got = host(out)
                if kind == "exact":
                    Vi, wi = V.astype(np.int64), w.astype(np.int64)
                    want = (Vi @ wi if mode == "dot" else (Vi * Vi).sum(1)).astype(np.float64)
                    assert np.array_equal(got, want), (cols, mode)
                else:
                    ref = R.rows_dot_ld(V, w if mode == "dot" else None)
                    mag = np.abs(V) @ np.abs(w) if mode == "dot" else (V * V).sum(1)
                    assert np.all(np.abs(got - ref) <= gamma(cols) * mag), (cols, mode)


# ---- g. logp -------------------------------------------------------------------------------------------------------------------------------
def test_logp_on_a_graded_factor(ctx):
    """-1/2 y.alpha - sum log L_ii - n/2 log 2 pi on the factor whose diagonal spans about 12 decades, against longdouble:
    error <= gamma_{n+2} (1/2 sum |y alpha| + sum |log L_ii| + n/2 log 2 pi)."""
    f = factored(ctx, ("spd",) + R.FACTOR_CASES[-1])
    n, g = f["n"], f["g"]
    assert f["info"] == 0
    rng = np.random.default_rng(R.SEED + 2)
    y, alpha = rng.normal(size=g.n_pad), rng.normal(size=g.n_pad)
    out = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    yd, ad = dev(y), dev(alpha)
    nat.check(nat.lib().gprc_dev_logp(ctx.handle, f["a"].data_ptr(), g.n_pad, n, yd.data_ptr(), ad.data_ptr(), out.data_ptr()))
    got = float(host(out)[0])
    ref, mag = R.logp_ld(f["Lp"], n, y, alpha)
    assert abs(R.LD(got) - ref) <= gamma(n + 2) * mag, (got, float(ref))


# ---- h. fill_cross -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 17])
@pytest.mark.parametrize("kind,kid,par", [("sqrexp", nat.SQREXP, [0.8]), ("rationalquadratic", nat.RATQUAD, [1.1, 1.5])], ids=["sqrexp", "ratquad"])
def test_fill_cross_against_the_oracle(ctx, orc, kind, kid, par, d):
    n = 513
    n_pad = R.geometry(n).n_pad
    rng = np.random.default_rng(d)
    X = rng.uniform(-1, 1, (n, d))                       # one point per row of the host array = per column of the d x n matrix
    Xd = dev(X)
    _, pp, npar = nat.params_array(par)
    for m, m_pad in [(1, 128), (127, 128), (129, 256)]:
        ld = m_pad + 128
        Xs = rng.uniform(-1, 1, (m, d))
        Xsd = dev(Xs)
        buf = rng.normal(size=(n_pad, ld))
        vt = dev(buf)
        nat.check(nat.lib().gprc_dev_fill_cross(ctx.handle, kid, pp, npar, Xsd.data_ptr(), d, m, m_pad, Xd.data_ptr(), n, n_pad, vt.data_ptr(), ld))
        out = host(vt).reshape(n_pad, ld)
        ref = orc.kernel_matrix(orc.KERNEL_IDS[kind], par, Xs.T, X.T)            # m x n
        assert nerr(out[:n, :m].T, ref) <= 1e-13, (kind, d, m)
        assert not out[:n, m:m_pad].any() and not out[n:, :m_pad].any()         # exact zeros in the padding
        assert np.array_equal(out[:, m_pad:], buf[:, m_pad:])                   # the ld gap is not touched


# ---- i. info is the FIRST failing minor, under every schedule --------------------------------------------------------------------------------
_NOT_PD = {}


def not_pd_packed(k):
    if k not in _NOT_PD:
        _NOT_PD[k] = R.pack(R.not_pd_at(R.INFO_N, k, R.SEED), R.INFO_N)
    return _NOT_PD[k]


def infos(ctx, schedule):
    g = R.geometry(R.INFO_N)
    got = {}
    for k in R.INFO_KS:
        a = dev(not_pd_packed(k))
        w, info, _ = workspace(g, with_inv=False)
        got[k] = schedule(ctx, g, a, w, info)
    return got


def test_info_is_the_first_failing_minor_with_the_service(ctx):
    was = nat.lib().gprc_factor_service(1)               # on is the default; an earlier wait timeout in the process may have switched it off
    try:
        assert infos(ctx, factor_all) == {k: k for k in R.INFO_KS}
    finally:
        nat.lib().gprc_factor_service(was)


def test_info_is_the_first_failing_minor_without_the_service(ctx):
    was = nat.lib().gprc_factor_service(0)
    try:
        assert infos(ctx, factor_all) == {k: k for k in R.INFO_KS}
    finally:
        nat.lib().gprc_factor_service(was)


def test_info_is_the_first_failing_minor_in_groups_of_one_panel(ctx, monkeypatch):
    monkeypatch.setenv("GPRC_FACTOR", "1")
    assert infos(ctx, factor_all) == {k: k for k in R.INFO_KS}


def test_info_is_the_first_failing_minor_in_the_panel_loop(ctx):
    assert infos(ctx, factor_panel_loop) == {k: k for k in R.INFO_KS}


def test_info_is_the_first_failing_minor_in_the_subpanel_quarters(ctx):
    assert infos(ctx, factor_quarters) == {k: k for k in R.INFO_KS}


def test_info_of_an_exactly_singular_matrix_is_two(ctx):
    n = 600
    g = R.geometry(n)
    a = dev(R.pack(R.rank_one(n, R.SEED), n))
    w, info, _ = workspace(g, with_inv=False)
    assert factor_all(ctx, g, a, w, info) == 2
