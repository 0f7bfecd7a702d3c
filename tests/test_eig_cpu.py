"""tests/eig_ref.py on the CPU: the schedule, the constructed spectra against 40-digit mpmath, the long-double checks against plain
longdouble products, the float64 model of the device's Jacobi inside every bound of the module's docstring, and -- for each assertion that
tests/test_gpu_eig.py makes -- a deliberately wrong model that fails it, so that no assertion there is one a wrong kernel would pass.

    assertion of the GPU test                         wrong model that fails it
    resid, orth, eig inside the analytic bounds       c and s rounded to float32
    sweeps < 40                                       one pair skipped in every round (runs into the cap)
    values non-increasing                             ascending sort
    resid <= rel + 4 resid_model                      stop rule at 1e-12 (graded); off-norm by cancellation (clusters); V left unrotated once
    orth <= 4 max(orth_model, m u)                    c and s rounded to float32
    sweeps <= sweeps_model + 1                        one pair skipped in every round
    exact cases: 0 sweeps, bits, ties in index order  ascending sort; unstable tie order
    scale: bits at 2^+-300, bounds at 2^-1000 .. 2^+1000     the sweeps on the unscaled matrix (the code before the range fix)
    products: gamma_{k+1} (|mean| + |L| |Z|)          L rounded to float32;  Cholesky: gamma_{m+1} |L| |L|^T with one entry of L moved by 1e-12
"""
import numpy as np
import pytest

import eig_ref as R
import packed_ref as P

LD = R.LD
SIZES = [1, 2, 3, 5, 64, 257]
CASES = [(f, 129) for f in R.FAMILIES] + [(f, m) for m in SIZES for f in ("psd", "indefinite")] + [("nearly-diagonal", 2)]


def run(name, m, **kw):
    A, lam = R.family(name, m)
    val, V, sweeps = R.jacobi(A, **kw)
    return A, lam, val, V, R.check_decomposition(A, lam, val, V, sweeps)


_MODEL = {}


def model(name, m):
    if (name, m) not in _MODEL:
        _MODEL[name, m] = run(name, m)
    return _MODEL[name, m]


def test_schedule_visits_every_pair_once_per_sweep():
    for m in range(1, 71):
        mm = m + (m & 1)
        seen = []
        for r in range(mm - 1):
            P_, Q_ = R.round_pairs(m, r)
            used = np.concatenate([P_, Q_])
            assert len(set(used.tolist())) == used.size                 # the pairs of a round are disjoint
            assert np.all(P_ < Q_) and np.all(Q_ < m)
            seen += list(zip(P_.tolist(), Q_.tolist()))
        assert sorted(seen) == [(p, q) for p in range(m) for q in range(p + 1, m)], m


@pytest.mark.parametrize("lam", [np.logspace(0.0, -16.0, 24), R.clusters_spectrum(24), R.clusters_spectrum(7), R.mvn_spectrum(24, -1e-9),
                                 R.mvn_spectrum(24, 1e-13)], ids=["graded", "clusters", "clusters7", "negative-tail", "positive-tail"])
def test_constructed_spectrum_against_mpmath(lam):
    """the float64 matrix has the stated eigenvalues to its own rounding, u ||A||_F (Weyl), the long-double construction adding 2^-5 of that"""
    mpmath = pytest.importorskip("mpmath")
    A = R.from_spectrum(lam, 7)
    assert np.array_equal(A, A.T)
    with mpmath.workdps(40):
        ev = sorted(mpmath.eigsy(mpmath.matrix(A.tolist()), eigvals_only=True), reverse=True)
        want = sorted((mpmath.mpf(float(x)) for x in lam), reverse=True)
        worst = max(abs(a - b) for a, b in zip(ev, want))
        assert worst <= (1 + 2.0 ** -5) * R.U * mpmath.mpf(float(R.fro(A)))


def test_long_double_checks_against_plain_longdouble():
    rng = np.random.default_rng(11)
    for m, k in [(1, 1), (7, 5), (130, 257)]:
        A = rng.normal(size=(m, k)) * np.logspace(0, -14, m)[:, None]
        B = rng.normal(size=(k, m)) * np.logspace(0, 9, m)[None, :]
        ref = A.astype(LD) @ B.astype(LD)
        scale = np.abs(A).max(axis=1)[:, None] * np.abs(B).max(axis=0)[None, :]
        assert np.all(np.abs(R.matmul_ld(A, B) - ref) <= 2.0 ** -60 * k * scale)
    S = R.family("indefinite", 64)[0]
    val, V, _ = R.jacobi(S)
    Sl, Vl = S.astype(LD), V.astype(LD)
    r_plain = float(R.fro_ld(Sl @ Vl - Vl * val.astype(LD)[None, :]) / R.fro_ld(Sl))
    o_plain = float(R.fro_ld(Vl.T @ Vl - np.eye(64, dtype=LD)))
    assert abs(R.resid(S, val, V) - r_plain) <= 1e-3 * r_plain and abs(R.orth(V) - o_plain) <= 1e-3 * o_plain
    for s in (-1000, 1000):                                             # the same figure at the ends of the range, nothing overflows
        assert abs(R.resid(np.ldexp(S, s), np.ldexp(val, s), V) - r_plain) <= 1e-3 * r_plain
    junk = np.triu(np.full((64, 64), np.nan), 1)                        # only the lower triangle is read
    assert R.resid(S + junk, val, V) == R.resid(S, val, V)


@pytest.mark.parametrize("name,m", CASES, ids=["%s-%d" % c for c in CASES])
def test_model_is_inside_every_bound(name, m):
    A, lam, val, V, c = model(name, m)
    print("%s m = %d: %d sweeps, resid %.3g of %.3g, orth %.3g of %.3g, eig %s of %.3g" % (name, m, c["sweeps"], c["resid"], c["b"]["resid"], c["orth"],
                                                                                          c["b"]["orth"], c["eig"], c["b"]["eig"]))
    assert R.analytic_failures(c, val) == []
    assert c["sweeps"] <= 19                                            # graded and clustered spectra take the most
    if name in ("diagonal", "zero", "nearly-diagonal"):
        assert R.exact_failures(A, val, V, c["sweeps"]) == []


def test_sharpness_of_the_analytic_bounds_and_the_model_comparison():
    for name in ("psd", "clusters"):
        A, lam, val, V, good = model(name, 129)
        _, _, v, _, c = run(name, 129, cs32=True)
        assert {"resid", "orth"} <= set(R.analytic_failures(c, v)) and ("eig" in R.analytic_failures(c, v)) == (lam is not None)
        assert {"resid", "orth"} <= set(R.model_failures(c, good, 129))
        _, _, v, _, c = run(name, 129, skip_pair=True)
        assert c["sweeps"] == R.MAX_SWEEPS and "sweeps" in R.analytic_failures(c, v) and "sweeps" in R.model_failures(c, good, 129)
        _, _, v, _, c = run(name, 129, sort="ascending")
        assert "order" in R.analytic_failures(c, v)
        _, _, v, _, c = run(name, 129, drop_v_once=True)
        assert "resid" in R.model_failures(c, good, 129)
        assert R.model_failures(good, good, 129) == []
    _, _, _, _, good = model("graded", 129)
    _, _, _, _, c = run("graded", 129, stop_rel=1e-12)
    assert c["sweeps"] < good["sweeps"] and R.model_failures(c, good, 129) == ["resid"]
    _, _, _, _, good = model("clusters", 129)
    _, _, _, _, c = run("clusters", 129, offnorm="cancel")             # sum of squares minus the diagonal's: stops early on an indefinite input
    assert c["sweeps"] < good["sweeps"] and R.model_failures(c, good, 129) == ["resid"] and c["resid"] > 1e-10


def test_sharpness_of_the_exact_cases():
    for name, m in (("diagonal", 129), ("nearly-diagonal", 2)):
        A, lam = R.family(name, m)
        assert R.exact_failures(A, *R.jacobi(A)) == []
        assert {"values", "vectors"} <= set(R.exact_failures(A, *R.jacobi(A, sort="ascending")))
    A, _ = R.family("diagonal", 129)
    assert R.exact_failures(A, *R.jacobi(A, sort="unstable")) == ["vectors"]   # the tied values are the same bits, their columns are not
    val, V, sweeps = R.jacobi(A)
    assert R.exact_failures(A, val, V, sweeps + 1) == ["sweeps"]


def test_scale_and_the_range_bug_of_the_unscaled_sweeps():
    """2^s A0: the model with the scaling returns the same vectors and 2^s times the values at every s; without it (the code before the fix)
    it is right at 2^+-300, returns the diagonal after 0 sweeps at 2^-560, stops a sweep early at 2^-520 and refuses 2^+520"""
    A0 = R.scale_base()
    val0, V0, s0 = R.jacobi(A0)
    c0 = R.check_decomposition(A0, None, val0, V0, s0)
    assert R.analytic_failures(c0, val0) == []
    for s in (-1000, -560, -520, -300, 300, 520, 1000):
        A = np.ldexp(A0, s)
        assert np.array_equal(np.ldexp(A, -s), A0)
        val, V, sw = R.jacobi(A)
        assert sw == s0 and np.array_equal(val, np.ldexp(val0, s)) and np.array_equal(V, V0)
    for s in (-300, 300):
        val, V, sw = R.jacobi(np.ldexp(A0, s), scale=False)
        assert sw == s0 and np.array_equal(val, np.ldexp(val0, s)) and np.array_equal(V, V0)
    val, V, sw = R.jacobi(np.ldexp(A0, -560), scale=False)
    assert sw == 0 and np.array_equal(val, np.sort(np.diag(np.ldexp(A0, -560)))[::-1])
    A = np.ldexp(A0, -520)
    val, V, sw = R.jacobi(A, scale=False)
    c = R.check_decomposition(A, None, val, V, sw)
    assert sw == s0 - 1 and c["resid"] > 1e-10 and "resid" in R.model_failures(c, c0, 64)
    with pytest.raises(ValueError, match="non-finite"):
        R.jacobi(np.ldexp(A0, 520), scale=False)


def test_factor_bounds_on_the_model():
    """the eigen branch of mvn_factor from the model's decomposition, L = V sqrt(max(val, 0)): inside both bounds with the negative tail
    and with the positive one; outside with c and s in float32"""
    for m, tail in [(129, -1e-9), (257, -1e-9), (129, 1e-13)]:
        lam = R.mvn_spectrum(m, tail)
        assert np.sqrt((lam ** 2).sum()) > 2 * lam[0]
        A = R.from_spectrum(lam, 96000 + m)
        for kw, ok in ((dict(), True), (dict(cs32=True), False)):
            val, V, sweeps = R.jacobi(A, **kw)
            f = R.factor_eigen_figures(A, lam, V * np.sqrt(np.maximum(val, 0.0))[None, :], sweeps)
            print("m = %d tail %g %s: |L L^T - A| %.3g of %.3g, columns %.3g of %.3g" % (m, tail, kw, f["llt"], f["llt_bound"], f["cols"], f["cols_bound"]))
            assert (f["llt"] <= f["llt_bound"] and f["cols"] <= f["cols_bound"]) == ok
            assert ok or (f["llt"] > f["llt_bound"] and f["cols"] > f["cols_bound"])


def test_product_bounds_hold_for_float64_and_fail_for_float32():
    rng = np.random.default_rng(12)
    m, nd = 257, 9
    B = rng.normal(size=(m, m))
    A = B @ B.T + m * np.eye(m)
    L = np.linalg.cholesky(A)
    assert P.omega_chol(A, L) <= R.gamma(m + 1)
    L2 = L.copy()
    L2[200, 100] *= 1.0 + 1e-12
    assert P.omega_chol(A, L2) > R.gamma(m + 1)
    mean, Z = rng.normal(size=m), rng.normal(size=(m, nd))
    for lower, Lf in ((True, L), (False, B)):
        out = mean[:, None] + Lf @ Z
        assert R.affine_fraction(out, mean, Lf, Z, lower) <= 1.0
        out32 = mean[:, None] + Lf.astype(np.float32).astype(np.float64) @ Z
        assert R.affine_fraction(out32, mean, Lf, Z, lower) > 1.0
    assert R.affine_fraction(np.array([[1.5]]), [1.5], [[0.0]], [[3.0]], False) == 0.0
