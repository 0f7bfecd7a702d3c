"""Model, checks, bounds and inputs for the sampling layer's eigensolver: the kernels of kernels_eig.hip behind gprc_sym_eigen and the eigen
branch of gprc_mvn_factor, with their host driver sym_eigen_dev (gprc_model.hip).  Helpers of tests/test_eig_cpu.py and tests/test_gpu_eig.py.
numpy only: no torch, no GPU.

Model.  jacobi() is the device algorithm in float64 numpy, operation by operation:
    * W = 2^-e sym(lower triangle of A), e = ilogb(max |A|) clamped to [-1022, 1022], V = I; the values are scaled back by 2^e;
    * the round-robin schedule of jacobi_pair on mm = m rounded up to even players, the dummy player m of an odd m sitting out;
    * per round the angles of all pairs from the W of the round's start -- tau = (w_qq - w_pp) / (2 w_pq) with w_pq = W[p, q], p < q,
      t = sign(tau) / (|tau| + sqrt(1 + tau^2)), c = 1 / sqrt(1 + t^2), s = t c; c = 1, s = 0 where w_pq == 0 -- then the columns of W and V,
      then the rows of W, a pair with s == 0 skipped in both;
    * the stop rule before every sweep: off2 <= rel^2 (off2 + dg2), rel = max(1e-15, m 2^-52), at most 40 sweeps; off2 is the sum over the
      columns of the float64 sums of the squared entries OFF the diagonal (the diagonal is left out of the sum, not subtracted from it: the
      subtraction cancels, see `offnorm="cancel"`), dg2 the sum of the squared diagonal, both accumulated in longdouble as on the host;
    * the stable sort that makes the values decreasing, ties in index order.
It differs from the device in what a compiler and a launch may choose: fused multiply-adds, and the order of the sum inside a column of the
off-norm.  Either changes which roundings occur, not how many.  The keyword arguments switch on the deliberately wrong variants with which
tests/test_eig_cpu.py shows that each assertion of the GPU test can fail.

Checks.  resid(A, val, V) = ||S V - V diag(val)||_F / ||S||_F, S the symmetric matrix of A's lower triangle, and orth(V) = ||V^T V - I||_F.
Both are scale free, so S and val are first divided by the power of two of max |S| (exact) and inputs of 2^-1000 or 2^+1000 neither
underflow nor overflow in the check itself.  The products come from matmul_ld: every factor is cut into slices of 20 bits, the slice
products are exact in float64 (integers below 2^52 for m <= 4096), and they are added in longdouble, as are the norms.  What is dropped is
below 2^-60 m of the row's largest entry times the column's; tests/test_eig_cpu.py holds it against the plain longdouble product.

Bounds, u = 2^-53, S = sweeps taken, mm - 1 rounds per sweep.  Write J for the exact rotation of the COMPUTED t: c = 1 / sqrt(1 + t^2), s = t c.
Whatever the error of t, J is orthogonal; an inexact angle leaves w_pq not quite zero, which the stop rule measures.
    gamma     the computed c carries 4 roundings (t t, 1 +, sqrt, 1 /), s one more; an output c a - s b has two products and one sum, so
              |fl(c a - s b) - (c a - s b)| <= (6 |c a| + 7 |s b|) u <= 7 u |(a, b)|_2 since c^2 + s^2 = 1; the same for s a + c b, so applying
              one rotation to a pair of entries x costs |fl(J x) - J x|_2 <= 7 sqrt(2) u |x|_2 <= GAMMA |x|_2, GAMMA = 10 u.  A fused
              multiply-add drops a rounding and never adds one.
    rot_w     a round applies disjoint rotations to all columns and then to all rows of W: 2 GAMMA ||W||_F.  After S sweeps the device's W is
              Q^T A Q + E with Q orthogonal and ||E||_F <= rot_w ||A||_F, rot_w = 2 S (mm - 1) GAMMA (first order: rot_w^2 < 1e-18 here).
    rot_v     V takes the column pass only: V = Q + F, ||F||_F <= S (mm - 1) GAMMA sqrt(m).
    stop      ||off(W)||_F <= rel ||W||_F <= rel (1 + rot_w) ||A||_F when the loop ended below its cap.
    eig       sorted diag(W) against the eigenvalues of the A that was handed in: Weyl on diag(W) = Q^T A Q + E - off(W), and u ||A||_F for the
              rounding of a constructed A = Q diag(lambda) Q^T to float64:
                  |val_k - lambda_k| <= (stop + rot_w + u) ||A||_F.
              (With Hoffman-Wielandt the same right-hand side bounds the 2-norm of the whole vector of differences.)
    resid     A V - V D = Q (off(W) - E) + (A F - F D), and ||A F - F D||_F <= 2 ||A||_2 ||F||_F <= 2 ||A||_F ||F||_F:
                  resid <= stop + rot_w + 2 rot_v.
              The sketch these tests were planned from, rel + 2 S (mm - 1) GAMMA, is the first two terms: it leaves out that the vectors
              themselves are inexact, and a rank-one A (ones(m, m)) has ||A||_2 = ||A||_F, so the third term cannot be dropped.
    orth      V^T V - I = Q^T F + F^T Q + F^T F:   orth <= 2 rot_v.   The sketch's S (mm - 1) GAMMA sqrt(m) is ||F||_F, which enters twice.
These grow linearly in the number of rotations, as worst-case bounds do, and sit two to three decades above what any correct
implementation shows.  The sharp assertions of the GPU test are therefore the ones against this model (tests/test_gpu_eig.py).
"""
import functools

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
EPS = 2.0 ** -52
GAMMA = 10.0 * U
MAX_SWEEPS = 40


def rel(m):
    return max(1e-15, m * EPS)


def gamma(k, u=U):
    return k * u / (1.0 - k * u)


# ---- the schedule ------------------------------------------------------------------------------------------------------------------
def jacobi_pair(m, mm, r, t):
    """(p, q, valid) of pair t in round r: jacobi_pair of kernels_eig.hip"""
    if t == 0:
        a, b = mm - 1, r
    else:
        a, b = (r + t) % (mm - 1), (r - t + (mm - 1)) % (mm - 1)
    p, q = min(a, b), max(a, b)
    return p, q, q < m


@functools.lru_cache(maxsize=None)
def round_pairs(m, r):
    """index arrays (P, Q) of the valid pairs of round r, in the order of t"""
    mm = m + (m & 1)
    pq = [jacobi_pair(m, mm, r, t) for t in range(mm // 2)]
    P = np.array([p for p, q, ok in pq if ok], dtype=np.intp)
    Q = np.array([q for p, q, ok in pq if ok], dtype=np.intp)
    return P, Q


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def sym_lower(A):
    A = np.asarray(A, dtype=np.float64)
    return np.tril(A) + np.tril(A, -1).T


def scale_exponent(S):
    amax = float(np.abs(S).max()) if S.size else 0.0
    if not amax > 0.0:
        return 0
    return int(min(max(np.frexp(amax)[1] - 1, -1022), 1022))


def offnorm2(W, how="exclude"):
    """(off2, dg2) in longdouble from per-column float64 sums"""
    d = np.diag(W).copy()
    sq = W * W
    if how == "exclude":
        sq[np.diag_indices_from(sq)] = 0.0
        cols = sq.sum(axis=0)
    else:                                                    # the mistake: all squares, minus the diagonal's
        cols = sq.sum(axis=0) - d * d
    off2 = LD(0)
    dg2 = LD(0)
    for j in range(W.shape[0]):
        off2 += LD(cols[j])
        dg2 += LD(d[j]) * LD(d[j])
    return off2, dg2


def jacobi(A, *, scale=True, stop_rel=None, cs32=False, drop_v_once=False, skip_pair=False, sort="stable-decreasing", offnorm="exclude"):
    """(values, vectors, sweeps) of the device algorithm on the lower triangle of A.  The keywords are the wrong variants:
    scale=False          the sweeps run on A itself (the code before the range fix)
    stop_rel=1e-12       a looser stop rule
    cs32                 c and s rounded to float32
    drop_v_once          V is left unrotated for the first rotated pair of the first round
    skip_pair            pair t = 1 of every round is skipped
    sort                 "ascending", or "unstable": decreasing with ties in reverse index order
    offnorm="cancel"     off2 as the sum of all squares minus the diagonal's"""
    S = sym_lower(A)
    m = S.shape[0]
    if not np.isfinite(S).all():
        raise ValueError("eigen: matrix has non-finite entries")
    e = scale_exponent(S) if scale else 0
    W = np.ldexp(S, -e)
    V = np.eye(m)
    mm = m + (m & 1)
    r_stop = LD(rel(m) if stop_rel is None else stop_rel)
    sweeps = 0
    dropped = False
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        while True:
            off2, dg2 = offnorm2(W, offnorm)
            if not np.isfinite(np.float64(off2 + dg2)) and not scale:
                raise ValueError("eigen: matrix has non-finite entries")
            if off2 <= r_stop * r_stop * (off2 + dg2) or sweeps >= MAX_SWEEPS:
                break
            for r in range(mm - 1 if m > 1 else 0):
                P, Q = round_pairs(m, r)
                apq = W[P, Q]
                nz = apq != 0.0
                tau = (W[Q, Q] - W[P, P]) / (2.0 * np.where(nz, apq, 1.0))
                tt = np.where(tau >= 0.0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
                c = 1.0 / np.sqrt(1.0 + tt * tt)
                s = tt * c
                c, s = np.where(nz, c, 1.0), np.where(nz, s, 0.0)
                if cs32:
                    c, s = c.astype(np.float32).astype(np.float64), s.astype(np.float32).astype(np.float64)
                go = s != 0.0
                if skip_pair and go.size > 1:
                    go[1] = False
                P, Q, c, s = P[go], Q[go], c[go], s[go]
                a, b = W[:, P], W[:, Q]
                W[:, P], W[:, Q] = c * a - s * b, s * a + c * b
                vP, vQ, vc, vs = P, Q, c, s
                if drop_v_once and not dropped and P.size:
                    vP, vQ, vc, vs = P[1:], Q[1:], c[1:], s[1:]
                    dropped = True
                a, b = V[:, vP], V[:, vQ]
                V[:, vP], V[:, vQ] = vc * a - vs * b, vs * a + vc * b
                a, b = W[P, :], W[Q, :]
                W[P, :], W[Q, :] = c[:, None] * a - s[:, None] * b, s[:, None] * a + c[:, None] * b
            sweeps += 1
    values = np.ldexp(np.diag(W).copy(), e)
    if sort == "stable-decreasing":
        perm = np.argsort(-values, kind="stable")
    elif sort == "ascending":
        perm = np.argsort(values, kind="stable")
    else:
        perm = np.argsort(-values[::-1], kind="stable")
        perm = (m - 1 - perm)
    return values[perm], V[:, perm], sweeps


# ---- long-double checks ------------------------------------------------------------------------------------------------------------
_BETA, _NSL = 20, 4


def _slices(X, axis):
    """X = sum of _NSL float64 slices, each an integer of at most _BETA + 1 bits times a power of two of its row (axis 1) or column"""
    mx = np.abs(X).max(axis=axis, keepdims=True)
    e = np.where(mx > 0, np.frexp(mx)[1], 0)
    e = np.maximum(e, -900)                                  # a row this small contributes nothing that a bound here can see
    out, R = [], X.astype(np.float64, copy=True)
    for k in range(_NSL):
        sig = np.ldexp(0.75, e + 53 - _BETA * (k + 1))
        Sk = (R + sig) - sig
        out.append(Sk)
        R = R - Sk
    return out


def matmul_ld(A, B):
    """A @ B in longdouble for float64 A, B with entries of ordinary size (|.| between 2^-900 and 2^100), inner dimension <= 4096"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    assert A.shape[1] == B.shape[0] and A.shape[1] <= 4096
    sa, sb = _slices(A, 1), _slices(B, 0)
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=LD)
    for tot in range(2 * _NSL - 2, -1, -1):                  # smallest terms first
        if tot > _NSL:
            continue                                         # below 2^-100 of the leading product
        for i in range(_NSL):
            j = tot - i
            if 0 <= j < _NSL:
                acc += (sa[i] @ sb[j]).astype(LD)
    return acc


def fro_ld(X):
    X = np.asarray(X, dtype=LD)
    return np.sqrt((X * X).sum())


def resid(A, val, V):
    """||S V - V diag(val)||_F / ||S||_F, S = sym_lower(A); 0 for S = 0 and val = 0"""
    S = sym_lower(A)
    e = scale_exponent(S)
    Sn = np.ldexp(S, -e)
    vn = np.ldexp(np.asarray(val, dtype=LD), -e)
    R = matmul_ld(Sn, V) - np.asarray(V, dtype=LD) * vn[None, :]
    den = fro_ld(Sn)
    num = fro_ld(R)
    if den == 0:
        return 0.0 if num == 0 else np.inf
    return float(num / den)


def orth(V):
    V = np.asarray(V, dtype=np.float64)
    G = matmul_ld(V.T.copy(), V)
    G[np.diag_indices_from(G)] -= LD(1)
    return float(fro_ld(G))


def fro(A):
    """||A||_F as a longdouble"""
    return fro_ld(A)


# ---- bounds ------------------------------------------------------------------------------------------------------------------------
def bounds(m, sweeps):
    """dict of the docstring's bounds for a run of `sweeps` sweeps at size m; eig is in units of ||A||_F"""
    mm = m + (m & 1)
    rounds = sweeps * (mm - 1)
    rot_w = 2.0 * rounds * GAMMA
    rot_v = rounds * GAMMA * np.sqrt(m)
    stop = rel(m) * (1.0 + rot_w)
    return dict(stop=stop, rot_w=rot_w, rot_v=rot_v, resid=stop + rot_w + 2.0 * rot_v, orth=2.0 * rot_v, eig=stop + rot_w + U)


# ---- matrix families ---------------------------------------------------------------------------------------------------------------
def _rng(m, salt):
    return np.random.default_rng(90000 + 131 * salt + m)


def from_spectrum(lam, seed):
    """float64 rounding of Q diag(lam) Q^T built in longdouble, Q = H1 H2 a product of two Householder reflectors"""
    lam = np.asarray(lam, dtype=LD)
    m = lam.size
    rng = np.random.default_rng(seed)
    A = np.diag(lam)
    for _ in range(2):                                       # A <- H A H, H = I - 2 v v^T / (v^T v); H2 first, then H1
        v = rng.normal(size=m).astype(LD)
        v /= np.sqrt((v * v).sum())
        A = A - LD(2) * np.outer(v, v @ A)
        A = A - LD(2) * np.outer(A @ v, v)
    A = (A + A.T) / LD(2)
    return A.astype(np.float64)


def clusters_spectrum(m):
    k = [m - 3 * (m // 4), m // 4, m // 4, m // 4]
    return np.concatenate([np.full(k[0], 3.0), np.full(k[1], 1.0), np.full(k[2], 1.0 + 1e-9), np.full(k[3], -2.0)])


def mvn_spectrum(m, tail, ntail=4):
    """lambda_1 = 1 down to 1e-3 over m - ntail values, then ntail copies of `tail`: ||lambda||_2 > 2 lambda_1 from m = 60"""
    return np.concatenate([np.logspace(0.0, -3.0, m - ntail), np.full(ntail, float(tail))])


def diag_entries(m):
    base = np.array([0.5, -1.25, 3.0, 0.0, 3.0, -1.25, 7.0, 0.0, 0.5, 2.0 ** -30, -(2.0 ** 40), 3.0])
    return np.resize(base, m) if m > 0 else base[:0]


FAMILIES = ["psd", "indefinite", "rank6", "graded", "clusters", "ones", "diagonal", "zero", "scaled", "sqexp"]


@functools.lru_cache(maxsize=None)
def family(name, m):
    """(A, lam): the float64 matrix (read-only) and its eigenvalues in decreasing order where they are known, else None"""
    lam = None
    if name == "psd":
        B = _rng(m, 1).normal(size=(m, m))
        A = B @ B.T
    elif name == "indefinite":
        B = _rng(m, 2).normal(size=(m, m))
        A = B + B.T
    elif name == "rank6":
        B = _rng(m, 3).normal(size=(m, min(m, 6)))
        A = B @ B.T
    elif name == "graded":
        lam = np.logspace(0.0, -16.0, m)
        A = from_spectrum(lam, 94000 + m)
    elif name == "clusters":
        lam = clusters_spectrum(m)
        A = from_spectrum(lam, 95000 + m)
    elif name == "ones":
        A = np.ones((m, m))
        lam = np.concatenate([[float(m)], np.zeros(m - 1)])
    elif name == "diagonal":
        lam = diag_entries(m)
        A = np.diag(lam)
    elif name == "zero":
        A = np.zeros((m, m))
        lam = np.zeros(m)
    elif name == "scaled":
        B = _rng(m, 4).normal(size=(m, m))
        D = np.logspace(0.0, -12.0, m)
        A = D[:, None] * (B @ B.T + np.eye(m)) * D[None, :]
    elif name == "sqexp":
        x = np.linspace(0.0, 1.0, m)
        A = np.exp(-0.5 * ((x[:, None] - x[None, :]) / 0.3) ** 2)
    elif name == "nearly-diagonal":                          # m is ignored: [[1, .], [1e-160, 2]], the square of 1e-160 is 0
        A = np.array([[1.0, 5.0], [1e-160, 2.0]])
        lam = np.array([1.0, 2.0])
    else:
        raise KeyError(name)
    A = np.asfortranarray(sym_lower(A) if name != "nearly-diagonal" else A)
    A.setflags(write=False)
    if lam is not None:
        lam = np.sort(np.asarray(lam, dtype=np.float64))[::-1]
        lam.setflags(write=False)
    return A, lam


def scale_base():
    """A0 of the scale tests: 64 x 64 symmetric normal; 2^s A0 is exact in float64 for |s| <= 1000 (no entry of A0 is below 2^-20)"""
    A = np.array(family("indefinite", 64)[0])
    assert np.abs(A[A != 0]).min() > 2.0 ** -20
    return A


def check_decomposition(A, lam, val, V, sweeps):
    """the measured figures of one decomposition and their bounds: dict(resid, orth, eig (or None), b=bounds(...))"""
    m = A.shape[0]
    b = bounds(m, sweeps)
    out = dict(resid=resid(A, val, V), orth=orth(V), eig=None, b=b, sweeps=sweeps)
    if lam is not None:
        nrm = fro(sym_lower(A))
        d = np.abs(np.asarray(val, dtype=LD) - np.asarray(lam, dtype=LD)).max() if m else LD(0)
        out["eig"] = float(d / nrm) if nrm > 0 else float(d)
    return out


# ---- the assertions of tests/test_gpu_eig.py, as functions, so that tests/test_eig_cpu.py can show each of them failing ----------------
def analytic_failures(c, val):
    """names of the analytic assertions that a decomposition `c` (check_decomposition) with values `val` misses"""
    bad = []
    if not c["sweeps"] < MAX_SWEEPS:
        bad.append("sweeps")
    if not np.all(np.diff(val) <= 0):
        bad.append("order")
    if not c["resid"] <= c["b"]["resid"]:
        bad.append("resid")
    if not c["orth"] <= c["b"]["orth"]:
        bad.append("orth")
    if c["eig"] is not None and not c["eig"] <= c["b"]["eig"]:
        bad.append("eig")
    return bad


MODEL_FACTOR = 4.0


def model_failures(c, cm, m):
    """names of the assertions against the model's own figures `cm` that `c` misses: resid <= rel + 4 resid_model,
    orth <= 4 max(orth_model, m u), sweeps <= sweeps_model + 1"""
    bad = []
    if not c["resid"] <= rel(m) + MODEL_FACTOR * cm["resid"]:
        bad.append("resid")
    if not c["orth"] <= MODEL_FACTOR * max(cm["orth"], m * U):
        bad.append("orth")
    if not c["sweeps"] <= cm["sweeps"] + 1:
        bad.append("sweeps")
    return bad


def model_fractions(c, cm, m):
    return dict(resid=c["resid"] / (rel(m) + MODEL_FACTOR * cm["resid"]), orth=c["orth"] / (MODEL_FACTOR * max(cm["orth"], m * U)))


def exact_failures(A, val, V, sweeps):
    """an input whose off-diagonal squares are all zero: 0 sweeps, the sorted diagonal bit for bit, permutation columns, ties in index order"""
    d = np.diag(np.asarray(A)).copy()
    m = d.size
    perm = sorted(range(m), key=lambda k: -d[k])             # sorted() is stable
    P = np.zeros((m, m))
    P[perm, np.arange(m)] = 1.0
    bad = []
    if sweeps != 0:
        bad.append("sweeps")
    if not np.array_equal(np.asarray(val).view(np.int64), d[perm].view(np.int64)):
        bad.append("values")
    if not np.array_equal(V, P):
        bad.append("vectors")
    return bad


def affine_fraction(out, mean, L, Z, lower):
    """max |out - (mean + L Z)| / (gamma_{k+1} (|mean| + |L| |Z|)), k = i + 1 terms in row i of a lower-triangular L and m otherwise; the
    reference in longdouble from the float64 L; 0 / 0 counts as 0"""
    Ll, Zl, ml = np.asarray(L, dtype=LD), np.asarray(Z, dtype=LD), np.asarray(mean, dtype=LD)
    m = Ll.shape[0]
    ref = ml[:, None] + Ll @ Zl
    mag = np.abs(ml)[:, None] + np.abs(Ll) @ np.abs(Zl)
    k = (np.arange(m) + 1 if lower else np.full(m, m)).astype(np.float64)
    bound = np.asarray(gamma(k + 1.0))[:, None].astype(LD) * mag
    err = np.abs(np.asarray(out, dtype=LD) - ref)
    ok = bound > 0
    if np.any(~ok & (err > 0)):
        return np.inf
    return float((err[ok] / bound[ok]).max()) if ok.any() else 0.0


def factor_eigen_figures(A, lam, L, sweeps):
    """eigen branch of mvn_factor on a matrix of known spectrum `lam` (decreasing): the figures and the bounds of
        ||L L^T - A||_F <= 2 resid_bound ||A||_F + ||lam_-||_2      and      | |L[:, k]|^2 - max(lam_k, 0) | <= (resid_bound + u) ||A||_F.
    With L = V sqrt(D+): A - V D V^T = R V^T - A G, R the residual and G = V V^T - I, so ||A - V D V^T||_F <= (resid_bound + orth_bound) ||A||_F
    <= 2 resid_bound ||A||_F less (stop + rot_w) ||A||_F; what is clipped is ||val_-||_2 <= ||lam_-||_2 + (stop + rot_w + u) ||A||_F by
    Hoffman-Wielandt; the 3 u of sqrt, the scaling of a column and u of the excess are far inside the slack of ||A||_2 <= ||A||_F / 2
    (mvn_spectrum).  A column's squared norm is |v_k|^2 max(val_k, 0), and | |v_k|^2 - 1 | <= orth_bound."""
    m = A.shape[0]
    b = bounds(m, sweeps)
    nrm = fro(A)
    Ll = np.asarray(L, dtype=np.float64)
    D = matmul_ld(Ll, Ll.T.copy()) - np.asarray(A, dtype=LD)
    lam = np.asarray(lam, dtype=LD)
    neg = np.sqrt((np.minimum(lam, 0) ** 2).sum())
    cols = (np.asarray(Ll, dtype=LD) ** 2).sum(axis=0)
    return dict(llt=float(fro_ld(D)), llt_bound=float(2 * b["resid"] * nrm + neg),
                cols=float(np.abs(cols - np.maximum(lam, 0)).max()), cols_bound=float((b["resid"] + U) * nrm))
