"""Reference of the iterative GPR's stochastic log evidence and gradient (gprc_igpr_probes, gprc_igpr_logp_grad, gprc_dev_lowrank_grad,
IterativeGPR.logp_grad, fit.optimize_iterative) for the tests (tests/test_igpr_logp_cpu.py, tests/test_gpu_igpr_logp.py): a numpy model of
exactly the device's algorithm on top of igpr_ref's (its conjugate-gradient loop, here returning the coefficients), the dense values the
estimators are judged against, and the checks with their bounds, written once: the CPU tests run them on the model's output, the GPU
tests on the device's.  No GPU, no torch.

    K_y = K + noise I,  alpha = K_y^-1 y,  P = L L^T + noise I (rank 0: P = I),  M = P^-1/2 K_y P^-1/2,  sigma = sqrt(noise)
    z_s = L g1_s + sigma g2_s (rank 0: g2_s),  w_s = P^-1 z_s,  u_s = K_y^-1 z_s by the preconditioned loop
    T_s from the column's coefficients: T[0,0] = 1 / a_0, T[j,j] = 1 / a_j + b_{j-1} / a_{j-1}, T[j,j+1] = sqrt(b_j) / a_j
    q_s = (z_s^T w_s) e_1^T log(T_s) e_1;   logp = -1/2 y^T alpha - 1/2 (log det P + mean q) - n/2 log 2 pi;   se = 1/2 std(q, ddof=1) / sqrt(T)
    grad_k = sum_ij G_ij dK_ij / dtheta_k,  G = 1/2 alpha alpha^T - 1/(2T) sum_s u_s w_s^T;   d / d noise = 1/2 alpha^T alpha - 1/(2T) sum_s u_s^T w_s

Problems: paths_ref.problem(index) of the eight paths_ref.CASES at noise 0.1, ranks 0 and 32, as igpr_ref.  u = 2^-53, gamma_k = k u / (1 - k u).

Bounds (derived; none from what the code under test gives):
  quadrature     |sum v_1i^2 log lambda_i - eigh's| <= QL_C m u |T|_2 / lambda_min(T) + 8 m u max|log lambda|.  QL (and LAPACK's eigh) are
                 backward stable: each returns the exact pairs of T + E, |E|_2 <= c' m u |T|_2 with c' a modest constant; e_1^T log(T) e_1
                 moves by at most |log'| |E| <= |E|_2 / lambda_min (the Frechet derivative of log on the spectrum's hull).  QL_C = 32
                 covers both sides' c' (a few units each).  The second term is the rounding of the m-term sum itself, on both sides.
  contraction    |got_k - ref_k| <= gamma_{n + R + c} sum_ij (|A| |B|^T)_ij |dK_ij / dtheta_k|,  c = 3 d + 64: a pair's weight is a sum of R
                 products, the sum over pairs has depth <= n (lane chain, tree, partials), the integrand carries the distance's ~3 d
                 roundings (ARD scales each coordinate twice) and a transcendental chain of a few ulps whose amplification (the argument of
                 exp) the 64 covers wherever the term matters.  Reference: longdouble, integrands included.
  probes         |Z - (L g1 + sigma g2)| <= gamma_{r + 2} (|L| |g1| + sigma |g2|): one fma chain of r + 1 terms
  q_s            |q_s - z_s^T P^-1 log(K_y P^-1) z_s| <= Q_BOUND |P^-1/2 z_s|^2 max(1, max |log lambda(M)|), Q_BOUND = 1e-11.  The float64
                 numpy model's worst value in these units is Q_MODEL_WORST = 4.1e-14 (measured on the CPU, tol 1e-10, the eight cases, ranks
                 0 and 32, 63 probes; 7.1e-14 at tol 1e-6 on three cases; tests/test_igpr_logp_cpu.py asserts it within a factor 2; the
                 issue that set Q_BOUND counted 2.0e-13 and a factor 50); the factor covers a different order of summation inside the
                 n-term dot products, which perturbs every coefficient by about n u kappa.  max(1, .): rationalquadratic d = 1 at
                 rank 32 converges in one step with M = I to 3e-11, where max |log lambda| is itself ~ 1e-11.
  gradient       |got_k - ref_k| <= eps mean_s |u_s| |dK_k w_s| + eps |alpha| |dK_k alpha| + the contraction's bound,
                 eps = kappa 2 tol + kappa n u (igpr_ref's solution bound), ref with longdouble solves and the same Z; dK = I for the noise.
                 (The device's w = P^-1 z differs from the reference's by ~ kappa(P) r u <= 1e-11 relative, far inside eps.)
  value, se      equal to the stated formulas recomputed on the host from terms, alpha and log det P to VALUE_ULPS = 8 ulps of the
                 largest of the three summands
  statistics     |logp - exact| <= 4 se and every gradient entry within 4 of its standard errors for DRAW_SEED's normals (a condition on
                 the inputs: the CPU test asserts the model stays within 3 for that seed)
"""
import functools

import numpy as np

import igpr_ref as I
import paths_ref as R
from kernel_ref import is_ard, kernel_derivs, pairwise

LD = np.longdouble
NOISE = I.NOISE
U64 = I.U64
gamma = I.gamma
RANKS = I.RANKS
T_PROBES = 63
DRAW_SEED = 1            # default_rng(DRAW_SEED): G2 (n x T) first, then G1 (32 x T)
QL_C = 32.0
Q_BOUND = 1e-11
Q_MODEL_WORST = 4.1e-14  # the numpy model's worst |q_s - dense| in the bound's units, measured; asserted (x 2) by the CPU test
VALUE_ULPS = 8


def draws(index, T=T_PROBES, seed=DRAW_SEED, rank=32):
    """(G1 rank x T, G2 n x T) of case `index`"""
    n = R.CASES[index][3]
    rng = np.random.default_rng(seed)
    G2 = np.asfortranarray(rng.standard_normal((n, T)))
    G1 = np.asfortranarray(rng.standard_normal((rank, T)))
    return G1, G2


# ---- the numpy model of the device's algorithm ----------------------------------------------------------------------------------------------
def pcg_coeffs(K, noise, B, tol, max_iter=1000, Q=None):
    """igpr_ref.pcg's loop, also returning per column its coefficients: (X, iterations, [alpha_0 .. alpha_{m-1}], [beta_0 .. beta_{m-2}],
    converged)"""
    B = np.asarray(B, dtype=np.float64).reshape(K.shape[0], -1)
    S = B.shape[1]

    def prec(V):
        return V if Q is None else (V - Q @ (Q.T @ V)) / noise

    X, Rm = np.zeros_like(B), B.copy()
    bb = (B * B).sum(0)
    thr2 = tol * tol * bb
    active = ~(bb <= thr2)
    Z = prec(Rm)
    P = np.where(active[None, :], Z, 0.0)
    rz = (Rm * Z).sum(0)
    iters = np.zeros(S, dtype=int)
    al, be = [[] for _ in range(S)], [[] for _ in range(S)]
    it = 0
    while active.any() and it < max_iter:
        AP = K @ P + noise * P
        pap = (P * AP).sum(0)
        if not ((pap[active] > 0).all() and np.isfinite(pap[active]).all()):
            raise ArithmeticError("p^T K_y p is not finite or not positive")          # the device's GPRC_ERR_NOT_PD
        with np.errstate(divide="ignore", invalid="ignore"):
            alpha = np.where(active, rz / pap, 0.0)
        X = np.where(active[None, :], X + alpha * P, X)
        Rm = np.where(active[None, :], Rm - alpha * AP, Rm)
        rr = (Rm * Rm).sum(0)
        it += 1
        iters[active] = it
        for c in np.flatnonzero(active):
            al[c].append(alpha[c])
        active = active & ~(rr <= thr2)
        Z = prec(Rm)
        rz_new = (Rm * Z).sum(0)
        with np.errstate(divide="ignore", invalid="ignore"):
            beta = np.where(active, rz_new / rz, 0.0)
        for c in np.flatnonzero(active):
            be[c].append(beta[c])
        P = np.where(active[None, :], Z + beta * P, P)
        rz = np.where(active, rz_new, rz)
    return X, iters, al, be, not active.any()


def tridiagonal(al, be):
    """(diag m, off m - 1) of the Lanczos tridiagonal from m steps' coefficients"""
    al, be = np.asarray(al, dtype=float), np.asarray(be, dtype=float)
    if not ((al > 0).all() and (be >= 0).all()):
        raise ArithmeticError("conjugate-gradient coefficients out of range")
    m = al.size
    dg = 1.0 / al
    dg[1:] += be[:m - 1] / al[:m - 1]
    return dg, np.sqrt(be[:m - 1]) / al[:m - 1]


def log_quadrature(dg, off):
    """(e_1^T log(T) e_1 by numpy's eigh, lambda): the quadrature the host's implicit QL is judged against"""
    m = dg.size
    lam, V = np.linalg.eigh(np.diag(dg) + np.diag(off, 1) + np.diag(off, -1)) if m > 1 else (dg.copy(), np.ones((1, 1)))
    if not (np.isfinite(lam).all() and (lam > 0).all()):
        raise ArithmeticError("the tridiagonal is not positive definite")               # the device's GPRC_ERR_NOT_PD
    return float((V[0] ** 2 * np.log(lam)).sum()), lam


def quadrature_bound(dg, off):
    lam = log_quadrature(dg, off)[1]
    m = dg.size
    return QL_C * m * U64 * float(np.abs(lam).max()) / float(lam.min()) + 8.0 * m * U64 * float(np.abs(np.log(lam)).max())


def probes(L, noise, G1, G2):
    """Z as the device forms it; L None or with no columns: Z = G2"""
    if L is None or L.shape[1] == 0:
        return np.array(G2, dtype=float, order="F")
    return np.asfortranarray(L @ G1[:L.shape[1]] + np.sqrt(noise) * G2)


def logdet_p(L, noise, n):
    if L is None or L.shape[1] == 0:
        return 0.0
    C = np.linalg.cholesky(np.eye(L.shape[1]) + L.T @ L / noise)
    return n * np.log(noise) + 2.0 * float(np.log(np.diag(C)).sum())


def model_L(ref, rank):
    if rank == 0:
        return None
    L, _, reached, _ = I.pivoted_cholesky(ref["K"], min(rank, ref["n"]))
    return L[:, :reached]


def estimate(name, par, X, y, noise, rank, G1, G2, tol, max_iter=1000, K=None, L=None):
    """the whole algorithm in numpy for arbitrary parameters: dict(value, se, grad, terms, alpha, U, W, Z, L, logdet_p, iters, al, be (the
    coefficients per probe), converged).
    K, L: the kernel matrix and the preconditioner's factor when the caller has them (the cases' references), else formed here."""
    X = np.asarray(X, dtype=float)
    n = X.shape[1]
    if K is None:
        K = pairwise(name, par, X, X, np.float64)[0]
    if rank > 0 and L is None:
        L, _, reached, _ = I.pivoted_cholesky(K, min(rank, n))
        L = L[:, :reached]
    Q = None if L is None else I.preconditioner(L, noise)
    Z = probes(L, noise, G1, G2)
    T = Z.shape[1]
    W = Z if Q is None else (Z - Q @ (Q.T @ Z)) / noise
    alpha, _, _, _, ok_a = pcg_coeffs(K, noise, y, tol, max_iter, Q)
    alpha = alpha[:, 0]
    U, iters, al, be, ok_u = pcg_coeffs(K, noise, Z, tol, max_iter, Q)
    zw = (Z * W).sum(0)
    terms = np.array([zw[s] * log_quadrature(*tridiagonal(al[s], be[s]))[0] for s in range(T)])
    ldp = logdet_p(L, noise, n)
    value = -0.5 * float(y @ alpha) - 0.5 * (ldp + terms.mean()) - 0.5 * n * np.log(2.0 * np.pi)
    se = 0.5 * terms.std(ddof=1) / np.sqrt(T) if T > 1 else float("nan")
    grad = [0.5 * float(alpha @ dK @ alpha) - float((U * (dK @ W)).sum()) / (2.0 * T) for dK in kernel_derivs(name, par, X, K)]
    grad.append(0.5 * float(alpha @ alpha) - float((U * W).sum()) / (2.0 * T))
    return dict(value=value, se=se, grad=np.array(grad), terms=terms, alpha=alpha, U=U, W=W, Z=Z, L=L, logdet_p=ldp, iters=iters, al=al, be=be,
                converged=ok_a and ok_u)


# ---- dense values ------------------------------------------------------------------------------------------------------------------------------
def derivs_ld(name, par, X):
    """generator of dK / dtheta_k in longdouble, parameter order: kernel_ref.kernel_derivs' formulas with every intermediate in longdouble"""
    X = np.asarray(X, dtype=LD)
    d = X.shape[0]
    par = [LD(p) for p in par]
    sq = [np.subtract.outer(X[k], X[k]) ** 2 for k in range(d)]
    one, two = LD(1), LD(2)
    if name.startswith("matern") or name == "sqrexp_ard":
        ell = par if is_ard(name) else [par[0]] * d
        rho2 = sum(s / (l * l) for s, l in zip(sq, ell))
        if name == "sqrexp_ard":
            h = np.exp(-rho2 / two)
        else:
            a = np.sqrt((LD(3) if name.startswith("matern32") else LD(5)) * rho2)
            h = LD(3) * np.exp(-a) if name.startswith("matern32") else LD(5) / LD(3) * (one + a) * np.exp(-a)
        if is_ard(name):
            for s, l in zip(sq, ell):
                yield h * s / l ** 3
        else:
            yield h * sum(sq) / ell[0] ** 3
        return
    s = sum(sq)
    if name == "sqrexp":
        yield np.exp(-s / (two * par[0] ** 2)) * s / par[0] ** 3
    elif name == "gammaexp":
        l, g = par
        r = np.sqrt(s)
        u = (r / l) ** g
        K = np.exp(-u)
        yield K * g * u / l
        with np.errstate(divide="ignore", invalid="ignore"):
            t = u * np.log(r / l)
        t[r == 0] = 0
        yield -K * t
    elif name == "rationalquadratic":
        l, al = par
        x = s / (two * al * l * l)
        q = one + x
        K = np.exp(-al * np.log1p(x))
        yield K * s / (l ** 3 * q)
        yield K * (-np.log1p(x) + x / q)
    else:
        raise KeyError(name)


def contraction_reference(name, par, X, A, B):
    """(ref, bound) per parameter of sum_ij (A B^T)_ij dK_ij / dtheta_k in longdouble and the componentwise bound above"""
    d, n = np.asarray(X).shape
    Rk = np.asarray(A).shape[1]
    G = np.asarray(A, dtype=LD) @ np.asarray(B, dtype=LD).T
    mag = np.abs(np.asarray(A, dtype=LD)) @ np.abs(np.asarray(B, dtype=LD)).T
    ref, bound = [], []
    for dK in derivs_ld(name, par, X):
        ref.append((G * dK).sum())
        bound.append(float(gamma(n + Rk + 3 * d + 64) * (mag * np.abs(dK)).sum()))
    return ref, bound


def check_contraction(name, par, X, A, B, got):
    ref, bound = contraction_reference(name, par, X, A, B)
    worst = 0.0
    for k in range(len(ref)):
        err = float(abs(LD(got[k]) - ref[k]))
        assert err <= bound[k], (k, got[k], float(ref[k]), err, bound[k])
        if bound[k] > 0:
            worst = max(worst, err / bound[k])
    return worst


@functools.lru_cache(maxsize=None)
def dense(index, rank, L_key=None):
    """the dense side of (case, rank) with the model's own L: P's Cholesky factor, M's eigen-decomposition, log det P, the exact evidence and
    gradient; computed once, never written to.  L_key: None for the numpy model's L, else a key into DEVICE_L (the device's own factor)."""
    ref = I.reference(index)
    n, K = ref["n"], ref["K"]
    L = model_L(ref, rank) if L_key is None else DEVICE_L[L_key]
    Ky = K + NOISE * np.eye(n)
    Pm = np.eye(n) if L is None else L @ L.T + NOISE * np.eye(n)
    Lp = np.linalg.cholesky(Pm)
    half = np.linalg.solve(Lp, Ky)
    M = np.linalg.solve(Lp, half.T).T
    lam, V = np.linalg.eigh(0.5 * (M + M.T))
    alpha_ld = I.solve_ld(ref, ref["y"])[:, 0]
    logdet = 2.0 * float(np.log(np.diag(ref["Lld"])).sum())
    exact = float(-0.5 * (np.asarray(ref["y"], dtype=LD) @ alpha_ld) - 0.5 * logdet - 0.5 * n * np.log(2.0 * np.pi))
    out = dict(L=L, Lp=Lp, lam=lam, V=V, alpha_ld=alpha_ld, exact=exact, logdet=logdet, logdet_p=logdet_p(L, NOISE, n),
               dK=[np.asarray(d, dtype=float) for d in kernel_derivs(ref["name"], ref["par"], ref["X"], K)])
    return out


DEVICE_L = {}   # (index, rank) -> the device's own L, put there by the GPU tests before dense(index, rank, key)


def dense_terms(dn, Z):
    """(z^T P^-1 log(K_y P^-1) z per column, its unit |P^-1/2 z|^2 max(1, max |log lambda(M)|))"""
    v = np.linalg.solve(dn["Lp"], Z)
    c = dn["V"].T @ v
    q = (c * c * np.log(dn["lam"])[:, None]).sum(0)
    return q, (v * v).sum(0) * max(1.0, float(np.abs(np.log(dn["lam"])).max()))


def check_terms(dn, Z, terms):
    """asserts the q_s bound; returns the worst figure in the bound's units (so 1e-11 is the bound)"""
    q, unit = dense_terms(dn, Z)
    fig = np.abs(np.asarray(terms) - q) / unit
    assert (fig <= Q_BOUND).all(), (int(fig.argmax()), float(fig.max()))
    return float(fig.max())


def check_probes(L, noise, G1, G2, Z):
    if L is None or L.shape[1] == 0:
        assert np.array_equal(Z, G2)
        return 0.0
    r = L.shape[1]
    want = np.asarray(L, dtype=LD) @ np.asarray(G1[:r], dtype=LD) + np.sqrt(LD(noise)) * np.asarray(G2, dtype=LD)
    bound = gamma(r + 2) * (np.abs(L) @ np.abs(G1[:r]) + np.sqrt(noise) * np.abs(G2))
    ratio = float((np.abs(np.asarray(Z, dtype=LD) - want).astype(float) / bound).max())
    assert ratio <= 1.0, ratio
    return ratio


def check_gradient(ref, dn, Z, grad, tol):
    """asserts the gradient's bound against longdouble solves with the same Z; returns the worst error / bound"""
    n, kappa = ref["n"], ref["kappa"]
    T = Z.shape[1]
    Uld = I.solve_ld(ref, Z)
    Wm = np.linalg.solve(dn["Lp"].T, np.linalg.solve(dn["Lp"], Z))
    a = dn["alpha_ld"]
    eps = kappa * 2.0 * tol + kappa * n * U64
    A = np.column_stack([np.asarray(a, dtype=float), np.asarray(Uld, dtype=float)])
    B = np.column_stack([0.5 * np.asarray(a, dtype=float), -Wm / (2.0 * T)])
    mag = np.abs(A) @ np.abs(B).T
    worst = 0.0
    for k, dK in enumerate(dn["dK"] + [np.eye(n)]):
        dKw = dK @ Wm
        want = LD(0.5) * (a @ np.asarray(dK, dtype=LD) @ a) - (Uld * np.asarray(dKw, dtype=LD)).sum() / LD(2 * T)
        bound = (eps * float(np.mean(np.linalg.norm(np.asarray(Uld, dtype=float), axis=0) * np.linalg.norm(dKw, axis=0)))
                 + eps * float(np.linalg.norm(np.asarray(a, dtype=float)) * np.linalg.norm(dK @ np.asarray(a, dtype=float)))
                 + gamma(n + T + 1 + 3 * ref["d"] + 64) * float((mag * np.abs(dK)).sum()))
        err = float(abs(LD(grad[k]) - want))
        assert err <= bound, (k, grad[k], float(want), err, bound)
        worst = max(worst, err / bound)
    return worst


def check_value(y, alpha, logdet_p_value, terms, value, se):
    """the stated formulas from terms, alpha and log det P, to VALUE_ULPS ulps of the largest summand"""
    T, n = len(terms), len(y)
    parts = [-0.5 * float(np.asarray(y, dtype=LD) @ np.asarray(alpha, dtype=LD)), -0.5 * (logdet_p_value + float(np.mean(terms))),
             -0.5 * n * np.log(2.0 * np.pi)]
    slack = VALUE_ULPS * 2.0 * U64 * max(abs(p) for p in parts)
    # y^T alpha is the device's own n-term dot product: gamma_n |y|^T |alpha| / 2 on top
    slack += 0.5 * gamma(n) * float(np.abs(y) @ np.abs(alpha))
    assert abs(value - sum(parts)) <= slack, (value, sum(parts), slack)
    if T > 1:
        want = 0.5 * float(np.std(terms, ddof=1)) / np.sqrt(T)
        # the deviations q_s - mean cancel: the mean's rounding, T u max |q|, enters each of them
        slack_se = VALUE_ULPS * 2.0 * U64 * want + 0.5 * np.sqrt(T) * 2.0 * U64 * float(np.abs(terms).max())
        assert abs(se - want) <= slack_se, (se, want, slack_se)
    return abs(value - sum(parts))


def statistics(ref, dn, est_value, est_se, est_grad, U, W, exact=None):
    """(|logp - exact| / se, the worst gradient entry's |got - exact| / its standard error); exact: (value, gradient) from elsewhere (the
    library's exact evidence), else the dense inverse's; a gradient entry's standard error from the per-probe terms u_s^T dK w_s (numpy)"""
    n = ref["n"]
    T = U.shape[1]
    a = np.asarray(dn["alpha_ld"], dtype=float)
    Kinv = np.asarray(I.solve_ld(ref, np.eye(n)), dtype=float) if exact is None else None
    zv = abs(est_value - (dn["exact"] if exact is None else exact[0])) / est_se
    zg = 0.0
    for k, dK in enumerate(dn["dK"] + [np.eye(n)]):
        exact_k = 0.5 * float(a @ dK @ a) - 0.5 * float((Kinv * dK).sum()) if exact is None else float(exact[1][k])
        per = (U * (dK @ W)).sum(0)
        se = 0.5 * per.std(ddof=1) / np.sqrt(T)
        zg = max(zg, abs(est_grad[k] - exact_k) / se)
    return float(zv), float(zg)
