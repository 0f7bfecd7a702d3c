"""Reference of the iterative exact GPR (gprc_igpr_*, gprc_dev_pivoted_cholesky, IterativeGPR) for the tests (tests/test_igpr_cpu.py,
tests/test_gpu_igpr.py): a numpy model of exactly the device's algorithm -- the partial pivoted Cholesky, the preconditioner
P^-1 = (I - Q Q^T) / noise and the batched preconditioned conjugate gradients with per-column freezing -- and the checks with their
derived bounds, written once: the CPU tests run them on the model's output, the GPU tests on the device's.  No GPU, no torch.

    K_y = K + noise I,  noise = paths_ref.NOISE = 0.1,  problems: paths_ref.problem(index) of the eight paths_ref.CASES
    u = 2^-53,  gamma_k = k u / (1 - k u),  kappa and lambda_min of K_y from numpy's eigvalsh,  longdouble Cholesky for x_ref

Bounds (all derived, none from what the code under test gives):
  pivoted Cholesky, r steps
    interpolation  |(L L^T)[:, piv] - K[:, piv]| <= gamma_{r+2}: an entry is a sum of at most r products whose partial sums stay within
                   1 in absolute value (Cauchy-Schwarz on rows of L, |row|^2 <= k(x, x) = 1), one division and one kernel value.
    greedy         with the device's pivot order replayed in numpy, each pivot's residual diagonal is within 16 (r + 2) u of the replay's
                   maximum: both sides carry at most r + 2 roundings of terms <= 1 and a few ulps of the kernel value.
    stop           after an early stop every remaining residual diagonal is <= n 2^-52 + 16 (r + 2) u.
  solve, tolerance tol on the recurrence residual
    true residual  |b - K_y x| / |b| <= 2 tol (the recurrence stops at tol; the true residual sits at 1.0e-10 in the model)
    solution       |x - x_ref| / |x_ref| <= kappa (that residual) + kappa n u
    report         the reported true residual is within a factor 2 of the test's own wherever the latter exceeds 100 kappa u
  predict          |mean_i - ref_i| <= |k*_i| |r| / lambda_min + gamma_{n+1} (|K*| |alpha|)_i,   r = y - K_y alpha (the test's own)
                   |var_i - ref_i|  <= |k*_i|^2 2 tol / lambda_min + gamma_{n+1} |k*_i|^2 / lambda_min
  paths            |U - U_ref|_F / |U_ref|_F <= kappa 2 tol + kappa n u
"""
import functools

import numpy as np

import paths_ref as R
from kernel_ref import pairwise
from pred_grad_ref import chol, solve_lower

LD = np.longdouble
NOISE = R.NOISE
CG_TOL = 1e-10
RANKS = (0, 32)
U64 = 2.0 ** -53


def gamma(k):
    return k * U64 / (1.0 - k * U64)


@functools.lru_cache(maxsize=None)
def reference(index):
    """problem `index` with what every check needs, computed once and shared; the arrays are never written to"""
    name, par, d, n, ns, D, S = R.CASES[index]
    X, y, Xs, nu, phase, W, E = R.problem(index)
    Kld = pairwise(name, par, X, X, LD)[0]
    Kyld = Kld + LD(NOISE) * np.eye(n, dtype=LD)
    K = Kld.astype(np.float64)
    lam = np.linalg.eigvalsh(K + NOISE * np.eye(n))
    out = dict(index=index, name=name, par=par, d=d, n=n, X=X, y=y, Xs=Xs, nu=nu, phase=phase, W=W, E=E, K=K, Kld=Kld, Kyld=Kyld, Lld=chol(Kyld),
               kappa=float(lam[-1] / lam[0]), lam_min=float(lam[0]))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def solve_ld(ref, B):
    """K_y^-1 B in longdouble"""
    B = np.asarray(B, dtype=LD).reshape(ref["n"], -1)
    return solve_lower(ref["Lld"], solve_lower(ref["Lld"], B), transpose=True)


def solve_rhs(ref):
    """B = [y, E[:, :4]]"""
    return np.asfortranarray(np.column_stack([ref["y"], ref["E"][:, :4]]))


# ---- the numpy model of the device's algorithm ------------------------------------------------------------------------------------------
def pivoted_cholesky(K, r, forced=None):
    """(L n x r, piv, rank, dg): the partial pivoted Cholesky of K (unit diagonal) as gprc_dev_pivoted_cholesky defines it.  forced: a pivot
    order to replay instead of the arg-max; then also the list of (dg[pivot], max dg) seen at each step.  dg: the residual diagonal of the
    points not chosen at the end, -1 at the chosen ones."""
    n = K.shape[0]
    L = np.zeros((n, r))
    piv = np.full(r, -1, dtype=np.int64)
    dg = np.ones(n)
    seen = []
    rank = r
    for j in range(r):
        p = int(np.argmax(dg))                        # the lowest index among the maxima; the chosen points hold -1
        if forced is not None:
            if forced[j] < 0:
                rank = j
                break
            seen.append((dg[forced[j]], dg[p]))
            p = int(forced[j])
        elif dg[p] <= n * 2.0 ** -52:
            rank = j
            break
        piv[j] = p
        free = dg >= 0
        L[p, j] = np.sqrt(dg[p])
        free[p] = False
        acc = K[free, p].copy()
        for t in range(j):
            acc -= L[free, t] * L[p, t]
        L[free, j] = acc / L[p, j]
        dg[free] = np.maximum(dg[free] - L[free, j] ** 2, 0.0)
        dg[p] = -1.0
    return (L, piv, rank, dg) if forced is None else (L, piv, rank, dg, seen)


def preconditioner(L, noise):
    """Q with P^-1 = (I - Q Q^T) / noise for P = L L^T + noise I: Q = L C^-T, C C^T = noise I + L^T L"""
    C = np.linalg.cholesky(noise * np.eye(L.shape[1]) + L.T @ L)
    return np.linalg.solve(C, L.T).T


def pcg(K, noise, B, tol, max_iter=1000, Q=None):
    """(X, iterations, recurrence |r| / |b|, true |b - K_y x| / |b|) per column: the batched loop with per-column scalars and freezing"""
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
    rr = bb.copy()
    iters = np.zeros(S, dtype=int)
    it = 0
    while active.any() and it < max_iter:
        AP = K @ P + noise * P
        pap = (P * AP).sum(0)
        assert (pap[active] > 0).all() and np.isfinite(pap[active]).all()
        with np.errstate(divide="ignore", invalid="ignore"):
            alpha = np.where(active, rz / pap, 0.0)
        X = np.where(active[None, :], X + alpha * P, X)
        Rm = np.where(active[None, :], Rm - alpha * AP, Rm)
        rr = np.where(active, (Rm * Rm).sum(0), rr)
        it += 1
        iters[active] = it
        active = active & ~(rr <= thr2)
        Z = prec(Rm)
        rz_new = (Rm * Z).sum(0)
        with np.errstate(divide="ignore", invalid="ignore"):
            beta = np.where(active, rz_new / rz, 0.0)
        P = np.where(active[None, :], Z + beta * P, P)
        rz = np.where(active, rz_new, rz)
    with np.errstate(divide="ignore", invalid="ignore"):
        T = B - (K @ X + noise * X)
        rec = np.where(bb > 0, np.sqrt(rr / bb), 0.0)
        true = np.where(bb > 0, np.sqrt((T * T).sum(0) / bb), 0.0)
    return X, iters, rec, true, not active.any()


def model_preconditioner(ref, rank):
    if rank == 0:
        return None
    L = pivoted_cholesky(ref["K"], min(rank, ref["n"]))[0]
    return preconditioner(L, NOISE)


# ---- the checks, for the model's output and for the device's ------------------------------------------------------------------------------
def check_pivoted_cholesky(ref, r, L, piv, rank):
    """asserts the interpolation, the greedy rule, the zero rows and, after an early stop, the remaining diagonal; returns the figures"""
    n, K = ref["n"], ref["K"]
    L, piv = np.asarray(L), np.asarray(piv)
    assert L.shape == (n, r) and piv.shape == (r,) and 1 <= rank <= r
    used = piv[:rank]
    assert (used >= 0).all() and (used < n).all() and len(set(used.tolist())) == rank
    assert (piv[rank:] == -1).all() and not L[:, rank:].any()                 # from the rank on: documented as zero columns, pivots -1
    Lr = L[:, :rank].astype(LD)
    interp = float(np.abs(Lr @ Lr[used].T - ref["Kld"][:, used]).max())
    assert interp <= gamma(r + 2), interp
    for j in range(1, rank):                                                  # the rows of the earlier pivots are exact zeros
        assert not L[used[:j], j].any()
    _, _, _, dg, seen = pivoted_cholesky(K, r, forced=piv)
    slack = 16.0 * (r + 2) * U64
    greedy = max(float(top - own) for own, top in seen)
    assert greedy <= slack, greedy
    left = float(dg.max()) if rank < r else None
    if rank < r:
        assert left <= n * 2.0 ** -52 + slack, left
    return dict(interpolation=interp, bound=gamma(r + 2), greedy=greedy, slack=slack, remaining=left)


def check_solve(ref, B, X, reported, tol=CG_TOL):
    """asserts the three solve bounds per column; returns the worst figures.  A zero column must come back as zeros."""
    n, kappa = ref["n"], ref["kappa"]
    B = np.asarray(B, dtype=np.float64).reshape(n, -1)
    X = np.asarray(X, dtype=np.float64).reshape(n, -1)
    Xref = solve_ld(ref, B)
    worst = dict(true=0.0, err=0.0, err_bound_ratio=0.0, report_ratio=1.0)
    for s in range(B.shape[1]):
        bn = float(np.linalg.norm(B[:, s]))
        if bn == 0.0:
            assert not X[:, s].any()
            continue
        own = float(np.linalg.norm(B[:, s].astype(LD) - ref["Kyld"] @ X[:, s].astype(LD)) / bn)
        assert own <= 2.0 * tol, (s, own)
        err = float(np.linalg.norm(X[:, s].astype(LD) - Xref[:, s]) / np.linalg.norm(Xref[:, s]))
        bound = kappa * own + kappa * n * U64
        assert err <= bound, (s, err, bound)
        worst["true"], worst["err"] = max(worst["true"], own), max(worst["err"], err)
        worst["err_bound_ratio"] = max(worst["err_bound_ratio"], err / bound)
        if reported is not None and own > 100.0 * kappa * U64:
            ratio = float(reported[s]) / own
            assert 0.5 <= ratio <= 2.0, (s, reported[s], own)
            worst["report_ratio"] = max(worst["report_ratio"], ratio, 1.0 / ratio)
    return worst


def check_predict(ref, alpha, mean, var, tol=CG_TOL):
    """asserts the mean's and the variance's bounds at the case's own test points; var may be None"""
    n, lam = ref["n"], ref["lam_min"]
    ks = pairwise(ref["name"], ref["par"], ref["Xs"], ref["X"], LD)[0]        # n* x n
    aref = solve_ld(ref, ref["y"])[:, 0]
    r = np.asarray(ref["y"], dtype=LD) - ref["Kyld"] @ np.asarray(alpha, dtype=LD)
    knorm = np.sqrt((ks * ks).sum(1)).astype(np.float64)
    mbound = knorm * float(np.linalg.norm(r)) / lam + gamma(n + 1) * (np.abs(ks).astype(np.float64) @ np.abs(alpha))
    mratio = float((np.abs(np.asarray(mean, dtype=LD) - ks @ aref).astype(np.float64) / mbound).max())
    assert mratio <= 1.0, mratio
    vratio = None
    if var is not None:
        v = solve_lower(ref["Lld"], ks.T)
        vref = LD(1) - (v * v).sum(0)
        vbound = knorm ** 2 * 2.0 * tol / lam + gamma(n + 1) * knorm ** 2 / lam
        vratio = float((np.abs(np.asarray(var, dtype=LD) - vref).astype(np.float64) / vbound).max())
        assert vratio <= 1.0, vratio
    return dict(mean_ratio=mratio, var_ratio=vratio)


def check_weights(ref, U, tol=CG_TOL):
    """|U - U_ref|_F / |U_ref|_F <= kappa 2 tol + kappa n u against paths_ref.paths"""
    Uref = R.paths(ref["name"], ref["par"], ref["X"], ref["y"], NOISE, ref["nu"], ref["phase"], ref["W"], ref["E"], ref["Xs"])[1]
    err = float(np.linalg.norm(U - Uref) / np.linalg.norm(Uref))
    bound = ref["kappa"] * 2.0 * tol + ref["kappa"] * ref["n"] * U64
    assert err <= bound, (err, bound)
    return dict(err=err, bound=bound)
