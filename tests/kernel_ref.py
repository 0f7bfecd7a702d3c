"""The per-kernel mathematics of the tests' numpy references, once: the eight kernels of fit.grad_dict (values, derivatives with respect to
the parameters and to a test point) and `linear`'s values for loo_ref, written from the formulas below and nothing else.  No GPU, no torch.
The structure around a kernel lives in the sibling modules and takes any name through this one: pred_grad_ref (prediction and its
gradients), ard_grad_ref (log marginal likelihood), gpc_grad_ref (Laplace evidence), loo_ref (leave-one-out).

With s = sum_k (x_k - y_k)^2, r = sqrt(s), and for ARD rho^2 = sum_k ((x_k - y_k) / l_k)^2:

    sqrexp (l)                    K = exp(-s / (2 l^2))                   dK/dl = K s / l^3                        h = K / l^2
    sqrexp_ard (l_1..l_d)         K = exp(-rho^2 / 2)                     dK/dl_k = K (x_k - y_k)^2 / l_k^3        h = K
    gammaexp (l, gamma)           K = exp(-u), u = (r / l)^gamma          dK/dl = K gamma u / l                    h = K gamma u / s;  0 at r = 0
                                                                          dK/dgamma = -K u log(r / l);  0 at r = 0
    rationalquadratic (l, alpha)  K = q^-alpha, q = 1 + s / (2 alpha l^2) dK/dl = K s / (l^3 q)                    h = K / (q l^2)
                                                                          dK/dalpha = K (-log q + (q - 1) / q)
    matern32      (l)             a = sqrt(3) r / l    K = (1 + a) exp(-a)                                         h = 3 exp(-a)
    matern52      (l)             a = sqrt(5) r / l    K = (1 + a + a^2 / 3) exp(-a)                               h = 5/3 (1 + a) exp(-a)
    matern32_ard  (l_1..l_d)      a = sqrt(3) rho      as matern32
    matern52_ard  (l_1..l_d)      a = sqrt(5) rho      as matern52
        Matern:  dK/dl = h s / l^3 (isotropic),  dK/dl_k = h (x_k - y_k)^2 / l_k^3 (ARD)
    linear (sigma | sigma_1..sigma_d)   K = sum_k sigma_k x_k y_k        (values only)

    dk(x*, x) / dx*_c = -h (x*_c - x_c) t_c,   t_c = 1 / l_c^2 (ARD), 1 / l^2 (isotropic Matern), 1 (the other isotropic kernels: l is in h)

No Matern derivative holds a 1 / r: at r = 0 the differences are 0 and h is finite, so a coinciding pair contributes an exact 0.
Parameter vectors are in the C ABI's order; points are columns (X is d x n).
"""
import numpy as np

NAMES = ("sqrexp", "gammaexp", "rationalquadratic", "sqrexp_ard", "matern32", "matern52", "matern32_ard", "matern52_ard")   # fit.grad_dict's
MATERN_NAMES = NAMES[4:]
KERNEL_ID = {"sqrexp": 3, "gammaexp": 4, "rationalquadratic": 5, "sqrexp_ard": 6,
             "matern32": 7, "matern52": 8, "matern32_ard": 9, "matern52_ard": 10}   # include/gprc_native.h

# (kernel name, parameters in the ABI's order, d): the cases of the prediction-gradient tests, CPU and GPU
BASE_CASES = [
    ("sqrexp", [0.7], 3),
    ("sqrexp", [1.5], 8),
    ("sqrexp_ard", [0.5, 1.5, 3.0], 3),
    ("gammaexp", [1.2, 1.5], 3),
    ("gammaexp", [1.2, 1.0], 2),
    ("rationalquadratic", [0.9, 1.7], 3),
]
MATERN_CASES = [
    ("matern32", [0.9], 3),
    ("matern52", [1.1], 3),
    ("matern52", [1.5], 8),
    ("matern32_ard", [0.5, 1.5, 3.0], 3),
    ("matern52_ard", [0.6, 1.4, 2.5], 3),
]
CASES = BASE_CASES + MATERN_CASES
SIZES = [(300, 0.1), (600, 0.01)]      # (n, noise)


def case_id(case):
    name, par, d = case
    return "%s-%s-d%d" % (name, "_".join("%g" % p for p in par), d)


def is_ard(name):
    return name.endswith("_ard")


def matern_value_and_h(name, rho2, dtype):
    """(K, h) from rho2 = s / l^2 (ARD: the scaled squared distance), in dtype"""
    nu2 = dtype(3) if name.startswith("matern32") else dtype(5)
    a = np.sqrt(nu2 * rho2)
    e = np.exp(-a)
    one = dtype(1)
    if name.startswith("matern32"):
        return (one + a) * e, dtype(3) * e
    if name.startswith("matern52"):
        return (one + a + a * a / dtype(3)) * e, dtype(5) / dtype(3) * (one + a) * e
    raise KeyError(name)


# ---- between two sets of points, any dtype (the prediction references) ------------------------------------------------------------
def pairwise(name, par, A, B, dtype):
    """(k, h, t): k[i, j] = k(A[:, i], B[:, j]), h as above, t the d per-coordinate factors; everything in dtype"""
    A, B = np.asarray(A, dtype=dtype), np.asarray(B, dtype=dtype)
    d = A.shape[0]
    diff = A[:, :, None] - B[:, None, :]                  # d x m x n
    if name in MATERN_NAMES:
        l = np.asarray(par, dtype=dtype)
        if not is_ard(name):
            assert l.size == 1
            l = np.full(d, l[0], dtype=dtype)
        assert l.size == d
        rho2 = ((diff / l[:, None, None]) ** 2).sum(0)
        k, h = matern_value_and_h(name, rho2, dtype)
        return k, h, dtype(1) / (l * l)
    par = [dtype(p) for p in par]
    one, two = dtype(1), dtype(2)
    if name == "sqrexp_ard":
        l = np.asarray(par, dtype=dtype)
        s = ((diff / l[:, None, None]) ** 2).sum(0)
        k = np.exp(-s / two)
        return k, k, one / (l * l)
    s = (diff * diff).sum(0)
    t = np.ones(d, dtype=dtype)
    if name == "sqrexp":
        l = par[0]
        k = np.exp(-s / (two * l * l))
        return k, k / (l * l), t
    if name == "gammaexp":
        l, g = par
        r = np.sqrt(s)
        u = (r / l) ** g
        k = np.exp(-u)
        zero = s == 0
        h = np.where(zero, dtype(0), k * g * u / np.where(zero, one, s))
        return k, h, t
    if name == "rationalquadratic":
        l, al = par
        q = one + s / (two * al * l * l)
        k = q ** (-al)
        return k, k / (q * l * l), t
    raise ValueError(name)


# ---- on one set of points, float64 (the evidence and leave-one-out references) ----------------------------------------------------
def sqdist_per_dim(X):
    """generator of the n x n matrices (x_ik - x_jk)^2, k = 0 .. d-1"""
    for k in range(X.shape[0]):
        yield np.subtract.outer(X[k], X[k]) ** 2


def _matern_scales(name, theta, d):
    if is_ard(name):
        assert theta.size == d
        return theta
    assert theta.size == 1
    return np.full(d, theta[0])


def kernel(name, theta, X):
    X = np.asarray(X, dtype=float)
    theta = np.atleast_1d(np.asarray(theta, dtype=float))
    if name in MATERN_NAMES:
        rho2 = sum(sk / (l * l) for sk, l in zip(sqdist_per_dim(X), _matern_scales(name, theta, X.shape[0])))
        return matern_value_and_h(name, rho2, np.float64)[0]
    if name == "linear":
        sig = np.full(X.shape[0], theta[0]) if theta.size == 1 else theta
        return (X * sig[:, None]).T @ X
    if name == "sqrexp_ard":
        s = sum(sk / (l * l) for sk, l in zip(sqdist_per_dim(X), theta))
        return np.exp(-0.5 * s)
    s = sum(sqdist_per_dim(X))
    if name == "sqrexp":
        return np.exp(-s / (2.0 * theta[0] ** 2))
    if name == "gammaexp":
        return np.exp(-(np.sqrt(s) / theta[0]) ** theta[1])
    if name == "rationalquadratic":
        return (1.0 + s / (2.0 * theta[1] * theta[0] ** 2)) ** (-theta[1])
    raise KeyError(name)


def kernel_derivs(name, theta, X, K=None):
    """generator of dK / dtheta_i in parameter order (one n x n matrix alive at a time); K = kernel(name, theta, X) when the caller has it
    (the Matern derivatives go through h, not through K)"""
    X = np.asarray(X, dtype=float)
    theta = np.atleast_1d(np.asarray(theta, dtype=float))
    if name in MATERN_NAMES:
        ell = _matern_scales(name, theta, X.shape[0])
        rho2 = sum(sk / (l * l) for sk, l in zip(sqdist_per_dim(X), ell))
        h = matern_value_and_h(name, rho2, np.float64)[1]
        if is_ard(name):
            for sk, l in zip(sqdist_per_dim(X), ell):
                yield h * sk / l ** 3
        else:
            yield h * sum(sqdist_per_dim(X)) / ell[0] ** 3
        return
    if K is None:
        K = kernel(name, theta, X)
    if name == "sqrexp_ard":
        for sk, l in zip(sqdist_per_dim(X), theta):
            yield K * sk / l ** 3
        return
    s = sum(sqdist_per_dim(X))
    if name == "sqrexp":
        yield K * s / theta[0] ** 3
    elif name == "gammaexp":
        l, g = theta
        r = np.sqrt(s)
        u = (r / l) ** g
        yield K * g * u / l
        with np.errstate(divide="ignore", invalid="ignore"):
            t = u * np.log(r / l)
        t[r == 0.0] = 0.0
        yield -K * t
    elif name == "rationalquadratic":
        l, al = theta
        q = 1.0 + s / (2.0 * al * l * l)
        yield K * s / (l ** 3 * q)
        yield K * (-np.log(q) + (q - 1.0) / q)
    else:
        raise KeyError(name)
