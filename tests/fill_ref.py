"""Elementwise reference, error bounds and inputs for every kernel-value form on the device: the fill's finish<KID> (kernels_fill.hip) and
pair_tile.h's kernel_value<KID> and pair_weight<KID>.  Helpers of tests/test_fill_cpu.py and tests/test_gpu_fill.py.  numpy only: no torch,
no GPU.

Reference.  reference() / weight_reference() evaluate the formulas at the head of tests/kernel_ref.py in numpy.longdouble (64-bit
significand) from the exact doubles the device sees: the differences x_k - y_k and the products x_k y_k are rounded once to 2^-64, the sums
are ordinary longdouble sums, rationalquadratic goes through log1p (q^-alpha = exp(-alpha log1p(x)): the natural form, exact for x below
2^-64 where 1 + x would be 1) except at half-integer alpha <= 4, where a root and an integer power keep the log's error, alpha log q 2^-64,
out of a reference that judges the device's root forms (gammaexp at gamma = 0.5, 1, 1.5, 2 likewise); no quantity here has the form
e^t - 1, so expm1 has no place in it.  polynomial follows R's `^`: p = 2 is
b * b, a negative base with a non-integer p is NaN.  Every rounding of the reference is 2^-64 = 2^-11 u where the device has one of u, and
it is amplified by the same condition numbers (cond for the roundings before the transcendental function, 1 for those after it), so the
reference's own error is 2^-11 of each bound below.  tests/test_fill_cpu.py holds it against 40-digit mpmath.

Bound, per element, u = 2^-53, F = 1e-290:

    |got - ref| <= (cond (d + A) + E + C) u max(|ref|, F)

cond = |s k'(s) / k(s)|, the condition number of the value with respect to the (ARD: scaled) squared distance s, from the longdouble
reference.  A relative error eps of s moves k by cond eps; a rounding of relative size delta applied AFTER the last operation that cond
amplifies moves it by delta.  One correctly rounded operation (+ - * / sqrt fma) counts 1 (|delta| <= u); exp, log, log1p and pow of the
device library are 1 ulp functions and count 2.  Below F the check is absolute (F u times the same factor): there exp(-a) of the Matern
kernels is subnormal while the value is not (up to 1e5 u lost between 2^-1022 and 1e-303 by ANY float64 evaluation), and no entry is left
out.  First-order terms only: the largest factor here is about 700 * 50 u = 4e-12, its square is far below one rounding.

d + A: the squared distance and what happens to it before the function.
    distance, isotropic      t = a - b: 1 rounding, twice in t^2 ........................ 2     fma(t, t, s): 1 per coordinate ...... d
    distance, ARD fill       sig = 1 / l_k: 1;  a - b: 1;  (a - b) * sig: 1;  each twice . 6     fma: d
    constant of the quotient sqrexp 2 (l l): 1 (the doubling is exact);  matern (l l) / 3: 2;  gammaexp l l: 1;
                             rationalquadratic 2 alpha (l l): 2 (2 alpha exact, l l, the product)
    quotient                 q = s rc;  q = fma(fma(-q, c, s), rc, q): the residual is exact and the correction leaves s / c to O(u^2)
                             whatever rc's rounding was: 1 (the last fma)
    ARD Matern               u = 3 s (5 s): 1
  A = 4 sqrexp, 6 sqrexp_ard, 5 matern32 / 52, 7 matern32_ard / 52_ard, 4 gammaexp's quotient forms, 2 gammaexp gamma = 2 (no quotient: the
  root and the division by l act on r and are in E), 5 rationalquadratic.  None exceeds 8.

E: the branch's own term, each from the comment on the branch in kernels_fill.hip; a rounding delta of a quantity w that the value
depends on as k(w) costs |w k'(w) / k| delta, which is not cond and is therefore written out here.
    matern32                 a = sqrt(u): 1 rounding of a;  |a k'(a) / k| = a^2 / (1 + a) = 2 cond ............................ E = 2 cond
    matern52, fill           a enters 1 + a and exp(-a) but not u / 3 ("taken from u, which the root has not rounded"):
                             |a d/da [(1 + a + u/3) e^-a]| / k = a (a + a^2/3) / (1 + a + a^2/3) ............................. E = that
    gammaexp, gamma = 2      power = (sqrt(s) / l)^2: sqrt 1, / l 1, each twice in the square, the square 1 ................. E = 5 power
    gammaexp, root forms     power = sqrt(u) (gamma = 1): 1;  sqrt(sqrt(u)) (0.5): 1/2 + 1;  r * rr (1.5): 1 + 3/2 + 1 ..... E = {1.5, 1, 3.5} power
    gammaexp, general        power = exp(gamma/2 log u): the log, a 1 ulp function, 2 and the product with gamma/2 1, both relative to
                             gamma/2 |log u|; the inner exp 2.  (The comment's figure, gamma/2 |log| + 2, read in units of u counts one
                             rounding for the log and its product together: a float64 model of the branch on a host libm reaches 1.03 of
                             the bound made with it, so the count here is the derived one) ........ E = power (3 gamma/2 |log(s / l^2)| + 2);  0 at s = 0
    rationalquadratic, all   the rounding of q = 1 + x, through q^-alpha .................. E = 2 alpha
    rationalquadratic, rsqrt the root's error times 2 alpha, and the Newton steps ......... E = 2 alpha + (2 alpha + 2)
    rationalquadratic, exp / log   exp(-alpha log q): the log 2 and the product 1, both relative to alpha log q (the comment's alpha log q,
                             counted as for gammaexp).  2 alpha alone cannot hold the far tail: alpha log q reaches 668 where cond is
                             alpha x / (1 + x) <= alpha, and the float64 model of the branch is at 20 times a bound without this
                             term (alpha = 0.7, q = 1e100) .............................. E = 2 alpha + 3 alpha log q
    polynomial, table        b = s + sigma rounded once, through b^p: p;  the comment's 3 .. E = p + 3
    everything else          0

C: the roundings after which nothing is amplified.
    exp 2 everywhere it ends the value.  matern32: fma(a, e, e) 1: C = 3.  matern52 (fill): 1/3 as a constant 1, 1 + a 1, the fma 1, the
    product with e 1: C = 6.  rationalquadratic alpha = 2: q q 1, the division 1: C = 2;  rsqrt table: r^h by multiplications, h - 1
    amplified roundings (case 7: r2 three times, r4, r2 r, the product: 6; case 8: 4 + 2 + 1 = 7): C = h - 1;  exp / log form: 2.
    polynomial: table p - 1 by the same count;  p = 2: b's rounding twice and the product, 3;  the library's pow: p for b's rounding
    and 2 for pow, p + 2 (11 at p = 9) -- p = 1 too: the device's pow(b, 1) is not b as a host libm's is (1.5 u measured).  constant: 0 (the parameter comes back as it went in).  None exceeds 16.

linear and polynomial have no s.  The fma chain of the dot product has the absolute error gamma_n sum_k |sigma_k x_k y_k| with n = d
(polynomial) or d + 1 (linear: x_k y_k is rounded before the fma with sigma_k), gamma_n = n u / (1 - n u); carried through the power it is
    p (|b| + D)^(p - 1) D,   D = gamma_n sum_k |x_k y_k|
(the mean-value form: where the base cancels to less than D the first-order p |b|^(p-1) D would no longer be a bound), and the (E + C) u
term multiplies max((|b| + D)^p, F) for the same reason.  linear: p = 1, b = the sum, E = C = 0.

kernel_value and pair_weight (pair_tile.h; reached through gprc_dev_kernel_gemm / gprc_dev_kernel_gemm_grad with an identity matrix on the
f64 matrix cores: a product with exact ones and zeros adds nothing) have their own constants (make_deriv_spec) and the contraction
kernels' staging: see value_terms() and weight_reference() below, which carry their counts.

Inputs: points(), cases(), the conditions of input_conditions().  model64(): a float64 numpy restatement of each device branch in the
device's order of operations; numpy has no fma, so every fma(a, b, c) is formed in longdouble (the product rounded to 64 bits, the sum to
64 and then to 53): not the device's single rounding, but within 2^-11 u of it except at a tie.
"""
import math

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "tests/fill_ref.py needs an extended-precision numpy.longdouble (eps <= 2^-63); this platform's has eps = %g" % float(np.finfo(LD).eps)

U = 2.0 ** -53
F = 1e-290
KERNEL_ID = {"constant": 0, "linear": 1, "polynomial": 2, "sqrexp": 3, "gammaexp": 4, "rationalquadratic": 5, "sqrexp_ard": 6,
             "matern32": 7, "matern52": 8, "matern32_ard": 9, "matern52_ard": 10}   # include/gprc_native.h
STATIONARY = ("sqrexp", "gammaexp", "rationalquadratic", "sqrexp_ard", "matern32", "matern52", "matern32_ard", "matern52_ard")
GEMM_KERNELS = STATIONARY                         # the eight gprc_dev_kernel_gemm accepts
DIMS = (1, 3, 16, 17, 33)                         # one staging pass, the exact pass width, two passes, three with a last pass of one coordinate
GEMM_DIMS = (1, 3, 17, 20)
NA, NB, NA_EVEN = 257, 130, 256
SEED = 11


def gamma(k, u=U):
    return k * u / (1.0 - k * u)


def is_ard(kind):
    return kind.endswith("_ard")


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
DUPLICATES = ((3, 100), (130, 7), (255, 128))     # A[i] == B[j], off the diagonal
DUPLICATE_IN_A = (40, 201)

_POINTS = {}


def points(d, nA=NA, nB=NB, seed=SEED):
    """(A, B): nA x d and nB x d, one point per row (the d x n column-major matrix of the C ABI).  Every point is centre + 10^e v, v a random
    unit vector, e uniform in [-9, 1.5], the centre the origin or one random point of norm 1: pair distances span 20 decades.  Three exact
    duplicates between A and B off the diagonal (DUPLICATES) and one pair inside A (DUPLICATE_IN_A).  Cached; do not write to the result."""
    key = (d, nA, nB, seed)
    if key not in _POINTS:
        rng = np.random.default_rng([seed, d])
        c = rng.normal(size=d)
        centres = np.stack([np.zeros(d), c / np.linalg.norm(c)])

        def draw(n):
            v = rng.normal(size=(n, d))
            v /= np.linalg.norm(v, axis=1)[:, None]
            return centres[rng.integers(0, 2, n)] + 10.0 ** rng.uniform(-9.0, 1.5, n)[:, None] * v

        A, B = draw(max(nA, NA)), draw(max(nB, NB))   # the same points whatever nA: the 256-row run sees the first 256 of the 257
        A, B = A[:nA].copy(), B[:nB].copy()
        for i, j in DUPLICATES:
            B[j] = A[i]
        A[DUPLICATE_IN_A[1]] = A[DUPLICATE_IN_A[0]]
        A.setflags(write=False)
        B.setflags(write=False)
        _POINTS[key] = (A, B)
    return _POINTS[key]


def ard_scales(d, factor):
    """unequal length scales over two decades: factor * 10^(-1 .. 1), in an order that is not monotone"""
    if d == 1:
        return [factor]
    e = np.linspace(-1.0, 1.0, d)
    return (factor * 10.0 ** e[np.random.default_rng(d).permutation(d)]).tolist()


# The small scale of a stationary case: the l (ARD: the common factor) that puts a pair at distance 1 -- the bulk: two points near different
# centres -- at -log k of about 230 (k = 1e-100), so that the pairs beyond pass F.  gammaexp 0.1 needs it nearer the edge (-log k grows
# as r^0.1).  rationalquadratic falls as x^-alpha only: alpha >= 1 reaches F with l^2 still a normal double, alpha = 0.5, 0.7 and 1e-3 cannot
# (q = 1 + s / (2 alpha l^2) overflows first: k >= 1e-155^(2 alpha)); they run at x(1) = 1e100, far beyond anything a fit produces.
def _small_scale(kind, par):
    if kind == "sqrexp":
        return 0.05
    if kind in ("matern32", "matern52"):
        return (math.sqrt(3.0) if kind == "matern32" else math.sqrt(5.0)) / 230.0
    if kind == "gammaexp":
        return (600.0 if par[1] < 0.5 else 230.0) ** (-1.0 / par[1])
    if kind == "rationalquadratic":
        al = par[1]
        if al >= 100.0:
            return math.sqrt(1.0 / (2.0 * al * math.expm1(230.0 / al)))
        if al >= 1.0:
            return math.sqrt(1.0 / (2.0 * al * 10.0 ** ((290.0 - 1.5 * al) / al)))     # k(1) = 10^(-290 + 1.5 alpha): F is passed at s = 10^1.5
        return math.sqrt(1.0 / (2.0 * al * 1e100))
    raise KeyError(kind)


def REACHES_F(kind, par):
    """whether some length scale takes the kernel below F within the 20 decades of the distances (see _small_scale)"""
    return not (kind == "rationalquadratic" and par[1] < 1.0)


GAMMAS = (0.5, 1.0, 1.5, 2.0, 0.1, 1.3, 1.999)
ALPHAS = (0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 4.5, 0.7, 1e-3, 1e3)
DEGREES = (1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 2.5)
SIGMA_SMALL, SIGMA_LARGE = -0.25, 2000.0   # -0.25: every pair with a point near the origin has a negative base; 2000 > max |x . y| = 1100: none has
# the common factor of the ARD scales at the small scale, by d (the permutation of ard_scales decides which coordinates weigh): tried by
# hand until input_conditions() held, no more
ARD_SMALL = {"sqrexp_ard": {1: 0.05, 3: 0.1, 17: 0.3, 20: 0.2, 33: 0.2}, "matern32_ard": {1: 0.0075, 3: 0.02, 16: 0.02, 17: 0.02, 20: 0.02},
             "matern52_ard": {1: 0.0097, 3: 0.02, 17: 0.02, 20: 0.02, 33: 0.02}}


def cases():
    """[(kind, parameters in the ABI's order, d, scale)]: scale is "unit" (l = 1), "small" (see _small_scale) or "-" (no length scale).
    d cycles through DIMS so that every family meets every d."""
    out, k = [], 0

    def add(kind, par, scale):
        nonlocal k
        out.append((kind, [float(v) for v in par], DIMS[k % len(DIMS)], scale))
        k += 1

    def both(kind, rest):
        dd = DIMS[k % len(DIMS)]
        out.append((kind, [1.0] + rest, dd, "unit"))
        out.append((kind, [_small_scale(kind, [1.0] + rest)] + rest, dd, "small"))

    for p in DEGREES:
        add("polynomial", [SIGMA_SMALL, p], "-")
        k -= 1
        add("polynomial", [SIGMA_LARGE, p], "-")
    for g in GAMMAS:
        both("gammaexp", [g])
        k += 1
    for al in ALPHAS:
        both("rationalquadratic", [al])
        k += 1
    for kind in ("sqrexp", "matern32", "matern52"):
        for dd in (DIMS if kind == "sqrexp" else DIMS[k % 5:k % 5 + 1]):   # sqrexp, the flagship, at every d
            out.append((kind, [1.0], dd, "unit"))
            out.append((kind, [_small_scale(kind, [1.0])], dd, "small"))
        k += 1
    for kind in ("sqrexp_ard", "matern32_ard", "matern52_ard"):
        for dd in (3, 17, 33) if kind == "sqrexp_ard" else ((16,) if kind == "matern32_ard" else (33,)):
            out.append((kind, ard_scales(dd, 1.0), dd, "unit"))
            out.append((kind, ard_scales(dd, ARD_SMALL[kind][dd]), dd, "small"))
    add("constant", [3.7], "-")
    add("linear", [0.3], "-")
    out.append(("linear", np.random.default_rng(5).uniform(-2.0, 2.0, 17).tolist(), 17, "-"))
    out.append(("linear", np.random.default_rng(6).uniform(-2.0, 2.0, 33).tolist(), 33, "-"))
    return out


def case_id(case):
    kind, par, d, scale = case
    return "%s-%s-d%d-%s" % (kind, "_".join("%.4g" % p for p in par[:2]), d, scale)


# one case per kernel family at the small scale: the panel and cross fills
FAMILY_CASES = [("sqrexp", [_small_scale("sqrexp", [1.0])], 3), ("sqrexp_ard", ard_scales(17, ARD_SMALL["sqrexp_ard"][17]), 17),
                ("matern32", [_small_scale("matern32", [1.0])], 16), ("matern52_ard", ard_scales(3, ARD_SMALL["matern52_ard"][3]), 3),
                ("gammaexp", [_small_scale("gammaexp", [1.0, 1.3]), 1.3], 17), ("gammaexp", [_small_scale("gammaexp", [1.0, 1.5]), 1.5], 1),
                ("rationalquadratic", [_small_scale("rationalquadratic", [1.0, 1e3]), 1e3], 33),
                ("rationalquadratic", [_small_scale("rationalquadratic", [1.0, 3.0]), 3.0], 3),
                ("polynomial", [SIGMA_SMALL, 7.0], 17), ("linear", [0.3], 3), ("constant", [3.7], 3)]


def gemm_cases():
    """[(kind, par, d)]: the eight kernels of gprc_dev_kernel_gemm at GEMM_DIMS; unit scale and small scale alternate over d"""
    out = []
    for kind in GEMM_KERNELS:
        for i, d in enumerate(GEMM_DIMS):
            small = i % 2 == 1
            if is_ard(kind):
                par = ard_scales(d, ARD_SMALL[kind][d] if small else 1.0)
            elif kind == "gammaexp":
                g = (0.5, 1.3, 2.0, 1.0)[i]
                par = [_small_scale(kind, [1.0, g]) if small else 1.0, g]
            elif kind == "rationalquadratic":
                al = (0.7, 1e3, 2.0, 1.5)[i]
                # alpha = 1.5 at l = 1e-3, not at the fill's 1e-97: pair_weight's k / (1 + x) underflows there before the tail's 1 / l^2 = 1e193
                # brings it back, which no bound relative to the result can follow and no fit can meet
                par = [(_small_scale(kind, [1.0, al]) if al >= 100.0 else 1e-3) if small else 1.0, al]
            else:
                par = [_small_scale(kind, [1.0]) if small else 1.0]
            out.append((kind, [float(v) for v in par], d))
    return out


# ---- the branch a case reaches -----------------------------------------------------------------------------------------------------
def branch(kind, par):
    """the switch case or early return of finish<KID> that (kind, par) reaches"""
    if kind == "polynomial":
        p = par[1]
        if 3.0 <= p <= 8.0 and p == int(p):
            return "polynomial/table case %s" % ("default (8)" if p == 8 else "%d" % p)
        return "polynomial/r_pow x*x" if p == 2.0 else "polynomial/r_pow pow"
    if kind == "gammaexp":
        g = par[1]
        if g == 2.0:
            return "gammaexp/gamma == 2 (sqrt, r_pow x*x)"
        if 2.0 * g in (1.0, 2.0, 3.0):
            return "gammaexp/root form h = %d" % int(2 * g)
        return "gammaexp/exp(g/2 log u)"
    if kind == "rationalquadratic":
        al = par[1]
        if al == 2.0:
            return "rationalquadratic/al == 2"
        h = 2.0 * al
        if 1.0 <= h <= 8.0 and h == int(h):
            return "rationalquadratic/rsqrt table case %s" % ("default (8)" if h == 8 else "%d" % h)
        return "rationalquadratic/exp(-al log q)"
    return kind


# ---- reference ---------------------------------------------------------------------------------------------------------------------
class Ref:
    """k: the values (longdouble, NaN where R's `^` gives NaN); cond; aux: what the bounds need (all longdouble, nA x nB)"""

    def __init__(self, k, cond, **aux):
        self.k, self.cond, self.aux = k, cond, aux


def _sqdist(A, B, inv_l=None):
    """sum_k ((a_k - b_k) [/ l_k])^2 in longdouble, coordinate by coordinate"""
    s = np.zeros((A.shape[0], B.shape[0]), dtype=LD)
    for k in range(A.shape[1]):
        t = A[:, k].astype(LD)[:, None] - B[:, k].astype(LD)[None, :]
        if inv_l is not None:
            t = t / LD(inv_l[k])
        s += t * t
    return s


def _stationary(kind, par, s):
    """(k, cond, aux) from the squared distance s (ARD: the scaled one), longdouble"""
    one, two, three = LD(1), LD(2), LD(3)
    if kind in ("sqrexp", "sqrexp_ard"):
        x = s / two if is_ard(kind) else s / (two * LD(par[0]) * LD(par[0]))
        return np.exp(-x), x, {}
    if kind.startswith("matern"):
        rho2 = s if is_ard(kind) else s / (LD(par[0]) * LD(par[0]))
        if kind.startswith("matern32"):
            a = np.sqrt(three * rho2)
            return (one + a) * np.exp(-a), a * a / (two * (one + a)), {"a": a}
        a = np.sqrt(LD(5) * rho2)
        P = one + a + a * a / three
        return P * np.exp(-a), a * a * (one + a) / (LD(6) * P), {"a": a}
    if kind == "gammaexp":
        l, g = LD(par[0]), LD(par[1])
        v = s / (l * l)
        with np.errstate(divide="ignore"):
            lg = np.log(v)
        if 2.0 * par[1] in (1.0, 2.0, 3.0, 4.0):                  # a power by roots where there is one: the reference must not carry
            r = np.sqrt(v)                                        # the log's error where the device's root forms do not
            power = {1: np.sqrt(r), 2: r, 3: r * np.sqrt(r), 4: v}[int(2 * par[1])]
        else:
            power = np.where(s == 0, LD(0), np.exp(g / two * np.where(s == 0, LD(0), lg)))   # u^(gamma/2), 0 at s = 0 as R's 0^gamma
        return np.exp(-power), power * g / two, {"power": power, "log": np.where(s == 0, LD(0), lg)}
    if kind == "rationalquadratic":
        l, al = LD(par[0]), LD(par[1])
        x = s / (two * al * l * l)
        lq = np.log1p(x)
        h = 2.0 * par[1]
        if 1.0 <= h <= 8.0 and h == int(h):                       # half-integer alpha: a root and an integer power, so that the reference does
            k = np.power(one / np.sqrt(one + x), LD(h))           # not carry alpha log q times the log's error where the device's table does not
        else:
            k = np.exp(-al * lq)
        return k, al * x / (one + x), {"x": x, "alogq": al * lq}
    raise KeyError(kind)


def reference(kind, par, A, B):
    """Ref of k(A[i], B[j]), nA x nB"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    d = A.shape[1]
    if kind == "constant":
        k = np.full((A.shape[0], B.shape[0]), LD(par[0]))
        return Ref(k, np.zeros(k.shape, dtype=LD))
    if kind in ("linear", "polynomial"):
        sig = np.ones(d) if kind == "polynomial" else (np.full(d, par[0]) if len(par) == 1 else np.asarray(par, dtype=np.float64))
        dot = np.zeros((A.shape[0], B.shape[0]), dtype=LD)
        dotabs = np.zeros_like(dot)
        for c in range(d):
            t = (LD(sig[c]) * A[:, c].astype(LD))[:, None] * B[:, c].astype(LD)[None, :]
            dot += t
            dotabs += np.abs(t)
        if kind == "linear":
            return Ref(dot, None, b=dot, dotabs=dotabs, p=1.0)
        b, p = dot + LD(par[0]), par[1]
        if p == 2.0:
            k = b * b
        elif p == int(p):
            k = np.power(b, LD(p))                               # an integer degree keeps the sign of an odd power
        else:
            with np.errstate(invalid="ignore"):
                k = np.where(b < 0, LD(np.nan), np.power(np.abs(b), LD(p)))   # R: pow of a negative base to a non-integer is NaN
        return Ref(k, None, b=b, dotabs=dotabs, p=p)
    s = _sqdist(A, B, par if is_ard(kind) else None)
    k, cond, aux = _stationary(kind, par, s)
    return Ref(k, cond, s=s, **aux)


# ---- bounds --------------------------------------------------------------------------------------------------------------------------
def fill_terms(kind, par, ref):
    """(A, E, C) of finish<KID> as derived in the module docstring; E may be an array"""
    if kind == "sqrexp":
        return 4, 0.0, 2
    if kind == "sqrexp_ard":
        return 6, 0.0, 2
    if kind.startswith("matern"):
        A = 7 if is_ard(kind) else 5
        a = ref.aux["a"]
        if kind.startswith("matern32"):
            return A, 2 * ref.cond, 3
        return A, a * (a + a * a / 3) / (1 + a + a * a / 3), 6
    if kind == "gammaexp":
        g, power = par[1], ref.aux["power"]
        if g == 2.0:
            return 2, 5 * power, 2
        if 2.0 * g in (1.0, 2.0, 3.0):
            return 4, {1: 1.5, 2: 1.0, 3: 3.5}[int(2 * g)] * power, 2
        return 4, power * (3 * g / 2 * np.abs(ref.aux["log"]) + 2), 2
    if kind == "rationalquadratic":
        al = par[1]
        if al == 2.0:
            return 5, 2 * al, 2
        h = 2.0 * al
        if 1.0 <= h <= 8.0 and h == int(h):
            return 5, 2 * al + (2 * al + 2), int(h) - 1
        return 5, 2 * al + 3 * ref.aux["alogq"], 2
    raise KeyError(kind)


def poly_terms(par):
    """(E, C) of finish<GPRC_POLYNOMIAL>"""
    p = par[1]
    if 3.0 <= p <= 8.0 and p == int(p):
        return p + 3, int(p) - 1
    if p == 2.0:
        return 0, 3
    return 0, p + 2


def _dot_bound(kind, par, d, ref):
    b, dotabs = np.abs(ref.aux["b"]), ref.aux["dotabs"]
    if kind == "linear":
        return gamma(d + 1) * dotabs
    p = par[1]
    D = gamma(d) * dotabs
    E, C = poly_terms(par)
    top = np.power(b + D, LD(p))
    return LD(p) * np.power(b + D, LD(p - 1)) * D + (E + C) * U * np.maximum(top, LD(F))


def _floor(ref_k):
    return np.maximum(np.abs(ref_k), LD(F))


def fill_bound(kind, par, d, ref):
    """the absolute bound of |got - ref.k| per element for the fill, longdouble; NaN where the reference is NaN"""
    if kind == "constant":
        return np.zeros(ref.k.shape, dtype=LD)
    if kind in ("linear", "polynomial"):
        bd = _dot_bound(kind, par, d, ref)
        return np.where(np.isnan(ref.k), LD(np.nan), bd)
    A, E, C = fill_terms(kind, par, ref)
    return (ref.cond * (d + A) + E + C) * U * _floor(ref.k)


# kernel_value<KID> (pair_tile.h), constants from make_deriv_spec.  The distance is the contraction kernels': isotropic as the fill's (2 + d);
# ARD stages a sig and b sig (sig = 1 / l_k: 1 rounding, the product 1: 2 each) and subtracts (1), so the difference carries an ABSOLUTE error
# 2 u (|a_k| + |b_k|) / l_k + u |t_k|, which is rho_k u |t_k| with rho_k = 1 + 2 (|a_k| + |b_k|) / |a_k - b_k|; t_k^2 carries twice that, and
#     the relative error of s is (d + D_ard) u,   D_ard = 2 sum_k rho_k t_k^2 / s    (0 for a duplicate)
# in place of d + 2: near a duplicate beside a centre of norm 1 it is large, and cond is small there.
#   sqrexp     p[1] = 1 / (2 (l l)): 2;  s p[1]: 1 .................................. A = 2 + 3,  C = 2 (exp)
#   sqrexp_ard -0.5 s exact ...................................................... A = D_ard,  C = 2
#   matern     p[1] = 3 / (l l): 2;  s p[1]: 1 (ARD: 3 s: 1) .................... A = 2 + 3 (D_ard + 1),  E = 2 cond (the root; matern52 forms a a, so a
#              enters consistently);  C = 3 (matern32), 2 + 1 (a a) + 4 = 7 (matern52)
#   gammaexp   p[2] = 1 / (l l): 2;  s p[2]: 1;  p[3] = gamma / 2 exact ......... A = 2 + 3,  E = power (3 gamma/2 |log| + 2) as the fill's general form:
#              the log's error and the product's, relative to the power;  C = 2;  s = 0 returns 1 exactly
#   ratquad    p[2] = 1 / (2 alpha (l l)): 3;  s p[2]: 1 ........................ A = 2 + 4,  E = 3 alpha log1p(x) as the fill's exp / log form (no q = 1 + x
#              is rounded: log1p),  C = 2
def _ard_dist(A, B, par, s):
    """D_ard above, longdouble nA x nB"""
    acc = np.zeros(s.shape, dtype=LD)
    for k in range(A.shape[1]):
        a, b = A[:, k].astype(LD)[:, None], B[:, k].astype(LD)[None, :]
        t = a - b
        rho = 1 + 2 * (np.abs(a) + np.abs(b)) / np.where(t == 0, LD(1), np.abs(t))
        acc += np.where(t == 0, LD(0), rho * (t / LD(par[k])) ** 2)
    return 2 * acc / np.where(s == 0, LD(1), s)


def value_terms(kind, par, ref, A, B):
    if kind == "sqrexp":
        return 5, 0.0, 2
    if kind == "sqrexp_ard":
        return _ard_dist(A, B, par, ref.aux["s"]), 0.0, 2
    if kind.startswith("matern"):
        Aterm = _ard_dist(A, B, par, ref.aux["s"]) + 1 if is_ard(kind) else 5
        return Aterm, 2 * ref.cond, 3 if kind.startswith("matern32") else 7
    if kind == "gammaexp":
        return 5, ref.aux["power"] * (3 * par[1] / 2 * np.abs(ref.aux["log"]) + 2), 2
    if kind == "rationalquadratic":
        return 6, 3 * ref.aux["alogq"], 2
    raise KeyError(kind)


def value_bound(kind, par, d, ref, A, B):
    At, E, C = value_terms(kind, par, ref, A, B)
    return (ref.cond * (d + At) + E + C) * U * _floor(ref.k)


# pair_weight<KID> through gprc_dev_kernel_gemm_grad: element (i, j, c) = -t_c h(a_i, b_j) (a_ic - b_jc), kernel_ref.pairwise's h and t.
# cond_h = |s h'(s) / h|.  Besides h's own roundings: the staged difference (isotropic 1; ARD rho_c, see above), its product with the
# weight 1, the pair-independent factor of the tail (deriv_tail_factor and, ARD, the derived p[c]) and the tail's product 1.
#   sqrexp      h = k / l^2: cond_h = x;  exp 2;  tail 1 / (l l): 2 ............................................ C = 2 + 1 + 1 + 2 + 1 = 7
#   sqrexp_ard  h = k: cond_h = s / 2;  exp 2;  tail 1.0 * p[c]: p[c]'s rounding 1 ............................ C = 2 + rho_c + 1 + 1 + 1
#   matern32    h = 3 e^-a: cond_h = a / 2, E = a (the root);  exp 2;  tail 3 (1 / (l l)): 3 (ARD 3 p[c]: 2) .. C = 2 + 1 + 1 + 3 + 1 = 8 (ARD 6 + rho_c)
#   matern52    h = 5/3 (1 + a) e^-a: cond_h = a^2 / (2 (1 + a)), E = 2 cond_h;  exp 2, fma 1;  tail 5/3 (1 / (l l)): 4 (ARD 5/3 p[c]: 3)
#                                                                                                      C = 3 + 1 + 1 + 4 + 1 = 10 (ARD 8 + rho_c)
#   gammaexp    h = k gamma u / s: cond_h = |gamma/2 (1 - u) - 1|;  the power's error enters e^-u u as |1 - u|: E = |1 - u| (3 gamma/2 |log| + 2);
#               exp 2, the product 1, the division 1;  tail gamma: 0 ........................................... C = 4 + 1 + 1 + 0 + 1 = 7;  s = 0: exactly 0
#   ratquad     h = k / (q l^2): cond_h = (alpha + 1) x / (1 + x);  E = 3 alpha log1p(x);  exp 2, 1 + x 1, the division 1;  tail 2 .... C = 4 + 1 + 1 + 2 + 1 = 9
def weight_reference(kind, par, A, B):
    """(want, bound): d x nA x nB longdouble arrays of -t_c h (a_ic - b_jc) and of the bound on |got - want|"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    d = A.shape[1]
    ref = reference(kind, par, A, B)
    one = LD(1)
    k, cond, s = ref.k, ref.cond, ref.aux["s"]
    if kind == "sqrexp":
        h, ch, E, At, C = k / (LD(par[0]) ** 2), cond, 0.0, 5, 7
    elif kind == "sqrexp_ard":
        h, ch, E, At, C = k, cond, 0.0, _ard_dist(A, B, par, s), 5
    elif kind.startswith("matern"):
        a = ref.aux["a"]
        e = np.exp(-a)
        ard = is_ard(kind)
        At = _ard_dist(A, B, par, s) + 1 if ard else 5
        if kind.startswith("matern32"):
            h, ch, C = LD(3) * e, a / 2, 6 if ard else 8
        else:
            h, ch, C = LD(5) / LD(3) * (one + a) * e, a * a / (2 * (one + a)), 8 if ard else 10
        E = 2 * ch
    elif kind == "gammaexp":
        g, u = LD(par[1]), ref.aux["power"]
        zero = s == 0
        h = np.where(zero, LD(0), k * g * u / np.where(zero, one, s))
        ch = np.abs(g / 2 * (one - u) - one)
        E, At, C = np.abs(one - u) * (3 * par[1] / 2 * np.abs(ref.aux["log"]) + 2), 5, 7
    elif kind == "rationalquadratic":
        x = ref.aux["x"]
        h = k / ((one + x) * LD(par[0]) ** 2)
        ch, E, At, C = (LD(par[1]) + one) * x / (one + x), 3 * ref.aux["alogq"], 6, 9
    else:
        raise KeyError(kind)
    tc = [one / (LD(par[c]) ** 2) if is_ard(kind) else (one / (LD(par[0]) ** 2) if kind.startswith("matern") else one) for c in range(d)]
    want = np.empty((d,) + k.shape, dtype=LD)
    bound = np.empty_like(want)
    for c in range(d):
        a, b = A[:, c].astype(LD)[:, None], B[:, c].astype(LD)[None, :]
        t = a - b
        want[c] = -tc[c] * h * t
        rho = 1 + 2 * (np.abs(a) + np.abs(b)) / np.where(t == 0, one, np.abs(t)) if is_ard(kind) else 0.0
        bound[c] = (ch * (d + At) + E + C + rho) * U * np.maximum(np.abs(want[c]), np.where(t == 0, LD(0), LD(F)))
    return want, bound


# ---- the float64 model of the device's branches ---------------------------------------------------------------------------------------
def _fma(a, b, c):
    return (np.asarray(a, dtype=LD) * np.asarray(b, dtype=LD) + np.asarray(c, dtype=LD)).astype(np.float64)


def _quot(s, c):
    rc = 1.0 / c
    q = s * rc
    return _fma(_fma(-q, c, s), rc, q)


def _pow_table(b, h):
    b2 = b * b
    b4 = b2 * b2
    return {1: b, 2: b2, 3: b2 * b, 4: b4, 5: b4 * b, 6: b4 * b2, 7: b4 * (b2 * b)}.get(h, b4 * b4)


def model64(kind, par, A, B, swap=0, ratquad_pow=False):
    """finish<KID> over accum<KID> in float64 numpy, nA x nB.  swap: the table entry taken is h + swap instead of h (polynomial degree,
    rationalquadratic 2 alpha, gammaexp 2 gamma): the neighbouring-entry typo of test_fill_cpu.py.  See the module docstring on fma."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    d = A.shape[1]
    s = np.zeros((A.shape[0], B.shape[0]))
    for c in range(d):
        a, b = A[:, c][:, None], B[:, c][None, :]
        if kind == "constant":
            pass
        elif kind == "linear":
            s = _fma(par[0] if len(par) == 1 else par[c], a * b, s)
        elif kind == "polynomial":
            s = _fma(a, b, s)
        elif is_ard(kind):
            t = (a - b) * (1.0 / par[c])
            s = _fma(t, t, s)
        else:
            t = a - b
            s = _fma(t, t, s)
    with np.errstate(all="ignore"):
        if kind == "constant":
            return np.full(s.shape, par[0])
        if kind == "linear":
            return s
        if kind == "polynomial":
            b, p = s + par[0], par[1]
            if 3.0 <= p <= 8.0 and p == int(p):
                return _pow_table(b, int(p) + swap)
            return b * b if p == 2.0 else np.power(b, p)
        if kind == "sqrexp":
            return np.exp(-_quot(s, 2.0 * (par[0] * par[0])))
        if kind == "sqrexp_ard":
            return np.exp(-0.5 * s)
        if kind.startswith("matern"):
            m32 = kind.startswith("matern32")
            u = (3.0 if m32 else 5.0) * s if is_ard(kind) else _quot(s, (par[0] * par[0]) / (3.0 if m32 else 5.0))
            a = np.sqrt(u)
            e = np.exp(-a)
            return _fma(a, e, e) if m32 else _fma(u, 1.0 / 3.0, 1.0 + a) * e
        if kind == "gammaexp":
            g = par[1]
            if g == 2.0:
                r = np.sqrt(s) / par[0]
                return np.exp(-(r * r))
            u = _quot(s, par[0] * par[0])
            h = int(2 * g) if 2.0 * g in (1.0, 2.0, 3.0) else 0
            if h:
                h += swap
                r = np.sqrt(u)
                rr = np.sqrt(r)
                return np.exp(-r) if h == 2 else np.exp(-rr if h == 1 else -(r * rr))
            return np.exp(-np.exp(0.5 * g * np.log(u)))
        if kind == "rationalquadratic":
            al = par[1]
            q = 1.0 + _quot(s, 2.0 * al * (par[0] * par[0]))
            if al == 2.0:
                return 1.0 / (q * q)
            h = 2.0 * al
            if 1.0 <= h <= 8.0 and h == int(h):
                r = 1.0 / np.sqrt(q)                             # v_rsq_f64 and its two Newton steps
                for _ in range(2):
                    e = _fma(-(q * r), r, 1.0)
                    r = _fma(0.5 * r, e, r)
                return _pow_table(r, int(h) + swap)
            return np.power(q, -al) if ratquad_pow else np.exp(-al * np.log(q))
    raise KeyError(kind)


# ---- measures --------------------------------------------------------------------------------------------------------------------------
def fractions(got, ref_k, bound):
    """|got - ref| / bound per element (float64), 0 where both are 0; NaN positions must agree and are reported as 0; inf where the bound is
    0 and got differs"""
    got = np.asarray(got, dtype=np.float64)
    nan_ref = np.isnan(ref_k)
    assert np.array_equal(np.isnan(got), nan_ref), "NaN mask: got %d, reference %d" % (np.isnan(got).sum(), nan_ref.sum())
    err = np.abs(np.where(nan_ref, LD(0), got.astype(LD) - np.where(nan_ref, LD(0), ref_k)))
    bd = np.where(nan_ref, LD(1), bound)
    out = np.where(err == 0, LD(0), err / np.where(bd == 0, LD(1), bd))
    out = np.where((bd == 0) & (err != 0), LD(np.inf), out)
    return out.astype(np.float64)


def input_conditions(case, A, B):
    """{name: value} of the conditions a case's inputs must meet, from the reference alone"""
    kind, par, d, scale = case
    ref = reference(kind, par, A, B)
    k = ref.k.astype(np.float64)
    out = {}
    if kind in STATIONARY:
        s = ref.aux["s"].astype(np.float64)
        if is_ard(kind):                                        # decades of the unscaled distance: the scales only shift them
            s = _sqdist(A, B).astype(np.float64)
        dec = np.floor(np.log10(s[s > 0])).astype(int)
        out["min_per_decade"] = min(int((dec == e).sum()) for e in range(-18, 3))
        if scale == "small":
            out["below_F"] = float((k < F).mean())
            out["mid"] = float(((k >= F) & (k <= 1e-10)).mean())
    if kind == "polynomial":
        out["negative"] = float((ref.aux["b"] < 0).mean())
    return out


def _staged_sqdist(kind, par, A, B):
    """the contraction kernels' distance in float64: ARD stages a * (1 / l_k) and b * (1 / l_k) and subtracts"""
    s = np.zeros((A.shape[0], B.shape[0]))
    for c in range(A.shape[1]):
        sig = 1.0 / par[c] if is_ard(kind) else 1.0
        t = (A[:, c] * sig)[:, None] - (B[:, c] * sig)[None, :]
        s = _fma(t, t, s)
    return s


def value_model64(kind, par, A, B):
    """kernel_value<KID> (pair_tile.h) with make_deriv_spec's constants in float64 numpy"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    s = _staged_sqdist(kind, par, A, B)
    with np.errstate(all="ignore"):
        if kind == "sqrexp":
            return np.exp(-s * (1.0 / (2.0 * (par[0] * par[0]))))
        if kind == "sqrexp_ard":
            return np.exp(-0.5 * s)
        if kind.startswith("matern"):
            m32 = kind.startswith("matern32")
            nu2 = 3.0 if m32 else 5.0
            a = np.sqrt(nu2 * s if is_ard(kind) else s * (nu2 / (par[0] * par[0])))
            e = np.exp(-a)
            return _fma(a, e, e) if m32 else _fma(a * a, 1.0 / 3.0, 1.0 + a) * e
        if kind == "gammaexp":
            return np.where(s > 0, np.exp(-np.exp(0.5 * par[1] * np.log(s * (1.0 / (par[0] * par[0]))))), 1.0)
        if kind == "rationalquadratic":
            return np.exp(-par[1] * np.log1p(s * (1.0 / (2.0 * par[1] * (par[0] * par[0])))))
    raise KeyError(kind)


def weight_model64(kind, par, A, B):
    """d x nA x nB: pair_weight<KID> times the staged difference times the tail's factor (deriv_tail_factor), float64 numpy"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    d = A.shape[1]
    s = _staged_sqdist(kind, par, A, B)
    il2 = 1.0 / (par[0] * par[0])
    with np.errstate(all="ignore"):
        if kind == "sqrexp":
            w, iso = np.exp(-s * (1.0 / (2.0 * (par[0] * par[0])))), il2
        elif kind == "sqrexp_ard":
            w, iso = np.exp(-0.5 * s), 1.0
        elif kind.startswith("matern"):
            m32 = kind.startswith("matern32")
            nu2 = 3.0 if m32 else 5.0
            a = np.sqrt(nu2 * s if is_ard(kind) else s * (nu2 / (par[0] * par[0])))
            e = np.exp(-a)
            w = e if m32 else _fma(a, e, e)
            iso = (3.0 if m32 else 5.0 / 3.0) * (1.0 if is_ard(kind) else il2)
        elif kind == "gammaexp":
            u = np.exp(0.5 * par[1] * np.log(s * il2))
            w, iso = np.where(s > 0, np.exp(-u) * u / np.where(s > 0, s, 1.0), 0.0), par[1]
        elif kind == "rationalquadratic":
            x = s * (1.0 / (2.0 * par[1] * (par[0] * par[0])))
            w, iso = np.exp(-par[1] * np.log1p(x)) / (1.0 + x), il2
        else:
            raise KeyError(kind)
    out = np.empty((d,) + s.shape)
    for c in range(d):
        sig = 1.0 / par[c] if is_ard(kind) else 1.0
        g = w * ((A[:, c] * sig)[:, None] - (B[:, c] * sig)[None, :])
        out[c] = g * (-1.0 * (iso * sig if is_ard(kind) else iso))
    return out
