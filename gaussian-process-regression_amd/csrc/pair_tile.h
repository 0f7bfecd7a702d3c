// pair_tile.h -- the pairwise-tile core of the covariance side for gfx950 (MI355X), shared by kernels_fill.hip (the fills),
// kernels_grad.hip (the contractions of both exact evidence gradients), kernels_pgrad.hip (the prediction gradients' contraction),
// kernels_sgrad.hip (the sparse bound gradient's contraction; its weight per pair, cross_weight, is its own, for the reasons below) and
// kernels_igrad.hip (the iterative GPR's evidence gradient: cross_weight and the staging; its lane layout is the f64 MFMA accumulator's).
//
// One tile of point pairs: PT_R x PT_C = 128 x 64 per 256-thread workgroup, two consecutive rows x 16 columns per lane.  Both point
// sets go through LDS PT_D = 16 coordinates at a time (As[r][i] coordinate-major for the 16-byte row reads, Bs[j][r] padded by one for
// the column broadcasts); the squared distance of a lane's 32 pairs accumulates in s0[16] / s1[16]; a per-kernel epilogue follows.
// What is here: the tile shape, the staging loop, the distance loop of the contraction kernels, the wave and four-wave sums, R's `^`,
// the weight h of a pair in dk / dx* (pair_weight) with the factor it leaves to the tail (deriv_tail_factor), the weight and theta
// integrands of a pair in dk / dtheta for a general weight matrix (cross_weight) and what such a pair adds to the theta sums (theta_terms:
// kernels_igrad.hip and the small-model kernels of small_model.h; kernels_sgrad.hip's `pair` lambda feeds its dz sums from the same
// weight inside the same branch and stays its own),
// and for the host the derived constants of the contraction kernels, the set of kernels with an exact gradient and the dispatcher
// from a run-time kernel id to a template instantiation.
//
// What is deliberately NOT shared:
//   * the fill's accum<KID> (kernels_fill.hip).  Its ARD term is (a - b) * sig, the contraction kernels stage a * sig and b * sig and
//     subtract: the two round differently, the fill is tied to the oracle at 1e-13 and the gradients to their own references, and
//     both stay as they are.
//   * the kernel value and its intermediates per kernel (u, log for gammaexp; x, q, log1p for ratquad).  kernels_grad.hip forms
//     (m * exp(-u)) * u and m * exp(-alpha log1p x), pair_weight below (the gradients with respect to a point: kernels_pgrad.hip and
//     the sample paths' gradient product of kernels_paths.hip) exp(-u) * u / s and exp(-alpha log1p x) / (1 + x), the fill
//     its measured fast paths (finish<KID>): a shared function would fix one order of multiplications for all three.  kernel_value
//     below is a fourth form and belongs to the generated-operand products (kernels_paths.hip) and the pivoted Cholesky that
//     preconditions them (kernels_cg.hip): those two must see the same matrix, nobody else uses it.
#pragma once
#include <string>
#include <type_traits>
#include <utility>

#include "gprc_internal.h"

namespace gprc {

constexpr int PT_R = 128;  // tile rows: 2 consecutive rows per lane x 64 lanes
constexpr int PT_C = 64;   // tile cols: 16 per wave x 4 waves
constexpr int PT_D = 16;   // coordinates staged per pass

// ---- host: kernel ids -> instantiations ----------------------------------------------------------------------------------------
// f(std::integral_constant<int, ID>{}) for the ID among Ids that equals id; false when none does
template <int... Ids, class F>
inline bool with_kernel_id(int id, F&& f) {
  return ((id == Ids ? (f(std::integral_constant<int, Ids>{}), true) : false) || ...);
}
template <class F>
inline bool with_any_kernel(int id, F&& f) {
  return with_kernel_id<GPRC_CONSTANT, GPRC_LINEAR, GPRC_POLYNOMIAL, GPRC_SQREXP, GPRC_GAMMAEXP, GPRC_RATQUAD, GPRC_SQREXP_ARD, GPRC_MATERN32, GPRC_MATERN52,
                        GPRC_MATERN32_ARD, GPRC_MATERN52_ARD>(id, std::forward<F>(f));
}
// the families the per-kernel bodies branch on: one length scale per coordinate; Matern of either order, ARD or not
constexpr bool is_ard(int id) { return id == GPRC_SQREXP_ARD || id == GPRC_MATERN32_ARD || id == GPRC_MATERN52_ARD; }
constexpr bool is_matern32(int id) { return id == GPRC_MATERN32 || id == GPRC_MATERN32_ARD; }
constexpr bool is_matern52(int id) { return id == GPRC_MATERN52 || id == GPRC_MATERN52_ARD; }
constexpr bool is_matern(int id) { return is_matern32(id) || is_matern52(id); }
// the kernels whose dK / dtheta and dk / dx* the contraction kernels know: THE statement of that set
template <class F>
inline bool with_gradient_kernel(int id, F&& f) {
  return with_kernel_id<GPRC_SQREXP, GPRC_GAMMAEXP, GPRC_RATQUAD, GPRC_SQREXP_ARD, GPRC_MATERN32, GPRC_MATERN52, GPRC_MATERN32_ARD, GPRC_MATERN52_ARD>(
      id, std::forward<F>(f));
}
inline bool has_exact_gradient(int kernel_id) { return with_gradient_kernel(kernel_id, [](auto) {}); }
inline int check_grad_kernel(const char* who, int kernel_id) {
  if (has_exact_gradient(kernel_id)) return 0;
  set_error(std::string(who) + ": defined for sqrexp, gammaexp, rationalquadratic and sqrexp_ard, matern32, matern52, matern32_ard and matern52_ard");
  return GPRC_ERR_ARG;
}

// the spec with the constants the contraction kernels want:
//   sqrexp p[1] = 1 / (2 l^2);  gammaexp p[2] = 1 / l^2, p[3] = gamma / 2;  ratquad p[2] = 1 / (2 alpha l^2);  ARD p[k] = 1 / l_k;
//   matern32 p[1] = 3 / l^2;  matern52 p[1] = 5 / l^2
inline KernelSpec make_deriv_spec(const KernelSpec& ks) {
  KernelSpec g = ks;
  if (ks.id == GPRC_SQREXP) g.p[1] = 1.0 / (2.0 * (ks.p[0] * ks.p[0]));
  if (ks.id == GPRC_GAMMAEXP) { g.p[2] = 1.0 / (ks.p[0] * ks.p[0]); g.p[3] = 0.5 * ks.p[1]; }
  if (ks.id == GPRC_RATQUAD) g.p[2] = 1.0 / (2.0 * ks.p[1] * (ks.p[0] * ks.p[0]));
  if (ks.id == GPRC_MATERN32) g.p[1] = 3.0 / (ks.p[0] * ks.p[0]);
  if (ks.id == GPRC_MATERN52) g.p[1] = 5.0 / (ks.p[0] * ks.p[0]);
  if (is_ard(ks.id))
    for (int k = 0; k < ks.n_params; ++k) g.p[k] = 1.0 / ks.p[k];
  return g;
}

// the factor of dk / dx*_c that pair_weight leaves out, without its sign and, for ARD, without the second 1 / l_c (the tail kernels
// multiply by the deriv spec's p[c]; sqrexp_ard's 1.0 * p[c] is p[c] exactly): ks is the caller's spec, not the derived one (it reads
// p[0] of the isotropic kernels and gammaexp's p[1], which make_deriv_spec keeps: the batched kernels call it on their derived record)
__host__ __device__ inline double deriv_tail_factor(const KernelSpec& ks) {
  const double il2 = 1.0 / (ks.p[0] * ks.p[0]);
  switch (ks.id) {
    case GPRC_GAMMAEXP: return ks.p[1];
    case GPRC_SQREXP_ARD: return 1.0;
    case GPRC_MATERN32: return 3.0 * il2;
    case GPRC_MATERN52: return 5.0 / 3.0 * il2;
    case GPRC_MATERN32_ARD: return 3.0;
    case GPRC_MATERN52_ARD: return 5.0 / 3.0;
    default: return il2;
  }
}

// ---- device --------------------------------------------------------------------------------------------------------------------
namespace {

// base R `^` for doubles (arithmetic.c R_POW / R_pow): x^2 is x*x, the rest is libm pow
__device__ __forceinline__ double r_pow(double x, double y) {
  if (y == 2.0) return x * x;
  if (x == 1.0 || y == 0.0) return 1.0;
  if (x == 0.0) return y > 0.0 ? 0.0 : (y < 0.0 ? __builtin_huge_val() : y);
  return pow(x, y);
}

// a p - b p as the contraction kernels form it from their staged coordinates: two rounded products, then the difference.  Contracted
// into fma(a, p, -(b p)) the difference of two equal points would be the rounding error of the product, not 0.  (The small-model kernels,
// small_model.h's sqdist and kernels_batch_predict.hip, scale their ARD coordinates with it: a test point equal to a training point is s = 0.)
__device__ __forceinline__ double bt_scaled_diff(double a, double b, double p) {
#pragma clang fp contract(off)
  const double ap = a * p, bp = b * p;
  return ap - bp;
}

// Coordinates r0 .. r0 + dc - 1 of the points g0 .. g0 + count - 1 of P (point-major, d coordinates each; zero from point npts on),
// by the 256 threads of the workgroup (t: the thread): store(i, r, value) for point i of the tile and coordinate r of the pass.
// SCALED: times scale[r0 + r] (ARD in the contraction kernels: the coordinates divided by their length scale).
template <bool SCALED, class Store>
__device__ __forceinline__ void stage_points(const double* P, int64_t g0, int64_t npts, int64_t d, int64_t r0, int dc, int count,
                                             const double* scale, int t, Store store) {
  for (int e = t; e < count * dc; e += 256) {
    const int i = e / dc, r = e - i * dc;
    const int64_t g = g0 + i;
    double v = (g < npts) ? P[g * d + r0 + r] : 0.0;
    if constexpr (SCALED) v *= scale[r0 + r];
    store(i, r, v);
  }
}

// s0[c] / s1[c] += (a - b)^2 over the dc staged coordinates, for the lane's two rows and its wave's 16 columns
__device__ __forceinline__ void accum_sqdist(const double (&As)[PT_D][PT_R], const double (&Bs)[PT_C][PT_D + 1], int dc, int lane, int wave,
                                             double (&s0)[16], double (&s1)[16]) {
  for (int r = 0; r < dc; ++r) {
    const double2 av = *reinterpret_cast<const double2*>(&As[r][2 * lane]);
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const double b = Bs[wave * 16 + c][r];
      const double t0 = av.x - b, t1 = av.y - b;
      s0[c] = fma(t0, t0, s0[c]);
      s1[c] = fma(t1, t1, s1[c]);
    }
  }
}

// its sibling, ARD's second pass: sum over the lane's 32 pairs of w * (a - b)^2 for the ONE staged coordinate r, columns ascending
__device__ __forceinline__ double weighted_sqdiff(const double (&As)[PT_D][PT_R], const double (&Bs)[PT_C][PT_D + 1], int r, int lane, int wave,
                                                  const double (&w0)[16], const double (&w1)[16]) {
  const double2 av = *reinterpret_cast<const double2*>(&As[r][2 * lane]);
  double acc = 0.0;
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    const double b = Bs[wave * 16 + c][r];
    const double t0 = av.x - b, t1 = av.y - b;
    acc = fma(w0[c], t0 * t0, acc);
    acc = fma(w1[c], t1 * t1, acc);
  }
  return acc;
}

// h of dk(x*, x_j) / dx*_c = -h (x*_c - x_jc) t_c from the squared distance s, WITHOUT the factor that does not depend on the pair
// (deriv_tail_factor): the weight of kernels_pgrad.hip's contraction and of kernels_paths.hip's gradient product
template <int KID>
__device__ __forceinline__ double pair_weight(double s, const KernelSpec& ks) {
  if constexpr (KID == GPRC_SQREXP) return exp(-s * ks.p[1]);        // p[1] = 1 / (2 l^2)
  else if constexpr (KID == GPRC_SQREXP_ARD) return exp(-0.5 * s);   // s is the scaled distance
  else if constexpr (is_matern(KID)) {                               // p[1] = 3 / l^2 or 5 / l^2; ARD: s is the scaled distance
    const double a = sqrt(is_ard(KID) ? (is_matern32(KID) ? 3.0 : 5.0) * s : s * ks.p[1]), e = exp(-a);
    if constexpr (is_matern32(KID)) return e;
    else return fma(a, e, e);
  } else if constexpr (KID == GPRC_GAMMAEXP) {
    if (!(s > 0.0)) return 0.0;                                      // the limit for gamma > 1, the convention for gamma <= 1
    const double u = exp(ks.p[3] * log(s * ks.p[2]));                // p[2] = 1 / l^2, p[3] = gamma / 2
    return exp(-u) * u / s;
  } else {                                                           // rationalquadratic: p[1] = alpha, p[2] = 1 / (2 alpha l^2)
    const double x = s * ks.p[2];
    return exp(-ks.p[1] * log1p(x)) / (1.0 + x);
  }
}

// k from the squared distance s (ARD: the scaled one), constants from make_deriv_spec: the value of the generated-operand products
// (kernels_paths.hip) and of the pivoted Cholesky's columns (kernels_cg.hip); not the fill's finish<KID>, see the head of this file
template <int KID>
__device__ __forceinline__ double kernel_value(double s, const KernelSpec& ks) {
  if constexpr (KID == GPRC_SQREXP) return exp(-s * ks.p[1]);        // p[1] = 1 / (2 l^2)
  else if constexpr (KID == GPRC_SQREXP_ARD) return exp(-0.5 * s);
  else if constexpr (is_matern(KID)) {                               // p[1] = 3 / l^2 or 5 / l^2
    const double a = sqrt(is_ard(KID) ? (is_matern32(KID) ? 3.0 : 5.0) * s : s * ks.p[1]), e = exp(-a);
    if constexpr (is_matern32(KID)) return fma(a, e, e);
    else return fma(a * a, 1.0 / 3.0, 1.0 + a) * e;
  } else if constexpr (KID == GPRC_GAMMAEXP) {
    if (!(s > 0.0)) return 1.0;
    return exp(-exp(ks.p[3] * log(s * ks.p[2])));                    // p[2] = 1 / l^2, p[3] = gamma / 2
  } else {                                                           // rationalquadratic: p[1] = alpha, p[2] = 1 / (2 alpha l^2)
    return exp(-ks.p[1] * log1p(s * ks.p[2]));
  }
}

// the weight of a pair in dk / dtheta and in dk / dz, with the theta integrands that hang on it, WITHOUT the factors that do not depend on
// the pair (the table at the head of kernels_sgrad.hip): kernels_sgrad.hip's contraction over a stored G and kernels_igrad.hip's over a
// low-rank one
struct PairW { double h, hs, h2; };   // the weight, the first theta integrand (isotropic kernels), the second (gammaexp, ratquad)

template <int KID>
__device__ __forceinline__ PairW cross_weight(double s, const KernelSpec& ks) {
  if constexpr (KID == GPRC_SQREXP) {
    const double h = exp(-s * ks.p[1]);                               // p[1] = 1 / (2 l^2)
    return {h, h * s, 0.0};
  } else if constexpr (KID == GPRC_SQREXP_ARD) {
    return {exp(-0.5 * s), 0.0, 0.0};                                 // s is the scaled distance
  } else if constexpr (is_matern(KID)) {                              // p[1] = 3 / l^2 or 5 / l^2; ARD: s is the scaled distance
    const double a = sqrt(is_ard(KID) ? (is_matern32(KID) ? 3.0 : 5.0) * s : s * ks.p[1]), e = exp(-a);
    const double h = is_matern32(KID) ? e : fma(a, e, e);
    return {h, h * s, 0.0};
  } else if constexpr (KID == GPRC_GAMMAEXP) {                        // s > 0 (the caller skips s = 0: the limit for gamma > 1, the convention for gamma <= 1)
    const double lg = log(s * ks.p[2]), u = exp(ks.p[3] * lg), ku = exp(-u) * u;   // p[2] = 1 / l^2, p[3] = gamma / 2
    return {ku / s, ku, ku * lg};
  } else {                                                            // rationalquadratic: p[1] = alpha, p[2] = 1 / (2 alpha l^2)
    const double x = s * ks.p[2], q = 1.0 + x, lq = log1p(x), h = exp(-ks.p[1] * lq) / q;
    return {h, h * s, h * (x - q * lq)};
  }
}

// what one pair of squared distance s and weight gij adds to the theta sums: gammaexp skips s = 0 (its weight and both integrands are 0
// there) and takes hs and h2; the ARD kernels park gij h in `keep` for their second pass over the coordinates; ratquad takes hs and h2;
// everyone else hs.  kernels_batch.hip, kernels_vecchia.hip and kernels_igrad.hip: the three differ in where `keep` lives.
template <int KID>
__device__ __forceinline__ void theta_terms(double gij, double s, const KernelSpec& ks, double& a0, double& a1, double& keep) {
  if constexpr (KID == GPRC_GAMMAEXP) {
    if (s > 0.0) {
      const PairW pw = cross_weight<KID>(s, ks);
      a0 = fma(gij, pw.hs, a0);
      a1 = fma(gij, pw.h2, a1);
    }
  } else {
    const PairW pw = cross_weight<KID>(s, ks);
    if constexpr (is_ard(KID)) {
      keep = gij * pw.h;
    } else {
      a0 = fma(gij, pw.hs, a0);
      if constexpr (KID == GPRC_RATQUAD) a1 = fma(gij, pw.h2, a1);
    }
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;  // lane 0 holds the sum
}

// the four waves' partials in a fixed order, the two forms in use: pairwise (the scalar sums of the gradients) and in wave order
// (the fused predict epilogues, whose partials are also summed tile after tile in order)
__device__ __forceinline__ double sum4_pairs(double w0, double w1, double w2, double w3) { return (w0 + w1) + (w2 + w3); }
__device__ __forceinline__ double sum4_in_order(double w0, double w1, double w2, double w3) { return ((w0 + w1) + w2) + w3; }

}  // namespace

}  // namespace gprc
