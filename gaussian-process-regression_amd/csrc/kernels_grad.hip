// kernels_grad.hip -- the contraction of the exact marginal-likelihood gradient for gfx950 (gprc_gpr_logp_grad).
//
//   d logp / d theta = 1/2 sum_ij M_ij dK_ij / d theta,     M = alpha alpha^T - K_y^-1,  K_y = K + noise I
//
// K_y^-1 arrives as W = -K_y^-1 (the inverse GEMM subtracts from a zeroed matrix), lower triangle stored.  One pass reads that
// triangle -- 8 B per element, 16 B per lane, 1 KiB contiguous per wave and column, the only HBM traffic -- in the fill's tile
// shape (128 x 64, two rows x 16 columns per lane); K_ij and dK_ij / d theta are recomputed from X through LDS exactly as the fill
// forms them, so no derivative array and no second kernel matrix exists.  Off-diagonal entries count twice (symmetry), entries
// above the diagonal or in the padding not at all; the diagonal also carries d / d noise = 1/2 sum_i M_ii.
//
// What the device leaves per parameter is the sum WITHOUT the factors that do not depend on (i, j); the host applies them:
//   sqrexp        sum M K s                     (x 1 / l^3)                  s = |x - y|^2
//   gammaexp      sum M K u, sum M K u L        (x gamma / l, x -1/2)        u = (s / l^2)^(gamma / 2), L = log(s / l^2); 0 at s = 0
//   ratquad       sum M K s / q, sum M K (x / q - log q)   (x 1 / l^3, x 1)  x = s / (2 alpha l^2), q = 1 + x
//   sqrexp_ard    sum M K t_k^2  per k          (x 1 / l_k)                  t_k = (x_k - y_k) / l_k
//   matern32      sum M e^-a u                  (x 1 / l)                    u = 3 s / l^2, a = sqrt(u)         (dK / dl = 3 e^-a s / l^3)
//   matern52      sum M (1 + a) e^-a u          (x 1 / (3 l))                u = 5 s / l^2, a = sqrt(u)         (dK / dl = 5/3 (1 + a) e^-a s / l^3)
//   matern32_ard  sum M e^-a t_k^2  per k       (x 3 / l_k)                  a = sqrt(3 sum_k t_k^2)
//   matern52_ard  sum M (1 + a) e^-a t_k^2      (x 5 / (3 l_k))              a = sqrt(5 sum_k t_k^2)
// (no 1 / r anywhere in the Matern derivatives: s = 0 needs no convention.)
// For ARD a lane keeps M K of its 32 elements in registers and passes over the coordinates a second time, 16 at a time: the d sums
// never live in registers at once (d <= 256), and nothing of size n x d is formed.
//
// Order of summation is fixed: a lane's elements in column order, the 64 lanes by a shuffle tree, the four waves in wave order, a
// workgroup's tiles in tile order (a fixed grid strides over the tile list), the workgroups by the host in long double.  No atomics:
// two calls on the same input give the same bits.
//
// The LAPLACE variant (gprc_gpc_logq_grad, DESIGN.md "GPC evidence gradient") is the same pass over W = -B^-1, B = I + sw K sw, with
//   M_ij = a_i a_j + sw_i sw_j W_ij + u_i g_j + u_j g_i
// (explicit part a a^T - R, R = sw B^-1 sw, plus the rank-two form of the implicit part through the mode).  A tile stages the four
// vectors of its 128 rows and 64 columns in LDS (6 KiB) and reads them there inside the column loop; there is no diagonal sum.
// It is a compile-time parameter: the regression instantiations are the code they were.
//
// The tile shape, the staging and both distance loops are pair_tile.h's.  Also here: the derivative row sums of the reference's own
// fit() gradient (gprc_fit_gradient), the other consumer of dK / dtheta.
#include "pair_tile.h"

#include <algorithm>

namespace gprc {

namespace {

constexpr int GRAD_WGS = 1024; // workgroups of the launch = rows of the partial buffer (a constant: the order of summation does not depend on the device)

struct GradArgs {
  const double* X;
  const double* alpha;
  const double* W;
  double* part;
  int64_t n, d, ld;
  int64_t ntiles;
  KernelSpec ks;   // derived constants, see make_deriv_spec
};
struct LaplaceArgs : GradArgs {   // alpha: the mode search's a = K^-1 f
  const double* sw;
  const double* u;
  const double* g;
};

template <int KID, bool LAPLACE>
__global__ __launch_bounds__(256) void grad_contract_kernel(std::conditional_t<LAPLACE, LaplaceArgs, GradArgs> a) {
  __shared__ __attribute__((aligned(16))) double As[PT_D][PT_R];
  __shared__ double Bs[PT_C][PT_D + 1];
  __shared__ double Al[PT_C];
  __shared__ double red[4][PT_D + 1];
  __shared__ double gacc[MAX_PARAMS + 1];
  __shared__ __attribute__((aligned(16))) double Rv[LAPLACE ? 4 : 1][PT_R];   // Laplace: a, sw, u, g of the tile's rows ...
  __shared__ double Cv[LAPLACE ? 4 : 1][PT_C];                                 // ... and of its columns
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int np = is_ard(KID) ? (int)a.d : ((KID == GPRC_SQREXP || is_matern(KID)) ? 1 : 2);
  constexpr int NZ = LAPLACE ? 0 : 1;   // regression leaves one more sum per workgroup, the diagonal's
  for (int k = t; k <= np; k += 256) gacc[k] = 0.0;
  double a0 = 0.0, a1 = 0.0, nz = 0.0;  // isotropic kernels: this lane's sums over all its tiles; nz: the diagonal's M_ii

  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    // row tile bi holds the column tiles 0 .. 2 bi + 1 (everything that touches the lower triangle): tiles before it = bi (bi + 1)
    int64_t bi = (int64_t)((sqrt(4.0 * (double)tile + 1.0) - 1.0) * 0.5);
    while ((bi + 1) * (bi + 2) <= tile) ++bi;
    while (bi * (bi + 1) > tile) --bi;
    const int64_t bj = tile - bi * (bi + 1);
    const int64_t ti = bi * PT_R, tj = bj * PT_C;

    auto stage = [&](int64_t r0, int dc) {  // coordinates r0 .. r0 + dc - 1 of the tile's points (ARD: divided by their length scale)
      __syncthreads();
      stage_points<is_ard(KID)>(a.X, ti, a.n, a.d, r0, dc, PT_R, a.ks.p, t, [&](int i, int r, double v) { As[r][i] = v; });
      stage_points<is_ard(KID)>(a.X, tj, a.n, a.d, r0, dc, PT_C, a.ks.p, t, [&](int j, int r, double v) { Bs[j][r] = v; });
      if constexpr (LAPLACE) {
        if (r0 == 0) {
          const int v = t >> 6, j = t & 63;   // 4 vectors x 64 columns; 4 x 128 rows, two per thread
          const double* src = v == 0 ? a.alpha : (v == 1 ? a.sw : (v == 2 ? a.u : a.g));
          Cv[v][j] = (tj + j < a.n) ? src[tj + j] : 0.0;
          Rv[v][j] = (ti + j < a.n) ? src[ti + j] : 0.0;
          Rv[v][j + 64] = (ti + j + 64 < a.n) ? src[ti + j + 64] : 0.0;
        }
      } else {
        if (r0 == 0 && t < PT_C) Al[t] = (tj + t < a.n) ? a.alpha[tj + t] : 0.0;
      }
      __syncthreads();
    };

    double s0[16], s1[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) { s0[c] = 0.0; s1[c] = 0.0; }
    for (int64_t r0 = 0; r0 < a.d; r0 += PT_D) {
      const int dc = (int)((a.d - r0 < PT_D) ? (a.d - r0) : PT_D);
      stage(r0, dc);
      accum_sqdist(As, Bs, dc, lane, wave, s0, s1);
    }

    const int64_t gi0 = ti + 2 * lane;
    const double al0 = (!LAPLACE && gi0 < a.n) ? a.alpha[gi0] : 0.0, al1 = (!LAPLACE && gi0 + 1 < a.n) ? a.alpha[gi0 + 1] : 0.0;
    // rows < 128 ceil(n / 128) <= n_pad and columns <= 64 (2 bi + 1) + 63 < 128 (bi + 1): every load is inside the n_pad x n_pad matrix
    const double* wp = a.W + gi0 + (tj + wave * 16) * a.ld;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const int64_t gj = tj + wave * 16 + c;
      const double2 w = *reinterpret_cast<const double2*>(wp + c * a.ld);
      const double alj = LAPLACE ? 0.0 : Al[wave * 16 + c];
      double m0 = fma(al0, alj, w.x), m1 = fma(al1, alj, w.y);
      const bool jin = gj < a.n;
      if constexpr (LAPLACE) {   // a_i a_j + sw_i sw_j W_ij + u_i g_j + u_j g_i, the eight vector entries from LDS
        const int cj = wave * 16 + c;
        const double2 ra = *reinterpret_cast<const double2*>(&Rv[0][2 * lane]), rs = *reinterpret_cast<const double2*>(&Rv[1][2 * lane]);
        const double2 ru = *reinterpret_cast<const double2*>(&Rv[2][2 * lane]), rg = *reinterpret_cast<const double2*>(&Rv[3][2 * lane]);
        const double aj = Cv[0][cj], sj = Cv[1][cj], uj = Cv[2][cj], gj_ = Cv[3][cj];
        m0 = fma(ra.x, aj, (rs.x * sj) * w.x) + fma(ru.x, gj_, uj * rg.x);
        m1 = fma(ra.y, aj, (rs.y * sj) * w.y) + fma(ru.y, gj_, uj * rg.y);
      } else {
        if (jin && gi0 == gj) nz += m0;
        if (jin && gi0 + 1 == gj) nz += m1;
      }
      m0 = (jin && gi0 < a.n && gi0 > gj) ? 2.0 * m0 : 0.0;          // the diagonal's dK / d theta is zero for all four kernels
      m1 = (jin && gi0 + 1 < a.n && gi0 + 1 > gj) ? 2.0 * m1 : 0.0;
      if constexpr (KID == GPRC_SQREXP) {
        const double h = a.ks.p[1];  // 1 / (2 l^2)
        a0 = fma(m0 * exp(-s0[c] * h), s0[c], a0);
        a0 = fma(m1 * exp(-s1[c] * h), s1[c], a0);
      } else if constexpr (KID == GPRC_SQREXP_ARD) {
        s0[c] = m0 * exp(-0.5 * s0[c]);  // M K, kept for the second pass
        s1[c] = m1 * exp(-0.5 * s1[c]);
      } else if constexpr (KID == GPRC_MATERN32 || KID == GPRC_MATERN52) {
        const double h = a.ks.p[1];  // 3 / l^2, 5 / l^2
        const double u0 = s0[c] * h, u1 = s1[c] * h, q0 = sqrt(u0), q1 = sqrt(u1), e0 = exp(-q0), e1 = exp(-q1);
        a0 = fma(m0 * (KID == GPRC_MATERN32 ? e0 : fma(q0, e0, e0)), u0, a0);
        a0 = fma(m1 * (KID == GPRC_MATERN32 ? e1 : fma(q1, e1, e1)), u1, a0);
      } else if constexpr (is_matern(KID)) {  // ARD: M g~ kept for the second pass; s is the scaled distance
        constexpr double nu2 = is_matern32(KID) ? 3.0 : 5.0;
        const double q0 = sqrt(nu2 * s0[c]), q1 = sqrt(nu2 * s1[c]), e0 = exp(-q0), e1 = exp(-q1);
        s0[c] = m0 * (is_matern32(KID) ? e0 : fma(q0, e0, e0));
        s1[c] = m1 * (is_matern32(KID) ? e1 : fma(q1, e1, e1));
      } else if constexpr (KID == GPRC_GAMMAEXP) {
        const double rl2 = a.ks.p[2], hg = a.ks.p[3];  // 1 / l^2, gamma / 2
        if (s0[c] > 0.0) {
          const double lg = log(s0[c] * rl2), u = exp(hg * lg), ku = m0 * exp(-u) * u;
          a0 += ku;
          a1 = fma(ku, lg, a1);
        }
        if (s1[c] > 0.0) {
          const double lg = log(s1[c] * rl2), u = exp(hg * lg), ku = m1 * exp(-u) * u;
          a0 += ku;
          a1 = fma(ku, lg, a1);
        }
      } else {  // rationalquadratic
        const double al = a.ks.p[1], rc = a.ks.p[2];  // alpha, 1 / (2 alpha l^2)
        {
          const double x = s0[c] * rc, q = 1.0 + x, lq = log1p(x), k = m0 * exp(-al * lq);
          a0 = fma(k, s0[c] / q, a0);
          a1 = fma(k, x / q - lq, a1);
        }
        {
          const double x = s1[c] * rc, q = 1.0 + x, lq = log1p(x), k = m1 * exp(-al * lq);
          a0 = fma(k, s1[c] / q, a0);
          a1 = fma(k, x / q - lq, a1);
        }
      }
    }

    if constexpr (is_ard(KID)) {
      for (int64_t r0 = 0; r0 < a.d; r0 += PT_D) {
        const int dc = (int)((a.d - r0 < PT_D) ? (a.d - r0) : PT_D);
        if (a.d > PT_D) stage(r0, dc);  // (d <= 16: the only chunk is still in LDS)
        for (int r = 0; r < dc; ++r) {
          const double acc = wave_sum(weighted_sqdiff(As, Bs, r, lane, wave, s0, s1));
          if (lane == 0) red[wave][r] = acc;
        }
        __syncthreads();
        if (t < dc) gacc[r0 + t] += sum4_pairs(red[0][t], red[1][t], red[2][t], red[3][t]);
        if (a.d <= PT_D) __syncthreads();  // (otherwise the next stage() separates these reads from the next chunk's writes)
      }
    }
  }

  a0 = wave_sum(a0);
  a1 = wave_sum(a1);
  if constexpr (!LAPLACE) nz = wave_sum(nz);
  __syncthreads();
  if (lane == 0) { red[wave][0] = a0; red[wave][1] = a1; red[wave][2] = nz; }
  __syncthreads();
  if (t == 0) {
    if constexpr (!is_ard(KID)) {
      gacc[0] = sum4_pairs(red[0][0], red[1][0], red[2][0], red[3][0]);
      if (np == 2) gacc[1] = sum4_pairs(red[0][1], red[1][1], red[2][1], red[3][1]);
    }
    if constexpr (!LAPLACE) gacc[np] = sum4_pairs(red[0][2], red[1][2], red[2][2], red[3][2]);
  }
  __syncthreads();
  for (int k = t; k < np + NZ; k += 256) a.part[(int64_t)blockIdx.x * (np + NZ) + k] = gacc[k];
}

// One launcher behind both public ones: they differ in the argument struct, the width of a partial row (regression: one more sum, the
// diagonal's), the profile kind and its flop / byte constants.  a: everything but ntiles and ks.
template <bool LAPLACE>
int launch_contract(hipStream_t s, const KernelSpec& ks, std::conditional_t<LAPLACE, LaplaceArgs, GradArgs> a) {
  const std::string who = LAPLACE ? "gpc_grad_contract" : "grad_contract";
  if (a.n <= 0) return 0;
  if ((a.ld & 1) || (reinterpret_cast<uintptr_t>(a.W) & 15)) { set_error(who + ": the inverse must be 16-byte aligned with an even leading dimension"); return GPRC_ERR_ARG; }
  const int64_t R = (a.n + PT_R - 1) / PT_R;
  if (a.ld < R * PT_R) { set_error(who + ": leading dimension smaller than the padded size"); return GPRC_ERR_ARG; }
  GPRC_TRY(check_grad_kernel(LAPLACE ? "logq_grad" : "logp_grad", ks.id));
  a.ntiles = R * (R + 1);
  a.ks = make_deriv_spec(ks);
  GPRC_HIP(hipMemsetAsync(a.part, 0, sizeof(double) * (size_t)(GRAD_WGS * (ks.n_params + (LAPLACE ? 0 : 1))), s));   // rows of workgroups that are not launched
  const dim3 grid((unsigned)std::min<int64_t>(a.ntiles, GRAD_WGS)), block(256);
  // bytes: the stored triangle once + X and alpha (Laplace: four vectors); flops: the distance (3 d), the kernel and its derivatives
  // (~60; Laplace: the 9 of M more), ARD's second pass (4 d)
  const double elems = 0.5 * (double)a.n * (double)(a.n + 1), n = (double)a.n, d = (double)a.d;
  ProfScope ps(s, LAPLACE ? PK_GPC_GRAD_CONTRACT : PK_GRAD_CONTRACT, elems * (3.0 * d + (LAPLACE ? 69.0 : 60.0) + (is_ard(ks.id) ? 4.0 * d : 0.0)),
               8.0 * (elems + n * d + (LAPLACE ? 4.0 * n : n)));
  with_gradient_kernel(ks.id, [&](auto kid) { hipLaunchKernelGGL((grad_contract_kernel<decltype(kid)::value, LAPLACE>), grid, block, 0, s, a); });
  GPRC_LAUNCH_CHECK();
  return 0;
}

// ---- derivative row sums for fit()'s gradient (R/fit.R:126-139) ---------------------------------------------------
// deriv(x, y, v...) of cov_dict (R/fit.R:4-31), with v bound POSITIONALLY as the reference's do.call does:
//   sqrexp (l)            r = |x-y| :  r^2/l^3 * exp(-r^2/(2 l^2))
//   gammaexp (gamma, l)   r = |x-y| :  ( -exp(-(r/l)^gamma) (r/l)^gamma log(r/l) ,  exp(-(r/l)^gamma) gamma r^gamma / l^(gamma+1) )
//   polynomial (sigma, p) s = x.y + sigma :  ( p s^(p-1) ,  s^p log(s) )
//   rationalquadratic (alpha, l)  r = |x-y|^2, q = r/(2 l^2 alpha) + 1 :
//                         ( q^-alpha (r - (2 l^2 alpha + r) log q) / (2 l^2 alpha + r) ,  r q^(-alpha-1) / l^3 )
// (gammaexp's first component is 0 * -Inf = NaN at r = 0, i.e. on the diagonal: kept, it decides what optim does.)
template <int KID>
__device__ __forceinline__ void deriv_pair(double s, double v0, double v1, double& g0, double& g1) {
  if constexpr (KID == GPRC_SQREXP) {
    g0 = s / (v0 * v0 * v0) * exp(-s / ((v0 * v0) * 2.0));
    g1 = 0.0;
  } else if constexpr (KID == GPRC_GAMMAEXP) {
    const double r = sqrt(s), rl = r / v1, e = exp(-r_pow(rl, v0));
    g0 = -e * r_pow(rl, v0) * log(rl);
    g1 = e * v0 * r_pow(r, v0) / r_pow(v1, v0 + 1.0);
  } else if constexpr (KID == GPRC_POLYNOMIAL) {
    const double t = s + v0;
    g0 = v1 * r_pow(t, v1 - 1.0);
    g1 = r_pow(t, v1) * log(t);
  } else {  // rationalquadratic
    const double c = 2.0 * (v1 * v1) * v0, q = s / c + 1.0;
    g0 = (r_pow(q, -v0) * (s - (c + s) * log(q))) / (c + s);
    g1 = (s * r_pow(q, -v0 - 1.0)) / (v1 * v1 * v1);
  }
}

template <int KID>
__global__ __launch_bounds__(256) void deriv_rowsum_kernel(double v0, double v1, const double* X, int64_t d, int64_t n, double* S) {
  const int64_t r = blockIdx.x;
  const double* xr = X + r * d;
  double a0 = 0.0, a1 = 0.0;
  for (int64_t c = threadIdx.x; c < n; c += 256) {
    const double* xc = X + c * d;
    double s = 0.0;
    for (int64_t k = 0; k < d; ++k) {
      if constexpr (KID == GPRC_POLYNOMIAL) s += xr[k] * xc[k];
      else { const double t = xr[k] - xc[k]; s += t * t; }
    }
    double g0, g1;
    deriv_pair<KID>(s, v0, v1, g0, g1);
    a0 += g0;
    a1 += g1;
  }
  __shared__ double red[2][4];
  a0 = wave_sum(a0);
  a1 = wave_sum(a1);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a0; red[1][threadIdx.x >> 6] = a1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    S[r] = sum4_pairs(red[0][0], red[0][1], red[0][2], red[0][3]);
    if (KID != GPRC_SQREXP) S[n + r] = sum4_pairs(red[1][0], red[1][1], red[1][2], red[1][3]);
  }
}

}  // namespace

int64_t grad_partial_rows() { return GRAD_WGS; }

int launch_grad_contract(hipStream_t s, const KernelSpec& ks, const double* X, int64_t d, int64_t n, const double* alpha, const double* W,
                         int64_t ld, double* part) {
  return launch_contract<false>(s, ks, GradArgs{X, alpha, W, part, n, d, ld, 0, {}});
}

int launch_gpc_grad_contract(hipStream_t s, const KernelSpec& ks, const double* X, int64_t d, int64_t n, const double* a_vec, const double* sw,
                             const double* u, const double* g, const double* W, int64_t ld, double* part) {
  return launch_contract<true>(s, ks, LaplaceArgs{{X, a_vec, W, part, n, d, ld, 0, {}}, sw, u, g});
}

int launch_deriv_rowsum(hipStream_t s, int kernel, double v0, double v1, const double* X, int64_t d, int64_t n, double* S) {
  if (n <= 0) return 0;
  ProfScope ps(s, PK_DERIV, (double)n * n * (3.0 * d + 40.0), 8.0 * ((double)n * d + 2.0 * n));
  if (!with_kernel_id<GPRC_SQREXP, GPRC_GAMMAEXP, GPRC_POLYNOMIAL, GPRC_RATQUAD>(kernel, [&](auto kid) {
        hipLaunchKernelGGL((deriv_rowsum_kernel<decltype(kid)::value>), dim3((unsigned)n), dim3(256), 0, s, v0, v1, X, d, n, S);
      })) {
    set_error("fit gradient: the reference defines it for sqrexp, gammaexp, polynomial, rationalquadratic only (R/fit.R:125)");
    return GPRC_ERR_ARG;
  }
  GPRC_LAUNCH_CHECK();
  return 0;
}

}  // namespace gprc
