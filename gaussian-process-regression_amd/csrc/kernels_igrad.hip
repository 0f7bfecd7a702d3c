// kernels_igrad.hip -- the low-rank-weighted contraction of the iterative GPR's evidence gradient for gfx950 (gprc_igpr_logp_grad,
// gprc_dev_lowrank_grad; DESIGN.md section 7, "Iterative GPR evidence"): kernels_sgrad.hip's contraction with a weight that is never stored,
//
//   sums_k = sum_{i, j < n} (sum_{r < R} A[i, r] B[j, r]) dk(x_i, x_j) / d theta_k          A, B: n x R, column-major, R <= IG_RMAX
//
// in O(n^2 (R + d)) work and O(n R) memory, and the vector kernels around it (the probes, the column dots).
//
// One tile of point pairs is IG_R x IG_C = 64 x 64 per 256-thread workgroup: wave w owns rows 16 w .. 16 w + 15 and the four 16 x 16
// sub-tiles beside each other.  The weight of a sub-tile is one accumulator of v_mfma_f64_16x16x4_f64 over r in groups of four (operand:
// one double per lane, (index lane & 15, r = lane >> 4), straight from A and B; rows >= n and r >= R are exact zeros), and the
// accumulator's layout -- col = lane & 15, row = (lane >> 4) + 4 reg -- decides which four pairs of a sub-tile a lane owns: it forms
// their squared distances from the points in LDS (PT_D coordinates at a time, as everywhere else) and the theta integrands of
// cross_weight (pair_tile.h; theta_terms adds them up) in place, so the weight makes no trip through LDS or HBM.  The ARD kernels' per-coordinate sums take
// kernels_grad.hip's second coordinate pass, d <= 256.  What the device leaves is the sum WITHOUT the factors that do not depend on
// (i, j): cross_grad_finish (kernels_sgrad.hip) applies them.  gammaexp's weight is 0 at s = 0.
//
// Order of summation, fixed: the MFMA's own chain over r ascending; a lane's sixteen pairs of a tile (sub-tile, then register,
// ascending) and its tiles down the stripe in one fma chain; the 64 lanes by a shuffle tree; the four waves pairwise; one partial per
// workgroup (stripe of row tiles x column tile); the partials in workgroup order by the host in long double.  (ARD: the tree and the
// four waves per tile and coordinate, the tiles of the stripe added in order.)  The stripe length is a function of n alone.  No
// atomics, no scratch: two calls give the same bits.
#include "pair_tile.h"

namespace gprc {

namespace {

constexpr int IG_R = 64;             // tile rows: 16 per wave
constexpr int IG_C = 64;             // tile columns: four 16-wide sub-tiles per wave
constexpr int IG_SUB = IG_C / 16;
constexpr int IG_MAX_STRIPES = 32;   // row stripes of a launch

typedef double v4d __attribute__((ext_vector_type(4)));

struct IgradArgs {
  const double* X;   // d x n, the points
  const double* A;   // n x R, pitch lda: the row side of the weight
  const double* B;   // n x R, pitch ldb: the column side
  double* part;      // (stripes x column tiles) x np sums
  int64_t n, d, lda, ldb, R;
  int64_t stripe_tiles, ntiles;   // 64-row tiles per stripe, in all
  KernelSpec ks;     // derived constants, see make_deriv_spec
};

template <int KID>
__global__ __launch_bounds__(256) void lowrank_grad_kernel(IgradArgs a) {
  __shared__ double As[PT_D][IG_R];
  __shared__ double Bs[IG_C][PT_D + 1];
  __shared__ double red[4][PT_D + 1];
  __shared__ double gacc[MAX_PARAMS];
  constexpr bool ARD = is_ard(KID);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lc = lane & 15, lr = lane >> 4;
  const int np = ARD ? (int)a.d : ((KID == GPRC_SQREXP || is_matern(KID)) ? 1 : 2);
  const int64_t tj = (int64_t)blockIdx.x * IG_C;
  const int64_t stripe = blockIdx.y;
  const int64_t tile0 = stripe * a.stripe_tiles;
  const int64_t tile1 = (tile0 + a.stripe_tiles < a.ntiles) ? tile0 + a.stripe_tiles : a.ntiles;
  if constexpr (ARD)
    for (int k = t; k < np; k += 256) gacc[k] = 0.0;
  double a0 = 0.0, a1 = 0.0;   // isotropic kernels: this lane's theta sums over its stripe

  for (int64_t tile = tile0; tile < tile1; ++tile) {
    const int64_t ti = tile * IG_R;
    // the weight of the lane's sixteen pairs: w[sub][reg] = sum_r A[ti + 16 wave + lr + 4 reg, r] B[tj + 16 sub + lc, r]
    v4d w[IG_SUB];
#pragma unroll
    for (int sub = 0; sub < IG_SUB; ++sub) w[sub] = v4d{0.0, 0.0, 0.0, 0.0};
    const int64_t ai = ti + wave * 16 + lc;
    for (int64_t r0 = 0; r0 < a.R; r0 += 4) {
      const int64_t r = r0 + lr;
      const bool rin = r < a.R;
      const double av = (rin && ai < a.n) ? a.A[ai + r * a.lda] : 0.0;   // the padding of n and of R: exact zeros
#pragma unroll
      for (int sub = 0; sub < IG_SUB; ++sub) {
        const int64_t bj = tj + sub * 16 + lc;
        const double bv = (rin && bj < a.n) ? a.B[bj + r * a.ldb] : 0.0;
        w[sub] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, w[sub], 0, 0, 0);
      }
    }

    // coordinates r0 .. r0 + dc - 1 of the tile's points (ARD: divided by their length scale); the column points are the same for every
    // tile of the stripe, so for d <= 16 their only chunk is staged once
    auto stage = [&](int64_t r0, int dc) {
      __syncthreads();
      stage_points<ARD>(a.X, ti, a.n, a.d, r0, dc, IG_R, a.ks.p, t, [&](int i, int r, double v) { As[r][i] = v; });
      if (a.d > PT_D || tile == tile0) stage_points<ARD>(a.X, tj, a.n, a.d, r0, dc, IG_C, a.ks.p, t, [&](int j, int r, double v) { Bs[j][r] = v; });
      __syncthreads();
    };

    double s[IG_SUB][4];   // the squared distances, then (ARD) weight x h for the second pass
#pragma unroll
    for (int sub = 0; sub < IG_SUB; ++sub)
#pragma unroll
      for (int g = 0; g < 4; ++g) s[sub][g] = 0.0;
    for (int64_t r0 = 0; r0 < a.d; r0 += PT_D) {
      const int dc = (int)((a.d - r0 < PT_D) ? (a.d - r0) : PT_D);
      stage(r0, dc);
      for (int r = 0; r < dc; ++r) {
        double xr[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) xr[g] = As[r][wave * 16 + lr + 4 * g];
#pragma unroll
        for (int sub = 0; sub < IG_SUB; ++sub) {
          const double b = Bs[sub * 16 + lc][r];
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const double df = xr[g] - b;
            s[sub][g] = fma(df, df, s[sub][g]);
          }
        }
      }
    }

#pragma unroll
    for (int sub = 0; sub < IG_SUB; ++sub)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        theta_terms<KID>(w[sub][g], s[sub][g], a.ks, a0, a1, s[sub][g]);   // (ARD: weight x h takes the distance's place)

    if constexpr (ARD) {
      for (int64_t r0 = 0; r0 < a.d; r0 += PT_D) {
        const int dc = (int)((a.d - r0 < PT_D) ? (a.d - r0) : PT_D);
        if (a.d > PT_D) stage(r0, dc);   // (d <= 16: the only chunk is still in LDS)
        for (int r = 0; r < dc; ++r) {
          double xr[4];
#pragma unroll
          for (int g = 0; g < 4; ++g) xr[g] = As[r][wave * 16 + lr + 4 * g];
          double acc = 0.0;
#pragma unroll
          for (int sub = 0; sub < IG_SUB; ++sub) {
            const double b = Bs[sub * 16 + lc][r];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const double df = xr[g] - b;
              acc = fma(s[sub][g], df * df, acc);
            }
          }
          const double v = wave_sum(acc);
          if (lane == 0) red[wave][r] = v;
        }
        __syncthreads();
        if (t < dc) gacc[r0 + t] += sum4_pairs(red[0][t], red[1][t], red[2][t], red[3][t]);
        if (a.d <= PT_D) __syncthreads();   // (otherwise the next stage() separates these reads from the next chunk's writes)
      }
    }
  }

  if constexpr (!ARD) {
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
    __syncthreads();
    if (lane == 0) { red[wave][0] = a0; red[wave][1] = a1; }
    __syncthreads();
    if (t == 0) {
      gacc[0] = sum4_pairs(red[0][0], red[1][0], red[2][0], red[3][0]);
      if (np == 2) gacc[1] = sum4_pairs(red[0][1], red[1][1], red[2][1], red[3][1]);
    }
  }
  __syncthreads();
  for (int k = t; k < np; k += 256) a.part[(stripe * gridDim.x + blockIdx.x) * np + k] = gacc[k];
}

// sum over the workgroup's 256 threads, kernels_cg.hip's order: the 64 lanes by a butterfly, the four waves in wave order
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// out[s] = sum_i U[i + s ldu] V[i + s ldv]: row i to thread i mod 256, ascending, one fma chain a thread; one workgroup a column
__global__ __launch_bounds__(256) void col_dots_kernel(const double* U, int64_t ldu, const double* V, int64_t ldv, int64_t n, double* out) {
  __shared__ double red[4];
  const int64_t s = blockIdx.x;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) acc = fma(U[i + s * ldu], V[i + s * ldv], acc);
  const double q = block_sum(acc, red);
  if (threadIdx.x == 0) out[s] = q;
}

// Z[i + s ldz] = fma(sigma, G2[i + s ldg2], sum_{a < r} L[i + a n] G1[a + s ldg1]), a ascending in one fma chain; r = 0: Z = G2
__global__ __launch_bounds__(256) void probes_kernel(const double* L, int64_t r, const double* G1, int64_t ldg1, const double* G2, int64_t ldg2,
                                                     double sigma, int64_t n, int64_t T, double* Z, int64_t ldz) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t s = blockIdx.y;
  if (i >= n || s >= T) return;
  const double g2 = G2[i + s * ldg2];
  if (r == 0) { Z[i + s * ldz] = g2; return; }
  double acc = 0.0;
  for (int64_t c = 0; c < r; ++c) acc = fma(L[i + c * n], G1[c + s * ldg1], acc);
  Z[i + s * ldz] = fma(sigma, g2, acc);
}

int64_t stripe_tiles_of(int64_t ntiles) { return (ntiles + IG_MAX_STRIPES - 1) / IG_MAX_STRIPES; }

}  // namespace

int64_t lowrank_grad_wgs(int64_t n) {
  const int64_t ntiles = (n + IG_R - 1) / IG_R, st = stripe_tiles_of(ntiles);
  return ((ntiles + st - 1) / st) * ((n + IG_C - 1) / IG_C);
}

int launch_lowrank_grad(hipStream_t s, const KernelSpec& ks, const double* X, int64_t d, int64_t n, const double* A, int64_t lda, const double* B,
                        int64_t ldb, int64_t R, double* part) {
  GPRC_TRY(check_grad_kernel("lowrank_grad", ks.id));
  if (!X || !A || !B || !part || n < 1 || d < 1 || R < 1 || R > IG_RMAX || lda < n || ldb < n) {
    set_error("lowrank_grad: bad arguments (null pointer, n < 1, d < 1, R outside 1 .. 64, lda < n or ldb < n)");
    return GPRC_ERR_ARG;
  }
  const int64_t ntiles = (n + IG_R - 1) / IG_R, st = stripe_tiles_of(ntiles), stripes = (ntiles + st - 1) / st, ctiles = (n + IG_C - 1) / IG_C;
  if (ctiles > 0x7fffffff) { set_error("lowrank_grad: too many points"); return GPRC_ERR_ARG; }
  IgradArgs a{X, A, B, part, n, d, lda, ldb, R, st, ntiles, make_deriv_spec(ks)};
  // per pair: the weight (2 R, the padding of R to four included), the distance (3 d), the integrands (~40), ARD's second pass (4 d);
  // bytes: the points and both factors once per tile.  Counted with the exact gradient's contraction (the set of profiling kinds is fixed).
  const double pairs = (double)(ntiles * IG_R) * (double)(ctiles * IG_C);
  ProfScope ps(s, PK_GRAD_CONTRACT, pairs * (2.0 * (double)pad_up(R, 4) + 3.0 * d + 40.0 + (is_ard(ks.id) ? 4.0 * d : 0.0)),
               8.0 * pairs * ((double)(d + R) / IG_R + (double)(d + R) / IG_C));
  with_gradient_kernel(ks.id, [&](auto kid) {
    hipLaunchKernelGGL((lowrank_grad_kernel<decltype(kid)::value>), dim3((unsigned)ctiles, (unsigned)stripes), dim3(256), 0, s, a);
  });
  GPRC_LAUNCH_CHECK();
  return 0;
}

int launch_col_dots(hipStream_t s, const double* U, int64_t ldu, const double* V, int64_t ldv, int64_t n, int64_t S, double* out) {
  if (S <= 0) return 0;
  hipLaunchKernelGGL(col_dots_kernel, dim3((unsigned)S), dim3(256), 0, s, U, ldu, V, ldv, n, out);
  GPRC_LAUNCH_CHECK();
  return 0;
}

int launch_igpr_probes(hipStream_t s, const double* L, int64_t r, const double* G1, int64_t ldg1, const double* G2, int64_t ldg2, double sigma,
                       int64_t n, int64_t T, double* Z, int64_t ldz) {
  if (T <= 0) return 0;
  if (T > 65535) { set_error("igpr_probes: at most 65535 probes a call"); return GPRC_ERR_ARG; }
  hipLaunchKernelGGL(probes_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)T), dim3(256), 0, s, L, r, G1, ldg1, G2, ldg2, sigma, n, T, Z, ldz);
  GPRC_LAUNCH_CHECK();
  return 0;
}

}  // namespace gprc
