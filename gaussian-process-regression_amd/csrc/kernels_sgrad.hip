// kernels_sgrad.hip -- the contraction of the sparse GPR's bound gradient for gfx950 (gprc_sgpr_elbo_grad, gprc_dev_cross_grad): the
// rectangular sibling of kernels_grad.hip's grad_contract_kernel.
//
//   d elbo / d theta = sum_ij G_ij dk(a_i, z_j) / d theta            G: rows x cols, column-major with pitch ld (the chunk layout)
//   d elbo / d z_jc  = sum_i  G_ij dk(a_i, z_j) / d z_jc             dk(a, z) / d z_c = h(a, z) (a_c - z_c) t_c
//
// One pass reads G -- 8 B per element, 16 B per lane, 1 KiB contiguous per wave and column, the only HBM traffic of size rows x cols --
// in the fill's tile shape (128 x 64, two rows x 16 columns per lane); s_ij comes from A (d x rows) and Z (d x cols) through LDS as the
// fill forms it, ONE weight h per pair follows, and both outputs hang on it.  What the device leaves is, as in kernels_grad.hip, the sum
// WITHOUT the factors that do not depend on (i, j):
//                 weight h (device)                   theta sums                          host factor            dZ factor
//   sqrexp        K                                   sum G h s                           1 / l^3                1 / l^2
//   gammaexp      K u / s, u = (s / l^2)^(gamma / 2)  sum G K u, sum G K u L              gamma / l, -1/2        gamma         L = log(s / l^2); all 0 at s = 0
//   ratquad       K / q, q = 1 + x                    sum G h s, sum G h (x - q log q)    1 / l^3, 1             1 / l^2       x = s / (2 alpha l^2)
//   matern32      e^-a                                sum G h s                           3 / l^3                3 / l^2       a = sqrt(3 s) / l
//   matern52      (1 + a) e^-a                        sum G h s                           5 / (3 l^3)            5 / (3 l^2)   a = sqrt(5 s) / l
//   sqrexp_ard, matern32_ard, matern52_ard: the same h on coordinates staged divided by l_k; sum G h t_k^2 per k (t_k the scaled
//                 difference) and sum_i G h t_c per column; both get c / l_k, c = 1, 3, 5/3
// The difference a_c - z_c is formed directly, as in kernels_pgrad.hip.  gammaexp's weight is 0 at s = 0 (inducing points that ARE
// training points make such pairs routine); the Matern weights are finite there and the difference is 0.
//
// Who sums what.  A workgroup owns ONE 64-column tile of G, one STRIPE of 128-row tiles below each other and (WITH_Z) one group of
// SG_Z coordinates, and walks down its stripe.  The column sums over rows, which dZ wants, then stay in registers for the whole stripe
// -- 16 columns x SG_Z coordinates per lane, the lane's two rows added tile after tile -- and meet the other 63 lanes in one shuffle
// tree per (column, coordinate) at the END of the stripe, not once per tile: a wave owns its 16 columns alone, so no LDS and no second
// wave is involved.  (A shuffle tree per tile would cost 16 SG_Z trees for 32 pairs a lane; Z on the row side would want G transposed
// through 64 KiB of LDS.)  For d > SG_Z the further coordinate groups are further workgroups (blockIdx.z), each forming s and h again,
// as the prediction gradient does; only group 0 forms the theta sums.  ARD's per-coordinate theta sums take kernels_grad.hip's second
// coordinate pass, d <= 256.
//
// Order of summation, fixed: a lane's columns ascending and its tiles down the stripe; the 64 lanes by a shuffle tree; (theta) the four
// waves pairwise; one partial per (stripe, column tile) for theta and per (stripe, coordinate, column) for dZ; the stripes in order, by
// the host in long double (theta) and by cross_grad_sum_kernel (dZ).  The stripe length is a function of the padded row count alone.
// No atomics, no scratch: two calls give the same bits.  Rows >= rows and columns >= cols of G are never used, whatever they hold.
#include "pair_tile.h"

#include <algorithm>
#include <vector>

namespace gprc {

namespace {

// Coordinates whose column sums one workgroup forms: 16 x SG_Z running sums a lane, 96 registers beside the 64 of the distances.  Three
// is what the register file takes without scratch (profiles/sgpr_grad_isa.txt: four spills for every kernel at two waves per SIMD), and
// d <= 3 -- the spatial case -- is one group.
constexpr int SG_Z = 3;
constexpr int SG_MAX_STRIPES = 32;  // row stripes of a launch

struct SgradArgs {
  const double* G;    // rows_pad x cols_pad, pitch ld
  const double* A;    // d x rows, the row points
  const double* Z;    // d x cols, the column points
  double* part;       // (stripes x column tiles) x np theta sums
  double* pz;         // stripes x d x cols_pad column sums (WITH_Z)
  int64_t rows, cols, d, ld, cols_pad;
  int64_t stripe_tiles, ntiles;   // 128-row tiles per stripe, in all
  KernelSpec ks;      // derived constants, see make_deriv_spec
};

template <int KID, bool WITH_Z>
__global__ __launch_bounds__(256) void cross_grad_kernel(SgradArgs a) {
  __shared__ __attribute__((aligned(16))) double As[PT_D][PT_R];
  __shared__ double Bs[PT_C][PT_D + 1];
  __shared__ __attribute__((aligned(16))) double Az[WITH_Z ? SG_Z : 1][PT_R];   // the workgroup's own coordinates of the tile's row points ...
  __shared__ double Bz[WITH_Z ? PT_C : 1][SG_Z + 1];                             // ... and of its column points
  __shared__ double red[4][PT_D + 1];
  __shared__ double gacc[MAX_PARAMS];
  constexpr bool ARD = is_ard(KID);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int np = ARD ? (int)a.d : ((KID == GPRC_SQREXP || is_matern(KID)) ? 1 : 2);
  const int64_t tj = (int64_t)blockIdx.x * PT_C;
  const int64_t stripe = blockIdx.y;
  const int64_t z0 = (int64_t)blockIdx.z * SG_Z;
  const int dz = (int)((a.d - z0 < SG_Z) ? (a.d - z0) : SG_Z);
  const bool theta = blockIdx.z == 0;   // the theta sums belong to the first coordinate group
  const int64_t tile0 = stripe * a.stripe_tiles;
  const int64_t tile1 = (tile0 + a.stripe_tiles < a.ntiles) ? tile0 + a.stripe_tiles : a.ntiles;
  if constexpr (ARD)
    for (int k = t; k < np; k += 256) gacc[k] = 0.0;
  double a0 = 0.0, a1 = 0.0;            // isotropic kernels: this lane's theta sums over its stripe
  double acc[16][SG_Z];                 // WITH_Z: this lane's part of the column sums over its stripe
#pragma unroll
  for (int c = 0; c < 16; ++c)
#pragma unroll
    for (int r = 0; r < SG_Z; ++r) acc[c][r] = 0.0;

  for (int64_t tile = tile0; tile < tile1; ++tile) {
    const int64_t ti = tile * PT_R;
    // coordinates r0 .. r0 + dc - 1 of the tile's points (ARD: divided by their length scale); the column points are the same for every
    // tile of the stripe, so for d <= 16 their only chunk is staged once; own: also the workgroup's own SG_Z coordinates
    auto stage = [&](int64_t r0, int dc, bool own) {
      __syncthreads();
      stage_points<ARD>(a.A, ti, a.rows, a.d, r0, dc, PT_R, a.ks.p, t, [&](int i, int r, double v) { As[r][i] = v; });
      if (a.d > PT_D || tile == tile0) stage_points<ARD>(a.Z, tj, a.cols, a.d, r0, dc, PT_C, a.ks.p, t, [&](int j, int r, double v) { Bs[j][r] = v; });
      if constexpr (WITH_Z) {
        if (own) {   // all SG_Z slots, zero past dz: the column loop below then needs no branch on the coordinate
          auto own_coord = [&](const double* P, int64_t g, int64_t npts, int r) {
            double v = (r < dz && g < npts) ? P[g * a.d + z0 + r] : 0.0;
            if constexpr (ARD) { if (r < dz) v *= a.ks.p[z0 + r]; }
            return v;
          };
          for (int e = t; e < PT_R * SG_Z; e += 256) Az[e % SG_Z][e / SG_Z] = own_coord(a.A, ti + e / SG_Z, a.rows, e % SG_Z);
          if (tile == tile0 && t < PT_C * SG_Z) Bz[t / SG_Z][t % SG_Z] = own_coord(a.Z, tj + t / SG_Z, a.cols, t % SG_Z);
        }
      }
      __syncthreads();
    };

    double s0[16], s1[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) { s0[c] = 0.0; s1[c] = 0.0; }
    for (int64_t r0 = 0; r0 < a.d; r0 += PT_D) {
      const int dc = (int)((a.d - r0 < PT_D) ? (a.d - r0) : PT_D);
      stage(r0, dc, r0 == 0);
      accum_sqdist(As, Bs, dc, lane, wave, s0, s1);
    }

    const int64_t gi0 = ti + 2 * lane;
    const bool in0 = gi0 < a.rows, in1 = gi0 + 1 < a.rows;
    double az0[SG_Z], az1[SG_Z];   // WITH_Z: the workgroup's own coordinates of the lane's two rows
    if constexpr (WITH_Z) {
#pragma unroll
      for (int r = 0; r < SG_Z; ++r) {
        const double2 v = *reinterpret_cast<const double2*>(&Az[r][2 * lane]);
        az0[r] = v.x;
        az1[r] = v.y;
      }
    }
    // rows gi0, gi0 + 1 < 128 ntiles = rows_pad <= ld and columns tj + 63 < cols_pad: every load is inside the rows_pad x cols_pad matrix
    const double* gp = a.G + gi0 + (tj + wave * 16) * a.ld;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const int cj = wave * 16 + c;
      const bool jin = tj + cj < a.cols;
      const double2 g = *reinterpret_cast<const double2*>(gp + c * a.ld);
      double bz[SG_Z];
      if constexpr (WITH_Z) {
#pragma unroll
        for (int r = 0; r < SG_Z; ++r) bz[r] = Bz[cj][r];   // (slots past dz hold zeros on both sides: their sums stay 0 and are not written)
      }
      // one pair: its weight once, then every sum that hangs on it; `keep`: G h for ARD's second pass
      auto pair = [&](double gij, double s, const double (&az)[SG_Z], double& keep) {
        const PairW w = cross_weight<KID>(s, a.ks);
        const double p = gij * w.h;
        if constexpr (WITH_Z) {
#pragma unroll
          for (int r = 0; r < SG_Z; ++r) acc[c][r] = fma(p, az[r] - bz[r], acc[c][r]);
        }
        if constexpr (ARD) {
          keep = p;
        } else {
          a0 = fma(gij, w.hs, a0);
          if constexpr (KID == GPRC_GAMMAEXP || KID == GPRC_RATQUAD) a1 = fma(gij, w.h2, a1);
        }
      };
      const double g0 = (jin && in0) ? g.x : 0.0, g1 = (jin && in1) ? g.y : 0.0;   // the padding contributes exact zeros
      if constexpr (KID == GPRC_GAMMAEXP) {   // its weight and both integrands are 0 at s = 0: such a pair adds nothing (and log, the division stay in a block of their own)
        if (s0[c] > 0.0) pair(g0, s0[c], az0, s0[c]);
        if (s1[c] > 0.0) pair(g1, s1[c], az1, s1[c]);
      } else {
        pair(g0, s0[c], az0, s0[c]);
        pair(g1, s1[c], az1, s1[c]);
      }
      // WITH_Z holds 16 SG_Z running sums a lane: four columns of G and their weights in flight at a time, not sixteen
      if constexpr (WITH_Z) { if ((c & 3) == 3) __builtin_amdgcn_sched_barrier(0); }
    }

    if constexpr (ARD) {
      if (theta) {   // (uniform over the workgroup)
        for (int64_t r0 = 0; r0 < a.d; r0 += PT_D) {
          const int dc = (int)((a.d - r0 < PT_D) ? (a.d - r0) : PT_D);
          if (a.d > PT_D) stage(r0, dc, false);  // (d <= 16: the only chunk is still in LDS)
          for (int r = 0; r < dc; ++r) {
            const double v = wave_sum(weighted_sqdiff(As, Bs, r, lane, wave, s0, s1));
            if (lane == 0) red[wave][r] = v;
          }
          __syncthreads();
          if (t < dc) gacc[r0 + t] += sum4_pairs(red[0][t], red[1][t], red[2][t], red[3][t]);
          if (a.d <= PT_D) __syncthreads();  // (otherwise the next stage() separates these reads from the next chunk's writes)
        }
      }
    }
  }

  if (theta) {
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
  if constexpr (WITH_Z) {
    // a wave owns its 16 columns alone: one shuffle tree per (column, coordinate), once per stripe
#pragma unroll
    for (int c = 0; c < 16; ++c)
#pragma unroll
      for (int r = 0; r < SG_Z; ++r) {
        const double v = wave_sum(acc[c][r]);
        if (lane == 0 && r < dz) a.pz[(stripe * a.d + z0 + r) * a.cols_pad + tj + wave * 16 + c] = v;
        __builtin_amdgcn_sched_barrier(0);   // one tree after the other: 64 interleaved trees would want 64 more registers than the loop does
      }
  }
}

// dZ[c + d j] += f_c * sum over the stripes, in order, of pz[(st d + c) cols_pad + j];  f_c = ard ? f * ks.p[c] : f
__global__ __launch_bounds__(256) void cross_grad_sum_kernel(const double* pz, int64_t stripes, int64_t d, int64_t cols_pad, int64_t cols, double f,
                                                             int ard, KernelSpec ks, double* dZ) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;   // columns fastest: the partials are read contiguously
  if (idx >= cols * d) return;
  const int64_t c = idx / cols, j = idx - c * cols;
  double s = 0.0;
  for (int64_t st = 0; st < stripes; ++st) s += pz[(st * d + c) * cols_pad + j];
  dZ[c + d * j] = fma(ard ? f * ks.p[c] : f, s, dZ[c + d * j]);
}

// C[i, j] = sign u_i v_j, i < rows, j < cols
__global__ __launch_bounds__(256) void rank_one_kernel(double* C, int64_t ld, int64_t rows, int64_t cols, const double* u, const double* v, double sign) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  const double ui = sign * u[i];
  for (int64_t j = blockIdx.y; j < cols; j += gridDim.y) C[i + j * ld] = ui * v[j];
}

// From the lower triangles of W = -B^-1 and of B (n x n, pitch n), in place and symmetric: W := I + W, B := 2 I + W - B
__global__ __launch_bounds__(256) void sgrad_mid_kernel(double* W, double* B, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  for (int64_t j = blockIdx.y; j <= i; j += gridDim.y) {
    const double w = W[i + j * n], b = B[i + j * n], dg = (i == j) ? 1.0 : 0.0;
    const double iw = dg + w, mid = (2.0 * dg + w) - b;
    W[i + j * n] = iw;
    W[j + i * n] = iw;
    B[i + j * n] = mid;
    B[j + i * n] = mid;
  }
}

int64_t stripe_tiles_of(int64_t rows_pad) { return (rows_pad / PT_R + SG_MAX_STRIPES - 1) / SG_MAX_STRIPES; }

}  // namespace

int64_t cross_grad_stripes(int64_t rows_pad) {
  const int64_t st = stripe_tiles_of(rows_pad);
  return (rows_pad / PT_R + st - 1) / st;
}
int64_t cross_grad_wgs(int64_t rows_pad, int64_t cols_pad) { return cross_grad_stripes(rows_pad) * (cols_pad / PT_C); }
// (the stripe count is not monotonic in rows_pad: the buffers are sized for the most there can be)
int64_t cross_grad_partials(int64_t cols_pad, int n_params) { return SG_MAX_STRIPES * (cols_pad / PT_C) * n_params; }
int64_t cross_grad_zpartials(int64_t cols_pad, int64_t d) { return SG_MAX_STRIPES * d * cols_pad; }

int launch_cross_grad(hipStream_t s, const KernelSpec& ks, const double* G, int64_t ld, const double* A, int64_t rows, int64_t rows_pad,
                      const double* Z, int64_t cols, int64_t cols_pad, int64_t d, double* part, double* pz) {
  GPRC_TRY(check_grad_kernel("cross_grad", ks.id));
  if (!G || !A || !Z || !part || rows < 1 || cols < 1 || d < 1) { set_error("cross_grad: bad arguments (null pointer or an empty extent)"); return GPRC_ERR_ARG; }
  if (rows_pad % PT_R || rows_pad < rows || cols_pad % PT_C || cols_pad < cols) { set_error("cross_grad: rows are padded to 128, columns to 64"); return GPRC_ERR_ARG; }
  if (ld < rows_pad || (ld & 1) || (reinterpret_cast<uintptr_t>(G) & 15)) {
    set_error("cross_grad: the matrix must be 16-byte aligned with an even leading dimension >= the padded rows");
    return GPRC_ERR_ARG;
  }
  const int64_t zgroups = pz ? (d + SG_Z - 1) / SG_Z : 1, stripes = cross_grad_stripes(rows_pad);
  if (zgroups > 65535 || cols_pad / PT_C > 0x7fffffff) { set_error("cross_grad: too many coordinates or columns"); return GPRC_ERR_ARG; }
  SgradArgs a{G, A, Z, part, pz, rows, cols, d, ld, cols_pad, stripe_tiles_of(rows_pad), rows_pad / PT_R, make_deriv_spec(ks)};
  const dim3 grid((unsigned)(cols_pad / PT_C), (unsigned)stripes, (unsigned)zgroups);
  // per element and coordinate group: the distance (3 d), h (~40), the column sums (3 per coordinate), ARD's second pass (4 d, group 0);
  // bytes: G once per coordinate group + the points.  Counted with the exact gradient's contraction (the set of profiling kinds is fixed).
  const double elems = (double)rows_pad * (double)cols_pad;
  ProfScope ps(s, PK_GRAD_CONTRACT, elems * ((double)zgroups * (3.0 * d + 40.0 + (pz ? 3.0 * SG_Z : 0.0)) + (is_ard(ks.id) ? 4.0 * d : 4.0)),
               8.0 * (elems * (double)zgroups + (double)(rows + cols) * d));
  with_gradient_kernel(ks.id, [&](auto kid) {
    if (a.pz) hipLaunchKernelGGL((cross_grad_kernel<decltype(kid)::value, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((cross_grad_kernel<decltype(kid)::value, false>), grid, dim3(256), 0, s, a);
  });
  GPRC_LAUNCH_CHECK();
  return 0;
}

int launch_cross_grad_sum(hipStream_t s, const KernelSpec& ks, const double* pz, int64_t rows_pad, int64_t cols_pad, int64_t cols, int64_t d, double f,
                          double* dZ) {
  if (cols <= 0) return 0;
  GPRC_TRY(check_grad_kernel("cross_grad", ks.id));
  // the factor that does not depend on (i, j) (ARD: its constant times 1 / l_c per coordinate, from the spec)
  hipLaunchKernelGGL(cross_grad_sum_kernel, dim3((unsigned)((cols * d + 255) / 256)), dim3(256), 0, s, pz, cross_grad_stripes(rows_pad), d, cols_pad, cols,
                     f * deriv_tail_factor(ks), is_ard(ks.id) ? 1 : 0, make_deriv_spec(ks), dZ);
  GPRC_LAUNCH_CHECK();
  return 0;
}

void cross_grad_add_partials(const double* part_host, int64_t rows_pad, int64_t cols_pad, int n_params, long double f, long double* acc) {
  const int64_t wgs = cross_grad_wgs(rows_pad, cols_pad);
  for (int k = 0; k < n_params; ++k) {
    long double sum = 0.0L;
    for (int64_t g = 0; g < wgs; ++g) sum += (long double)part_host[g * n_params + k];
    acc[k] += f * sum;
  }
}

void cross_grad_finish(const KernelSpec& ks, const long double* acc, double* grad_out) {
  const long double l = (long double)ks.p[0], il3 = 1.0L / (l * l * l);
  switch (ks.id) {
    case GPRC_SQREXP: grad_out[0] = (double)(acc[0] * il3); break;
    case GPRC_GAMMAEXP:
      grad_out[0] = (double)(acc[0] * (long double)ks.p[1] / l);
      grad_out[1] = (double)(-0.5L * acc[1]);
      break;
    case GPRC_RATQUAD:
      grad_out[0] = (double)(acc[0] * il3);
      grad_out[1] = (double)acc[1];
      break;
    case GPRC_MATERN32: grad_out[0] = (double)(3.0L * acc[0] * il3); break;
    case GPRC_MATERN52: grad_out[0] = (double)(5.0L * acc[0] * il3 / 3.0L); break;
    default: {   // ARD
      const long double c = ks.id == GPRC_SQREXP_ARD ? 1.0L : (ks.id == GPRC_MATERN32_ARD ? 3.0L : 5.0L / 3.0L);
      for (int k = 0; k < ks.n_params; ++k) grad_out[k] = (double)(c * acc[k] / (long double)ks.p[k]);
    }
  }
}

int launch_rank_one(hipStream_t s, double* C, int64_t ld, int64_t rows, int64_t cols, const double* u, const double* v, double sign) {
  if (rows <= 0 || cols <= 0) return 0;
  hipLaunchKernelGGL(rank_one_kernel, dim3((unsigned)((rows + 255) / 256), (unsigned)std::min<int64_t>(cols, 4096)), dim3(256), 0, s, C, ld, rows, cols, u, v, sign);
  GPRC_LAUNCH_CHECK();
  return 0;
}

int launch_sgrad_mid(hipStream_t s, double* W, double* B, int64_t n) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(sgrad_mid_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)std::min<int64_t>(n, 4096)), dim3(256), 0, s, W, B, n);
  GPRC_LAUNCH_CHECK();
  return 0;
}

}  // namespace gprc
