// kernels_paths.hip -- the generated-operand GEMM of the posterior sample paths for gfx950 (gprc_gpr_paths_*, gprc_dev_feature_gemm,
// gprc_dev_kernel_gemm; DESIGN.md section 7, "Posterior sample paths"):
//
//   out[i + s ld] = scale * sum_j g(a_i, b_j) B[j + s ldb],      i < rows, s < S, j < cols
//
// where the left operand is never stored: a lane computes the elements it multiplies from the points.  Two generators:
//   features   g = cospi(2 t), t = sum_c Nu[c, j] a_i[c] + phase[j]   (frequencies in cycles, phases in turns: no 2 pi on the device;
//              cospi reduces its argument exactly)
//   kernel     g = k(a_i, b_j) from the squared distance, the eight stationary kernels of with_gradient_kernel, constants from
//              make_deriv_spec, ARD coordinates staged divided by their length scale as the contraction kernels stage them.  The value
//              is formed here and not taken from the fill's finish<KID>: it need not round like the fill's (pair_tile.h)
//
// v_mfma_f64_16x16x4_f64 takes each operand as ONE double per lane, (index lane & 15, k = lane >> 4).  So the lane that generates
// g for (row i0 + (lane & 15), column j0 + (lane >> 4)) already holds the operand: the generated matrix makes no trip through LDS or
// HBM.  It is the MFMA's B operand (its 16 columns are 16 rows i of the output), B^T is the A operand (16 sample columns s), and the
// accumulator holds out^T: element (s = 16 q + (lane >> 4) + 4 reg, i = lane & 15), so a store is 16 consecutive rows per lane group.
//
// A workgroup (four waves) owns one row tile (PT_R = 128 rows, two 16-row sub-tiles per wave), one STRIPE of column tiles
// (PT_C = 64 columns each) and one block of PA_SB = 64 sample columns.  Per column tile: the points go through LDS PT_D coordinates at
// a time (any d: the squared distance, or the phase's dot product, of a lane's 32 pairs accumulates over the passes, as in
// pair_tile.h); the tile's 64 x 64 block of B is staged once, zero where j >= cols or s >= S (the padding contributes exact zeros:
// B is padded, g is finite there); then per group of four columns a lane generates its two values and each feeds ceil(S / 16) <= 4
// MFMAs.  An f64 MFMA and a VALU instruction exclude each other on a SIMD, the generator is the cost, and every generated value is
// used for all sample columns of the block before the next one is formed.
//
// Order of summation is fixed: j ascending in the MFMA's groups of four, tile after tile of the stripe, one partial per (stripe, s, i);
// the stripes are added in order by gen_gemm_sum_kernel, which applies `scale` once to the sum.  No atomics.  The stripe is a function
// of the padded column count alone and a row's arithmetic touches no other row: a row's result does not depend on which other rows
// are in the call, bit for bit.
//
// Profiled under kind 19 (PK_PRED_GRAD, "prediction-gradient contraction"): like it, a contraction over pairs generated from the test
// and the training points.  The number of kinds stays 20.
//
// The gradient of the product with respect to the row points (gprc_gpr_paths_eval_grad, gprc_dev_feature_gemm_grad,
// gprc_dev_kernel_gemm_grad; DESIGN.md section 7, "Sample-path gradients and Thompson sampling") is gen_gemm_grad_kernel below: the same
// operand form with one generated operand per coordinate, its own blocking, the same stripes and order of summation, the same kind.
#include "pair_tile.h"

#include <algorithm>

namespace gprc {

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int PA_SB = 64;           // sample columns per workgroup: four MFMAs per generated value
constexpr int PA_LDB = PT_C + 2;     // pitch of the staged block of B: the 32 lanes of a ds_read_b64 group cover the 64 banks once
constexpr int PA_MAX_STRIPES = 32;
constexpr int GEN_FEATURES = -1;     // the generator that is not a kernel id

struct GenArgs {
  const double* A;       // d x rows: the points of the output's rows
  const double* Bp;      // d x cols: the column points (training points; the frequencies Nu)
  const double* phase;   // cols (features only)
  const double* B;       // cols x S, pitch ldb
  double* part;          // stripes x S x rows_pad
  int64_t rows, cols, d, ldb, S, rows_pad;
  int64_t stripe_tiles, ntiles;
  KernelSpec ks;         // derived constants, see make_deriv_spec (kernel generators only)
};

template <int GEN>
__global__ __launch_bounds__(256) void gen_gemm_kernel(GenArgs a) {
  __shared__ __attribute__((aligned(16))) double As[PT_D][PT_R];
  __shared__ double Bs[PT_C][PT_D + 1];
  __shared__ __attribute__((aligned(16))) double Bt[PA_SB][PA_LDB];   // Bt[s][j]: the tile's block of B
  __shared__ double Ph[PT_C];
  constexpr bool FEAT = GEN == GEN_FEATURES;
  constexpr bool ARD = !FEAT && is_ard(GEN);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const int64_t ti = (int64_t)blockIdx.x * PT_R;
  const int64_t stripe = blockIdx.y;
  const int64_t sb0 = (int64_t)blockIdx.z * PA_SB;
  const int ns = (int)((a.S - sb0 < PA_SB) ? (a.S - sb0) : PA_SB);   // sample columns of this block, workgroup-uniform
  const int nq = (ns + 15) >> 4;
  const int64_t tile0 = stripe * a.stripe_tiles;
  const int64_t tile1 = (tile0 + a.stripe_tiles < a.ntiles) ? tile0 + a.stripe_tiles : a.ntiles;
  const int i0 = wave * 32 + fr, i1 = i0 + 16;                       // the lane's two rows of the tile

  double4_t acc[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[m][q] = double4_t{0.0, 0.0, 0.0, 0.0};

  for (int64_t tile = tile0; tile < tile1; ++tile) {
    const int64_t tj = tile * PT_C;
    double s0[16], s1[16];   // per group of four columns kk: the lane's pair (i0 | i1, column 4 kk + fk)
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) { s0[kk] = 0.0; s1[kk] = 0.0; }
    for (int64_t r0 = 0; r0 < a.d; r0 += PT_D) {
      const int dc = (int)((a.d - r0 < PT_D) ? (a.d - r0) : PT_D);
      __syncthreads();
      if (a.d > PT_D || tile == tile0) {   // (d <= 16: the row points' only chunk stays in LDS for the whole stripe)
        stage_points<ARD>(a.A, ti, a.rows, a.d, r0, dc, PT_R, a.ks.p, t, [&](int i, int r, double v) { As[r][i] = v; });
      }
      stage_points<ARD>(a.Bp, tj, a.cols, a.d, r0, dc, PT_C, a.ks.p, t, [&](int j, int r, double v) { Bs[j][r] = v; });
      if (r0 == 0) {
        for (int e = t; e < PA_SB * PT_C; e += 256) {   // 64 consecutive j of one sample column per wave: 512 contiguous bytes
          const int sc = e >> 6, j = e & 63;
          Bt[sc][j] = (sc < ns && tj + j < a.cols) ? a.B[(tj + j) + (sb0 + sc) * a.ldb] : 0.0;
        }
        if constexpr (FEAT) {
          if (t < PT_C) Ph[t] = (tj + t < a.cols) ? a.phase[tj + t] : 0.0;
        }
      }
      __syncthreads();
      for (int r = 0; r < dc; ++r) {
        const double a0 = As[r][i0], a1 = As[r][i1];
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
          const double b = Bs[4 * kk + fk][r];
          if constexpr (FEAT) {
            s0[kk] = fma(a0, b, s0[kk]);
            s1[kk] = fma(a1, b, s1[kk]);
          } else {
            const double t0 = a0 - b, t1 = a1 - b;
            s0[kk] = fma(t0, t0, s0[kk]);
            s1[kk] = fma(t1, t1, s1[kk]);
          }
        }
      }
    }
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      double g0, g1;
      if constexpr (FEAT) {
        const double ph = Ph[4 * kk + fk];
        g0 = cospi(2.0 * (s0[kk] + ph));
        g1 = cospi(2.0 * (s1[kk] + ph));
      } else {
        g0 = kernel_value<GEN>(s0[kk], a.ks);
        g1 = kernel_value<GEN>(s1[kk], a.ks);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (q < nq) {
          const double b = Bt[16 * q + fr][4 * kk + fk];   // zero in the padding of j and of s
          acc[0][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(b, g0, acc[0][q], 0, 0, 0);
          acc[1][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(b, g1, acc[1][q], 0, 0, 0);
        }
      }
    }
  }

  // acc[m][q][reg] = element (s = sb0 + 16 q + fk + 4 reg, i = ti + wave 32 + 16 m + fr): rows < rows_pad always, columns guarded
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int sc = 16 * q + fk + 4 * reg;
      if (sc < ns) {
        double* dst = a.part + (stripe * a.S + sb0 + sc) * a.rows_pad + ti;
        dst[i0] = acc[0][q][reg];
        dst[i1] = acc[1][q][reg];
      }
    }
}

// out[i + s ld] = (accumulate ? out[i + s ld] : 0) + scale * (the stripes of part[(st S + s) rows_pad + i] in order)
__global__ __launch_bounds__(256) void gen_gemm_sum_kernel(const double* part, int64_t stripes, int64_t S, int64_t rows_pad, int64_t rows, double scale,
                                                           int accumulate, double* out, int64_t ld) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;   // rows fastest: the partials are read contiguously
  if (idx >= rows * S) return;
  const int64_t s = idx / rows, i = idx - s * rows;
  double v = 0.0;
  for (int64_t st = 0; st < stripes; ++st) v += part[(st * S + s) * rows_pad + i];
  v *= scale;
  out[i + s * ld] = accumulate ? out[i + s * ld] + v : v;
}

// ---- the gradient with respect to the row points ---------------------------------------------------------------------------------
//   part[((stripe d + c) S + s) rows_pad + i] = sum over the stripe's j of w(a_i, b_j) e_c(i, j) B[j + s ldb]
// the product whose generated operand carries one more index, the coordinate c (gprc_gpr_paths_eval_grad, gprc_dev_*_gemm_grad):
//   kernel     w = pair_weight<KID> (h of dk / da_c = -h (a_c - b_c) t_c without its pair-independent factor), e_c = a_ic - b_jc: the
//              direct difference of the staged coordinates (ARD: both divided by l_c), never a_ic sum - sum b_jc
//   features   w = sinpi(2 t), t as gen_gemm_kernel forms it, e_c = Nu[c, j]
// w is formed ONCE per pair; then per coordinate one multiply (the kernel's difference before it) and ceil(ns / 16) x 2 MFMAs, the
// operand in the lane as above.  The accumulators are coordinates x rows x sample columns, so a workgroup owns PGR_C = 4 coordinates and
// PGR_SB = 32 sample columns of one row tile and one stripe: 4 x 2 x 2 double4 = 128 registers.  A column tile goes through in two
// halves of PGR_TC = 32 columns, in order, so that the squared distances take 32 registers and not 64: with 64 five of the nine
// instantiations needed more than 256 registers and ran one wave per SIMD; now all stay at two (profiles/paths_grad_isa.txt; eight
// coordinates a workgroup would halve the generator's work and run one wave).  Further coordinate groups and sample blocks are
// further workgroups (blockIdx.z = group * sblocks + block) that form the distance again, as pred_grad_kernel does for d > 8.  The
// group's own coordinates of the column points are staged a second time (Bz), the lane's own of its two rows stay in registers.
// Any d: the distance takes ceil(d / PT_D) staging passes before w is known.  Order of summation as gen_gemm_kernel: j ascending in
// groups of four, tile after tile, one partial per (stripe, c, s, i); gen_gemm_grad_sum_kernel adds the stripes in order and applies
// the pair-independent factor once.  No atomics, no scratch.
constexpr int PGR_C = 4;
constexpr int PGR_SB = 32;
constexpr int PGR_TC = 32;   // columns staged at a time: half a column tile, so that the squared distances take 32 registers, not 64
constexpr int PGR_LDB = PGR_TC + 2;

struct GenGradArgs {
  const double* A;       // d x rows
  const double* Bp;      // d x cols
  const double* phase;   // cols (features only)
  const double* B;       // cols x S, pitch ldb
  double* part;          // stripes x d x S x rows_pad
  int64_t rows, cols, d, ldb, S, rows_pad;
  int64_t stripe_tiles, ntiles, sblocks;
  KernelSpec ks;
};

template <int GEN>
__global__ __launch_bounds__(256) void gen_gemm_grad_kernel(GenGradArgs a) {
  __shared__ __attribute__((aligned(16))) double As[PT_D][PT_R];
  __shared__ double Bs[PGR_TC][PT_D + 1];
  __shared__ __attribute__((aligned(16))) double Bt[PGR_SB][PGR_LDB];   // Bt[s][j]: the half tile's block of B
  __shared__ double Bz[PGR_TC][PGR_C + 1];                             // the group's own coordinates of the half tile's column points
  __shared__ double Ph[PGR_TC];
  constexpr bool FEAT = GEN == GEN_FEATURES;
  constexpr bool ARD = !FEAT && is_ard(GEN);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const int64_t ti = (int64_t)blockIdx.x * PT_R;
  const int64_t stripe = blockIdx.y;
  const int64_t zg = (int64_t)blockIdx.z / a.sblocks;
  const int64_t z0 = zg * PGR_C;
  const int64_t sb0 = ((int64_t)blockIdx.z - zg * a.sblocks) * PGR_SB;
  const int dz = (int)((a.d - z0 < PGR_C) ? (a.d - z0) : PGR_C);        // coordinates and sample columns of this workgroup, uniform
  const int ns = (int)((a.S - sb0 < PGR_SB) ? (a.S - sb0) : PGR_SB);
  const bool two = ns > 16;
  const int64_t tile0 = stripe * a.stripe_tiles;
  const int64_t tile1 = (tile0 + a.stripe_tiles < a.ntiles) ? tile0 + a.stripe_tiles : a.ntiles;
  const int i0 = wave * 32 + fr, i1 = i0 + 16;                       // the lane's two rows of the tile

  double xa0[PGR_C], xa1[PGR_C];   // kernel generators: the lane's own coordinates of its two rows, as staged
#pragma unroll
  for (int c = 0; c < PGR_C; ++c) {
    xa0[c] = xa1[c] = 0.0;
    if constexpr (!FEAT) {
      if (c < dz) {
        const double sc = ARD ? a.ks.p[z0 + c] : 1.0;
        if (ti + i0 < a.rows) xa0[c] = a.A[(ti + i0) * a.d + z0 + c] * sc;
        if (ti + i1 < a.rows) xa1[c] = a.A[(ti + i1) * a.d + z0 + c] * sc;
      }
    }
  }

  double4_t acc[PGR_C][2][2];
#pragma unroll
  for (int c = 0; c < PGR_C; ++c)
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int q = 0; q < 2; ++q) acc[c][m][q] = double4_t{0.0, 0.0, 0.0, 0.0};

  constexpr int HALVES = PT_C / PGR_TC, NKK = PGR_TC / 4;
  for (int64_t sub = tile0 * HALVES; sub < tile1 * HALVES; ++sub) {   // the halves of the stripe's column tiles in order
    const int64_t tj = sub * PGR_TC;
    double s0[NKK], s1[NKK];   // per group of four columns kk: the lane's pair (i0 | i1, column 4 kk + fk)
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) { s0[kk] = 0.0; s1[kk] = 0.0; }
    for (int64_t r0 = 0; r0 < a.d; r0 += PT_D) {
      const int dc = (int)((a.d - r0 < PT_D) ? (a.d - r0) : PT_D);
      __syncthreads();
      if (a.d > PT_D || sub == tile0 * HALVES) {   // (d <= 16: the row points' only chunk stays in LDS for the whole stripe)
        stage_points<ARD>(a.A, ti, a.rows, a.d, r0, dc, PT_R, a.ks.p, t, [&](int i, int r, double v) { As[r][i] = v; });
      }
      stage_points<ARD>(a.Bp, tj, a.cols, a.d, r0, dc, PGR_TC, a.ks.p, t, [&](int j, int r, double v) { Bs[j][r] = v; });
      if (r0 == 0) {
        for (int e = t; e < PGR_SB * PGR_TC; e += 256) {   // 32 consecutive j of one sample column per half wave
          const int sc = e / PGR_TC, j = e % PGR_TC;
          Bt[sc][j] = (sc < ns && tj + j < a.cols) ? a.B[(tj + j) + (sb0 + sc) * a.ldb] : 0.0;
        }
        stage_points<ARD>(a.Bp, tj, a.cols, a.d, z0, dz, PGR_TC, a.ks.p, t, [&](int j, int r, double v) { Bz[j][r] = v; });
        if constexpr (FEAT) {
          if (t < PGR_TC) Ph[t] = (tj + t < a.cols) ? a.phase[tj + t] : 0.0;
        }
      }
      __syncthreads();
      for (int r = 0; r < dc; ++r) {
        const double a0 = As[r][i0], a1 = As[r][i1];
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
          const double b = Bs[4 * kk + fk][r];
          if constexpr (FEAT) {
            s0[kk] = fma(a0, b, s0[kk]);
            s1[kk] = fma(a1, b, s1[kk]);
          } else {
            const double t0 = a0 - b, t1 = a1 - b;
            s0[kk] = fma(t0, t0, s0[kk]);
            s1[kk] = fma(t1, t1, s1[kk]);
          }
        }
      }
    }
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) {
      const int j = 4 * kk + fk;
      double w0, w1;
      if constexpr (FEAT) {
        const double ph = Ph[j];
        w0 = sinpi(2.0 * (s0[kk] + ph));
        w1 = sinpi(2.0 * (s1[kk] + ph));
      } else {
        w0 = pair_weight<GEN>(s0[kk], a.ks);
        w1 = pair_weight<GEN>(s1[kk], a.ks);
      }
      const double b0 = Bt[fr][j], b1 = Bt[16 + fr][j];   // zero in the padding of j and of s
#pragma unroll
      for (int c = 0; c < PGR_C; ++c) {
        if (c < dz) {
          const double bz = Bz[j][c];
          double g0, g1;
          if constexpr (FEAT) {
            g0 = w0 * bz;
            g1 = w1 * bz;
          } else {
            g0 = w0 * (xa0[c] - bz);
            g1 = w1 * (xa1[c] - bz);
          }
          acc[c][0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(b0, g0, acc[c][0][0], 0, 0, 0);
          acc[c][1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(b0, g1, acc[c][1][0], 0, 0, 0);
          if (two) {
            acc[c][0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(b1, g0, acc[c][0][1], 0, 0, 0);
            acc[c][1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(b1, g1, acc[c][1][1], 0, 0, 0);
          }
        }
      }
    }
  }

  // acc[c][m][q][reg] = element (coordinate z0 + c, s = sb0 + 16 q + fk + 4 reg, i = ti + wave 32 + 16 m + fr): rows < rows_pad always,
  // coordinates and columns guarded
#pragma unroll
  for (int c = 0; c < PGR_C; ++c)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int sc = 16 * q + fk + 4 * reg;
        if (c < dz && sc < ns) {
          double* dst = a.part + ((stripe * a.d + z0 + c) * a.S + sb0 + sc) * a.rows_pad + ti;
          dst[i0] = acc[c][0][q][reg];
          dst[i1] = acc[c][1][q][reg];
        }
      }
}

// dout[i + ld (s + S c)] = (accumulate ? dout[.] : 0) + f_c * (the stripes of part[((st d + c) S + s) rows_pad + i] in order),
// f_c = sign * (ard ? iso * ks.p[c] : iso) as pred_grad_sum_kernel forms it
__global__ __launch_bounds__(256) void gen_gemm_grad_sum_kernel(const double* part, int64_t stripes, int64_t d, int64_t S, int64_t rows_pad, int64_t rows,
                                                                double sign, double iso, int ard, KernelSpec ks, int accumulate, double* dout,
                                                                int64_t ld) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;   // rows fastest: the partials are read contiguously
  if (idx >= rows * S * d) return;
  const int64_t cs = idx / rows, i = idx - cs * rows;             // cs = s + S c
  const int64_t c = cs / S, s = cs - c * S;
  double v = 0.0;
  for (int64_t st = 0; st < stripes; ++st) v += part[((st * d + c) * S + s) * rows_pad + i];
  v *= sign * (ard ? iso * ks.p[c] : iso);
  dout[i + cs * ld] = accumulate ? dout[i + cs * ld] + v : v;
}

// the rows of a solve chunk from the prior term F (n x S, pitch ldf):  vt[s + j ldv] = y_j - F[j, s0 + s] - sqn E[j, s0 + s] for
// s < scur, j < n; zero in the padding (s < m_pad, j < n_pad)
__global__ __launch_bounds__(256) void paths_residual_kernel(const double* y, const double* F, int64_t ldf, const double* E, int64_t lde, double sqn,
                                                             int64_t s0, int64_t scur, int64_t n, int64_t m_pad, int64_t n_pad, double* vt, int64_t ldv) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= m_pad * n_pad) return;
  const int64_t j = idx / m_pad, s = idx - j * m_pad;
  double v = 0.0;
  if (s < scur && j < n) v = (y[j] - F[j + (s0 + s) * ldf]) - sqn * E[j + (s0 + s) * lde];
  vt[s + j * ldv] = v;
}

// U[j + (s0 + s) ldu] = vt[s + (n_pad - 1 - j) ldv]: the solved chunk leaves the reversed factor column-reversed
__global__ __launch_bounds__(256) void paths_weights_kernel(const double* vt, int64_t ldv, int64_t n_pad, int64_t s0, int64_t scur, int64_t n, double* U,
                                                            int64_t ldu) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= scur * n) return;
  const int64_t j = idx / scur, s = idx - j * scur;
  U[j + (s0 + s) * ldu] = vt[s + (n_pad - 1 - j) * ldv];
}

// column tiles per stripe: at most PA_MAX_STRIPES stripes
int64_t stripe_tiles_of(int64_t cols_pad) { return (cols_pad / PT_C + PA_MAX_STRIPES - 1) / PA_MAX_STRIPES; }

}  // namespace

int64_t gen_gemm_stripes(int64_t cols) {
  const int64_t cols_pad = pad_up(cols, PT_C), st = stripe_tiles_of(cols_pad);
  return (cols_pad / PT_C + st - 1) / st;
}

int launch_gen_gemm(hipStream_t s, const KernelSpec* ks, const double* Bp, const double* phase, int64_t cols, const double* A, int64_t rows,
                    int64_t rows_pad, int64_t d, const double* B, int64_t ldb, int64_t S, double scale, bool accumulate, double* part, double* out,
                    int64_t ld) {
  if (rows < 1 || cols < 1 || S < 1 || d < 1 || rows_pad % PT_R || rows_pad < rows || ldb < cols || ld < rows || !A || !Bp || !B || !part || !out ||
      (!ks && !phase)) {
    set_error("gen_gemm: bad arguments");
    return GPRC_ERR_ARG;
  }
  if (ks) GPRC_TRY(check_grad_kernel("kernel_gemm", ks->id));
  const int64_t sblocks = (S + PA_SB - 1) / PA_SB;
  if (sblocks > 65535) { set_error("gen_gemm: too many sample columns"); return GPRC_ERR_ARG; }
  const int64_t cols_pad = pad_up(cols, PT_C), stripes = gen_gemm_stripes(cols);
  GenArgs a{A, Bp, phase, B, part, rows, cols, d, ldb, S, rows_pad, stripe_tiles_of(cols_pad), cols_pad / PT_C, ks ? make_deriv_spec(*ks) : KernelSpec{}};
  const dim3 grid((unsigned)(rows_pad / PT_R), (unsigned)stripes, (unsigned)sblocks);
  // per pair and sample block: the distance or the phase (3 d), the value (~40), 2 flops per sample column on the MFMA
  const double pairs = (double)rows_pad * (double)cols_pad;
  ProfScope ps(s, PK_PRED_GRAD, pairs * ((3.0 * d + 40.0) * sblocks + 2.0 * S), 8.0 * ((double)(rows + cols) * d + (double)cols * S + (double)rows * S * (stripes + 1)));
  if (!ks) hipLaunchKernelGGL((gen_gemm_kernel<GEN_FEATURES>), grid, dim3(256), 0, s, a);
  else with_gradient_kernel(ks->id, [&](auto kid) { hipLaunchKernelGGL((gen_gemm_kernel<decltype(kid)::value>), grid, dim3(256), 0, s, a); });
  GPRC_LAUNCH_CHECK();
  hipLaunchKernelGGL(gen_gemm_sum_kernel, dim3((unsigned)((rows * S + 255) / 256)), dim3(256), 0, s, part, stripes, S, rows_pad, rows, scale,
                     accumulate ? 1 : 0, out, ld);
  GPRC_LAUNCH_CHECK();
  return 0;
}

int launch_gen_gemm_grad(hipStream_t s, const KernelSpec* ks, const double* Bp, const double* phase, int64_t cols, const double* A, int64_t rows,
                         int64_t rows_pad, int64_t d, const double* B, int64_t ldb, int64_t S, double scale, bool accumulate, double* part, double* dout,
                         int64_t ld) {
  if (rows < 1 || cols < 1 || S < 1 || d < 1 || rows_pad % PT_R || rows_pad < rows || ldb < cols || ld < rows || !A || !Bp || !B || !part || !dout ||
      (!ks && !phase)) {
    set_error("gen_gemm_grad: bad arguments");
    return GPRC_ERR_ARG;
  }
  if (ks) GPRC_TRY(check_grad_kernel("kernel_gemm_grad", ks->id));
  const int64_t sblocks = (S + PGR_SB - 1) / PGR_SB, zgroups = (d + PGR_C - 1) / PGR_C;
  if (sblocks * zgroups > 65535) { set_error("gen_gemm_grad: too many coordinates times sample columns"); return GPRC_ERR_ARG; }
  const int64_t cols_pad = pad_up(cols, PT_C), stripes = gen_gemm_stripes(cols);
  const KernelSpec ds = ks ? make_deriv_spec(*ks) : KernelSpec{};
  GenGradArgs a{A, Bp, phase, B, part, rows, cols, d, ldb, S, rows_pad, stripe_tiles_of(cols_pad), cols_pad / PT_C, sblocks, ds};
  const dim3 grid((unsigned)(rows_pad / PT_R), (unsigned)stripes, (unsigned)(sblocks * zgroups));
  // per pair and workgroup of (coordinate group, sample block): the distance or the phase (3 d), the weight (~40), two flops per
  // coordinate for the operand; 2 flops per sample column and coordinate on the MFMA
  const double pairs = (double)rows_pad * (double)cols_pad;
  ProfScope ps(s, PK_PRED_GRAD, pairs * ((3.0 * d + 40.0 + 2.0 * PGR_C) * sblocks * zgroups + 2.0 * S * d),
               8.0 * ((double)(rows + cols) * d + (double)cols * S + (double)rows * S * d * (stripes + 1)));
  if (!ks) hipLaunchKernelGGL((gen_gemm_grad_kernel<GEN_FEATURES>), grid, dim3(256), 0, s, a);
  else with_gradient_kernel(ks->id, [&](auto kid) { hipLaunchKernelGGL((gen_gemm_grad_kernel<decltype(kid)::value>), grid, dim3(256), 0, s, a); });
  GPRC_LAUNCH_CHECK();
  // d / da_c of the value product: -t_c h (a_c - b_c) for a kernel (deriv_tail_factor, ARD's second 1 / l_c from the derived spec),
  // -2 pi nu_c sin 2 pi t for the features; times `scale`
  const double iso = (ks ? deriv_tail_factor(*ks) : 6.283185307179586476925) * scale;
  hipLaunchKernelGGL(gen_gemm_grad_sum_kernel, dim3((unsigned)((rows * S * d + 255) / 256)), dim3(256), 0, s, part, stripes, d, S, rows_pad, rows, -1.0, iso,
                     (ks && is_ard(ks->id)) ? 1 : 0, ds, accumulate ? 1 : 0, dout, ld);
  GPRC_LAUNCH_CHECK();
  return 0;
}

int launch_paths_residual(hipStream_t s, const double* y, const double* F, int64_t ldf, const double* E, int64_t lde, double sqn, int64_t s0,
                          int64_t scur, int64_t n, int64_t m_pad, int64_t n_pad, double* vt, int64_t ldv) {
  hipLaunchKernelGGL(paths_residual_kernel, dim3((unsigned)((m_pad * n_pad + 255) / 256)), dim3(256), 0, s, y, F, ldf, E, lde, sqn, s0, scur, n, m_pad,
                     n_pad, vt, ldv);
  GPRC_LAUNCH_CHECK();
  return 0;
}

int launch_paths_weights(hipStream_t s, const double* vt, int64_t ldv, int64_t n_pad, int64_t s0, int64_t scur, int64_t n, double* U, int64_t ldu) {
  hipLaunchKernelGGL(paths_weights_kernel, dim3((unsigned)((scur * n + 255) / 256)), dim3(256), 0, s, vt, ldv, n_pad, s0, scur, n, U, ldu);
  GPRC_LAUNCH_CHECK();
  return 0;
}

}  // namespace gprc
