// chol_tile.h -- the device-side cores of the blocked fp64 Cholesky for gfx950 (MI355X), shared by kernels_gemm.hip and
// kernels_chol.hip (device code only; everything sits in the units' anonymous namespace).
//
// Replaces L <- t(chol(K + noise * diag(n)))  (reference R/GPRclass.R:142, LAPACK dpotrf) and, through
// the same GEMM tile, v <- solve(L, K_star) (R/GPRclass.R:162, which the reference runs as a general
// pivoted dgesv).  The pieces:
//   potf2_blocked_body  one workgroup factors a 128x128 diagonal block entirely in LDS and also forms
//                     its inverse (so every panel / right-hand-side solve is a GEMM);
//   gemm_tile_128     128x128 output tile per 256-thread workgroup, 4 waves x (64x64) of
//                     v_mfma_f64_16x16x4_f64, A/B strips staged through double-buffered LDS;
//   tile-id decoders  block id -> tile of a grouped grid / of the packed block-column layout (lower tiles only).
// The kernels around them: kernels_gemm.hip (no flags between workgroups: panel solve X := X * Winv^T, C -= A*B^T, the trailing
// updates, the predict's solve passes) and kernels_chol.hip (a whole panel's dependent chain in one launch / every panel's in one
// persistent launch -- the factor service -- with the caller's-stream kernels that go with it).
// The trailing update is the dominant kernel of the whole path: n^3/3 of the fit and n^2 n* of the
// predict go through gemm_tile_128().
#pragma once
#include <utility>

#include "gprc_internal.h"

namespace gprc {

typedef double double4_t __attribute__((ext_vector_type(4)));

namespace {

// ------------------------------------------------------------------------------------------------
// Diagonal block: Cholesky + inverse of a 128 x 128 block in one sweep by one workgroup.
// ------------------------------------------------------------------------------------------------
constexpr int PB = 128;

// ------------------------------------------------------------------------------------------------
// Blocked diagonal-block kernel (default): the same factor + inverse, 16 columns at a time.
// The 128 x 128 block lives in LDS (leading dimension 144: MFMA operand reads conflict-free).  Per 16-column step:
//   A  wave 0 factors the 16 x 16 diagonal sub-block and inverts it with a register-resident scalar sweep (diag16:
//      16 sequential pivots, a matrix row per lane, operands exchanged inside the 16-lane row by DPP row_newbcast; sqrt /
//      reciprocal from a Newton-refined v_rsq_f64 -- ~60 dependent cycles instead of the ~600 of the library
//      sqrt + division);
//   B  panel rows below: X_I = A_I * Wd^T, and row s of the inverse: X_sJ = Wd * Y_sJ   (4 MFMAs per 16x16 block);
//   C  Cholesky trailing blocks C_IJ -= X_I X_J^T and inverse blocks Y_IJ -= L_Is X_sJ  (4 MFMAs per block); wave 0
//      updates the next diagonal block first and runs phase A of step s+1 beside the other waves' blocks,
// one barrier after B and one after C.  L is kept in the lower triangle, the (unscaled-free) inverse transposed in the
// upper triangle, its diagonal in a side array -- the layout of the output.  The sequential depth drops from 128
// whole-workgroup steps to 128 single-wave steps on 16-row data.
// ------------------------------------------------------------------------------------------------
constexpr int BLD = 144;
constexpr int PB_SMEM_DOUBLES = PB * BLD + 512 + PB;  // S, 2 x Wd, Wdiag
constexpr size_t PB_SMEM_BYTES = PB_SMEM_DOUBLES * sizeof(double);
// Where potf2_blocked_body leaves things in sm, for the kernels that go on working in its image (small_model.h):
// the two 16 x 16 buffers (512 doubles, free between the body's calls), the diagonal of the inverse, and W[k][i] of the factored image
// S -- the inverse sits transposed above the diagonal, its diagonal in the side array
__device__ __forceinline__ double* pb_work(double* sm) { return sm + PB * BLD; }
__device__ __forceinline__ double* pb_wdiag(double* sm) { return sm + PB * BLD + 512; }
__device__ __forceinline__ double pb_w(const double* S, const double* Wdiag, int k, int i) {
  return k > i ? S[i + k * BLD] : (k == i ? Wdiag[i] : 0.0);
}

// sqrt(d) and 1/sqrt(d) from v_rsq_f64 + two Newton steps (+ one correction of the root)
__device__ __forceinline__ void sqrt_rsqrt(double d, double& root, double& rinv) {
  double r = __builtin_amdgcn_rsq(d);
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const double e = fma(-(d * r), r, 1.0);  // 1 - d r^2
    r = fma(0.5 * r, e, r);
  }
  double l = d * r;
  l = fma(0.5 * r, fma(-l, l, d), l);
  root = l;
  rinv = r;
}

// Phase A: one wave factors the 16x16 block at D (LDS, ld BLD; lower triangle valid) in place, writes its inverse dense to
// Wd[16][16] (column-major), transposed-strict-lower into D's upper triangle and the diagonal to wdiag.
//
// Outer-product Cholesky with the rank-1 update on the matrix core.  The wave holds the full SYMMETRIC working block A and a
// unit-lower-triangular V (Gauss-Jordan on [A | I]: W = diag(rinv) V at the end) in the accumulator layout of
// v_mfma_f64_16x16x4: lane (q = lane >> 4, r = lane & 15), register rr <-> element (x = q + 4 rr, y = r).  Row J of either matrix
// is then ONE register (rr = J / 4) of ONE 16-lane row (q = J % 4), indexed by the lane -- exactly the shape of an MFMA operand
// in k-slot q.  Pivot J:
//   u = row J of A (= column J: the block stays bitwise symmetric, l_x l_y and l_y l_x are the same product)
//   d = u[J] (DPP row_newbcast inside the 16-lane row), rinv = 1/sqrt(d) (v_rsq_f64 + two Newton steps)
//   l = u rinv below the diagonal, 0 elsewhere and in the other three lane rows;  m = -l rinv
//   A -= l l^T      one MFMA: both operands are l, k-slot J % 4, the other slots zero
//   V += m v_J^T    one MFMA: v_J = row J of V (V starts as I, so column J receives m and V[J][J] stays 1)
// The dependent chain of a column is DPP mov -> rsqrt -> one multiply -> one MFMA (~200 cycles: tools/microbench/dp_latency.hip has
// the instruction latencies), all 64 lanes work, and a pivot is ~35 instructions.  (An f64 MFMA runs on the SIMD's double-precision
// lanes: no VALU instruction of the wave issues beside it, so the second MFMA and the column's stores add to the chain rather than
// hide behind it -- ~400 cycles per pivot measured.)  (Round 2's sweep kept a
// row per lane quadruple and exchanged six operands per pivot by ds_bpermute: ~85 instructions and ~600 cycles per pivot, 3.7 us per
// sweep; a row-per-lane form with v_fmac_f64_dpp -- DPP on 64-bit operands issues at ~13 cycles -- reached 3.3 us.)
// No exec-masked branch and no store inside the sweep: a column's entries of L stay in a register of the lane row that computed
// them, a non-positive pivot is only noted for one atomic after the sweep.
template <int SRC>
__device__ __forceinline__ double row_bcast(double v) {   // lane SRC's v, in every lane of the same 16-lane row
  return __builtin_amdgcn_update_dpp(0.0, v, 0x150 + SRC, 0xf, 0xf, true);   // DPP_ROW_NEWBCAST0 + SRC
}

template <int J>
__device__ __forceinline__ void diag16_pivot(double4_t& A, double4_t& V, double (&rinvs)[4], double (&lcol)[4], unsigned& bad, int q, int r) {
  constexpr int QJ = J & 3, RJ = J >> 2;
  const bool inrow = q == QJ;
  const bool below = inrow && r > J;
  // ---- the chain (a wave issues in order: the sched_barriers make the program order the schedule)
  const double u = A[RJ];                             // row J of the working block (lane row QJ)
  const double d = row_bcast<J>(u);                   // the pivot
  double rinv = __builtin_amdgcn_rsq(d);              // sqrt_rsqrt's rinv: v_rsq_f64 + two Newton steps
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const double e = fma(-(d * rinv), rinv, 1.0);
    rinv = fma(0.5 * rinv, e, rinv);
  }
  const double t = u * rinv;
  const double lv = below ? t : 0.0;                  // column J of L below the diagonal; zero in the other k-slots
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (J < 15) A = __builtin_amdgcn_mfma_f64_16x16x4f64(lv, lv, A, 0, 0, 1);   // A -= l l^T
  __builtin_amdgcn_sched_barrier(0);
  // ---- behind the chain's MFMA
  if constexpr (J < 15) {
    const double mv = below ? -(t * rinv) : 0.0;
    const double vrow = inrow ? V[RJ] : 0.0;                                   // row J of V
    V = __builtin_amdgcn_mfma_f64_16x16x4f64(mv, vrow, V, 0, 0, 0);            // V += m v_J^T
  }
  lcol[RJ] = inrow ? lv : lcol[RJ];                   // column J of L below the diagonal: stored after the sweep by lane row QJ
  rinvs[RJ] = inrow ? rinv : rinvs[RJ];               // rows x = q + 4 rr of this lane: their pivots are seen by lane row q
  bad |= ((__builtin_amdgcn_fcmp(d, 0.0, 2 /* ogt */) >> (16 * QJ)) & 1ull) ? 0u : (1u << J);
  __builtin_amdgcn_sched_barrier(0);
}

template <int... J>
__device__ __forceinline__ void diag16_sweep(double4_t& A, double4_t& V, double (&rinvs)[4], double (&lcol)[4], unsigned& bad, int q, int r,
                                             std::integer_sequence<int, J...>) {
  (diag16_pivot<J>(A, V, rinvs, lcol, bad, q, r), ...);
}

template <int LDD = BLD>   // the leading dimension of D (kernels_vecchia.hip factors images narrower than the 128-wide block)
__device__ __forceinline__ void diag16(double* D, double* Wd, double* wdiag, int* info, int col) {
  const int l = threadIdx.x & 63, r = l & 15, q = l >> 4;
  double4_t A, V;
  double rinvs[4] = {1.0, 1.0, 1.0, 1.0}, lcol[4] = {0.0, 0.0, 0.0, 0.0};
  unsigned bad = 0;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int x = q + 4 * rr;
    A[rr] = (x >= r) ? D[x + r * LDD] : D[r + x * LDD];   // the upper triangle mirrors the lower one
    V[rr] = (x == r) ? 1.0 : 0.0;
  }
  diag16_sweep(A, V, rinvs, lcol, bad, q, r, std::make_integer_sequence<int, 16>{});
  if (bad != 0 && l == 0) atomicCAS(info, 0, col + __builtin_ctz(bad) + 1);  // LAPACK info: first non-PD leading minor
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int x = q + 4 * rr;                        // W[x][r] = rinv_x V[x][r]
    if (r == x) {                                    // the pivot of row x is still where it was read (later updates add l_x l_y with l_x = 0)
      double ljj, rinv;
      sqrt_rsqrt(A[rr], ljj, rinv);
      D[x + x * LDD] = ljj;
    }
    if (r > x) D[r + x * LDD] = lcol[rr];            // column x of L: lane row q = x % 4 kept it
    const double w = (r <= x) ? V[rr] * rinvs[rr] : 0.0;
    Wd[x + r * 16] = w;
    if (r < x) D[r + x * LDD] = w;                    // strict lower part of the inverse, transposed into the upper triangle
    if (r == x) wdiag[x] = w;
  }
}

// 16x16x16 block product on one wave: acc (+/-)= Aop * Bop with Aop[x][k] = pa[x + k*lda_], Bop[k][y] = pb[y + k*ldb_]
// (both operands are addressed "row index contiguous"), acc lane layout D[x = (lane>>4) + 4r][y = lane&15].
template <int NEG>
__device__ __forceinline__ double4_t block_mma(const double* pa, int lda_, const double* pb, int ldb_, double4_t acc) {
  const int l = threadIdx.x & 63, q = l >> 4, r = l & 15;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[r + (4 * kk + q) * lda_], pb[r + (4 * kk + q) * ldb_], acc, 0, 0, NEG);
  return acc;
}

// one 16x16 block of phase C: b < nchol -> Cholesky trailing block, else inverse block (see the kernel)
__device__ __forceinline__ void potf2_phase_c_block(double* S, const double* Wd, int s, int c0, int m, int b, int lane, int q, int r) {
  const int nchol = m * (m + 1) / 2;
  if (b < nchol) {
    int ii = 0;
    while ((ii + 1) * (ii + 2) / 2 <= b) ++ii;
    const int I = s + 1 + ii, J = s + 1 + (b - ii * (ii + 1) / 2);
    // D'[x][y] = C_IJ[y][x]: lanes run down the rows of C_IJ (contiguous in LDS)
    double4_t acc;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) acc[rr] = S[(16 * I + r) + (16 * J + q + 4 * rr) * BLD];
    acc = block_mma<1>(S + 16 * J + c0 * BLD, BLD, S + 16 * I + c0 * BLD, BLD, acc);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) S[(16 * I + r) + (16 * J + q + 4 * rr) * BLD] = acc[rr];
  } else {
    const int e = b - nchol;
    const int I = s + 1 + e / (s + 1), J = e % (s + 1);
    // Y_IJ[a][b'] -= sum_k L_Is[a][k] * X_sJ[k][b'];  Y_IJ[a][b'] sits transposed at S[(16J + b') + (16I + a) * BLD]
    double4_t acc;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) acc[rr] = S[(16 * J + r) + (16 * I + q + 4 * rr) * BLD];
    if (J < s) acc = block_mma<1>(S + 16 * I + c0 * BLD, BLD, S + 16 * J + c0 * BLD, BLD, acc);
    else {  // X_ss = Wd: Bop[k][b'] = Wd[k][b'] = Wd[k + b' * 16]  -> "row index contiguous" means pb[b' + k * ld] with the transposed view
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(S[(16 * I + (lane & 15)) + (c0 + 4 * kk + (lane >> 4)) * BLD],
                                                   Wd[(4 * kk + (lane >> 4)) + (lane & 15) * 16], acc, 0, 0, 1);
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) S[(16 * J + r) + (16 * I + q + 4 * rr) * BLD] = acc[rr];
  }
}

// the body: NW waves (16: the stand-alone kernel; 8: the factor role of panel_fused_kernel), sm = PB_SMEM_DOUBLES doubles
// of LDS.  Which wave computes a 16x16 block has no influence on the block's arithmetic: same bits for any NW.
// ptr (may be null; GPRC_POTF2_TRACE): s_memrealtime stamps of thread 0 -- [0] entry, [1] block loaded, [2] first 16x16 sweep done,
// [3 + 2 s] / [4 + 2 s] after the two barriers of step s, [19] exit (stores issued).  Measurement only.
#define POTF2_STAMP(k) do { if (ptr && threadIdx.x == 0) ptr[k] = __builtin_amdgcn_s_memrealtime(); } while (0)
// preloaded: S already holds the block (gemm_tile_128<.., LDSOUT>), the loads from A are skipped.
// STORE = false (kernels_batch_gpc.hip, which factors again and again and reads the image): L and the inverse stay in the LDS image and
// nothing goes to A or winv, which may be null with `preloaded`; the default is every other caller's code, instruction for instruction.
template <int NW, bool STORE = true>
__device__ __attribute__((noinline)) void potf2_blocked_body(double* sm, double* A, int64_t lda, double* winv, int* info, int col0,
                                                             unsigned long long* ptr = nullptr, bool preloaded = false) {
  static_assert(NW >= 8, "phase B needs one wave per task: 7 tasks per step");
  constexpr int TYS = NW / 2;          // column groups of the 128-row load / store loops (NW * 64 threads / 128 rows)
  double* S = sm;                      // PB x BLD
  double* Wd2 = pb_work(sm);           // 2 x (16 x 16): the 16x16 inverse of step s lives in buffer s & 1
  double* Wdiag = pb_wdiag(sm);        // PB
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int q = lane >> 4, r = lane & 15;
  POTF2_STAMP(0);
  if (!preloaded) {
    // all the loads of a thread's 128 / TYS columns are issued before the first LDS store (the loop with one conditional load
    // per iteration took 4 us of a 46-us block); entries above the diagonal are read too -- allocated storage -- and dropped
    const int i = t & 127, ty = t >> 7;
    constexpr int BATCH = (NW == 8) ? 32 : 16;      // loads in flight per thread (the 16-wave kernel is capped at 128 VGPRs)
    for (int k0 = 0; k0 < PB / TYS; k0 += BATCH) {
      double v[BATCH];
#pragma unroll
      for (int k = 0; k < BATCH; ++k) v[k] = A[i + (int64_t)(ty + TYS * (k0 + k)) * lda];
#pragma unroll
      for (int k = 0; k < BATCH; ++k) S[i + (ty + TYS * (k0 + k)) * BLD] = (i >= ty + TYS * (k0 + k)) ? v[k] : 0.0;
    }
  }
  __syncthreads();
  POTF2_STAMP(1);
  if (wave == 0) diag16(S, Wd2, Wdiag, info, col0);  // phase A of step 0
  __syncthreads();
  POTF2_STAMP(2);
  for (int s = 0; s < 8; ++s) {
    const int c0 = 16 * s, m = 7 - s;
    const double* Wd = Wd2 + (s & 1) * 256;
    // ---- phase B: m blocks of the panel below and s blocks of inverse row s -- always 7 tasks, one wave each
    if (wave < m) {
      const int I = s + 1 + wave;
      // D'[x][y] = sum_k Wd[x][k] * A_I[y][k] = X_I[y][x]
      double4_t acc = block_mma<0>(Wd, 16, S + 16 * I + c0 * BLD, BLD, (double4_t){0.0, 0.0, 0.0, 0.0});
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) S[(16 * I + r) + (c0 + q + 4 * rr) * BLD] = acc[rr];
    } else if (wave - m < s) {
      const int J = wave - m;
      // X_sJ[a][b] = sum_k Wd[a][k] * Y_sJ[k][b]; Y_sJ[k][b] sits transposed at S[(16J + b) + (c0 + k) * BLD]
      double4_t acc = block_mma<0>(Wd, 16, S + 16 * J + c0 * BLD, BLD, (double4_t){0.0, 0.0, 0.0, 0.0});
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) S[(16 * J + r) + (c0 + q + 4 * rr) * BLD] = acc[rr];
    }
    __syncthreads();
    POTF2_STAMP(3 + 2 * s);
    // ---- phase C with look-ahead: m(m+1)/2 Cholesky blocks then m*(s+1) inverse blocks.  Wave 0 takes block 0 -- the
    // next diagonal block (s+1, s+1) -- and goes straight on to phase A of step s+1 (the sequential 16-pivot sweep,
    // the longest single piece of the kernel) while the other waves work through the other blocks; nothing they touch
    // overlaps that block, and its 16x16 inverse goes to the other Wd buffer.
    const int total = m * (m + 1) / 2 + m * (s + 1);
    if (wave == 0) {
      if (s < 7) {
        potf2_phase_c_block(S, Wd, s, c0, m, 0, lane, q, r);
        diag16(S + (c0 + 16) + (c0 + 16) * BLD, Wd2 + ((s + 1) & 1) * 256, Wdiag + c0 + 16, info, col0 + c0 + 16);
      }
    } else {
      for (int b = wave; b < total; b += NW - 1) potf2_phase_c_block(S, Wd, s, c0, m, b, lane, q, r);
    }
    // (a preloaded block's stores to memory -- gemm_tile_128<.., LDSOUT> did not wait for them -- are complete in every wave before
    // this barrier, hence before any wave stores the factored block over them below; free after the first step)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    POTF2_STAMP(4 + 2 * s);
  }
  if constexpr (STORE) {
    const int i = t & 127, ty = t >> 7;
    const double wd = Wdiag[i];
    constexpr int BATCH = 8;
    for (int k0 = 0; k0 < PB / TYS; k0 += BATCH) {  // LDS reads of a batch first (S[c + i BLD]: a row walk, stride BLD), then its stores back to back
      double lv[BATCH], wv[BATCH];
#pragma unroll
      for (int k = 0; k < BATCH; ++k) {
        const int c = ty + TYS * (k0 + k);
        lv[k] = S[i + c * BLD];
        wv[k] = (i > c) ? S[c + i * BLD] : (i == c ? wd : 0.0);
      }
#pragma unroll
      for (int k = 0; k < BATCH; ++k) {
        const int c = ty + TYS * (k0 + k);
        if (i >= c) A[i + (int64_t)c * lda] = lv[k];
        winv[i + c * PB] = wv[k];
      }
    }
  }
  POTF2_STAMP(19);
}

// ------------------------------------------------------------------------------------------------
// GEMM tile core: acc(128x128) = A(128 x K) * B(128 x K)^T, A and B column-major strips.
//
// LDS image per operand and buffer: [KB=16][LDT=144] doubles, i.e. one k-slice of the strip per row
// of 128 contiguous matrix rows + 16 pad.  The pad moves consecutive k-slices by 32 banks, so the
// ds_read_b64 of an MFMA operand (16 matrix rows x 2 k per 32-lane half) is conflict-free, and the
// 16-byte staging stores of one wave cover 1 KiB contiguous.
// MFMA operands are swapped (A-operand <- B strip, B-operand <- A strip): the accumulator then holds
// C[row = 16m + (lane&15)][col = 16n + (lane>>4) + 4r], i.e. 16 consecutive ROWS per lane group,
// which is the contiguous direction of the column-major C tile.
// ------------------------------------------------------------------------------------------------
constexpr int G_KB = 16;
constexpr int G_LDT = 144;
constexpr int G_BUF = G_KB * G_LDT;           // doubles per operand per buffer
constexpr int G_SMEM_DOUBLES = 4 * G_BUF;     // A,B x 2 buffers = 73,728 B -> 2 workgroups per CU
constexpr size_t G_SMEM_BYTES = G_SMEM_DOUBLES * sizeof(double);

// operands of one k-step (4 consecutive k) for this wave's 64x64 sub-tile: 4 A + 4 B doubles per lane
__device__ __forceinline__ void read_ops(const double* Ac, const double* Bc, int kk, double (&a)[4], double (&b)[4]) {
#pragma unroll
  for (int m = 0; m < 4; ++m) a[m] = Ac[kk * 4 * G_LDT + m * 16];
#pragma unroll
  for (int n = 0; n < 4; ++n) b[n] = Bc[kk * 4 * G_LDT + n * 16];
}
// NEG = 1 sets the f64 MFMA's negate-A bit (the BLGP field is the NEG set on f64 MFMA; verified on gfx950 by
// tools/microbench/mfma_neg.hip): acc = acc - op_a * op_b, exactly.
template <int NEG>
__device__ __forceinline__ void mma_step(const double (&a)[4], const double (&b)[4], double4_t (&acc)[4][4]) {
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(b[n], a[m], acc[m][n], 0, 0, NEG);
}

// LDS-DMA of one k-tile of both strips: wave w moves k-slices w, w+4, w+8, w+12 of A and of B; one
// global_load_lds_dwordx4 per slice = 64 lanes x 16 B = the slice's 128 rows, landing contiguously at a
// wave-uniform LDS row (the 128-byte row pad survives because a row is exactly one instruction).
typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
__device__ __forceinline__ void dma_ktile(const double* Ag, int64_t lda, const double* Bg, int64_t ldb, double* Asb, double* Bsb) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    __builtin_amdgcn_global_load_lds((gptr_t)(Ag + (int64_t)(4 * i) * lda), (lptr_t)(Asb + 4 * i * G_LDT), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gptr_t)(Bg + (int64_t)(4 * i) * ldb), (lptr_t)(Bsb + 4 * i * G_LDT), 16, 0, 0);
  }
}

// Where k-tile kt of an operand strip lives (this lane's 16 bytes of k-slice `wave`).  Plain: a column-major strip with
// one leading dimension.  SEG: the strip is rows [brow, brow + 128) of the PACKED factor across its first K columns
// (B = packed base, ldb = n_pad): every NB columns it moves to the next panel, with that panel's own leading dimension.
template <bool SEG>
__device__ __forceinline__ const double* strip_ktile(const double* B, int64_t ldb, int64_t brow, int kt, int lane, int wave, int64_t& ld) {
  if constexpr (SEG) {
    const int pp = kt / (NB / 16);                    // panel that holds k-tile kt
    ld = panel_ld(ldb, pp);
    return B + panel_offset(ldb, pp) + (brow - (int64_t)pp * NB) + (int64_t)((kt % (NB / 16)) * 16 + wave) * ld + 2 * lane;
  } else {
    ld = ldb;
    return B + 2 * lane + (int64_t)(kt * 16 + wave) * ldb;
  }
}

// The same place WITHOUT the lane's part: the wave-uniform address of k-slice `wave` of k-tile kt (the lane adds 16 bytes x lane as a
// 32-bit VGPR offset of the LDS-DMA instruction, whose base is then an SGPR pair: no VALU address arithmetic in the loop).
template <bool SEG>
__device__ __forceinline__ const char* strip_ktile_s(const double* B, int64_t ldb, int64_t brow, int kt, int wave, int64_t& ld) {
  if constexpr (SEG) {
    const int pp = kt / (NB / 16);
    ld = panel_ld(ldb, pp);
    return reinterpret_cast<const char*>(B + panel_offset(ldb, pp) + (brow - (int64_t)pp * NB) + (int64_t)((kt % (NB / 16)) * 16 + wave) * ld);
  } else {
    ld = ldb;
    return reinterpret_cast<const char*>(B + (int64_t)(kt * 16 + wave) * ldb);
  }
}

// SSQ (the predict's panel solve only): besides storing the tile, leave in ssq[0..127] the sum of squares of each of the
// tile's 128 rows over its 128 columns -- these columns of v^T are final after this tile, so colSums(v * v)
// (R/GPRclass.R:164) is assembled from these per-block partials and the pass that re-read the whole solved chunk is gone.
// Fixed order: a lane's 16 columns (n, r ascending), the four lanes of a row (xor 16, xor 32), the two column waves.
// LDSOUT: the finished tile ALSO goes to lds_out as the 128 x 128 LDS image potf2_blocked_body works on (leading dimension 144,
// zero above the diagonal) -- the factor role hands the updated diagonal block to the factorisation without the round trip
// through memory (one more workgroup barrier than without: every wave must be past its last operand read, the image overlaps
// the staging buffers).
// ILV: the main loop with every non-MFMA instruction in the shadow of an MFMA (below) -- the throughput kernels; false keeps the
// block-structured loop for the roles of the fused panel / service kernels, which inline this function several times and spill
// with the larger body (their tiles are short -- K = 128..384 -- and paced by flags, not by the loop).
// CORE (interleaved loops only): 2 = the loop without VALU instructions (the plain throughput kernels), 1 = the first interleaved loop
// (kept for the tiles that run beside the factor service -- sweep kernel, trailing_service_kernel: measured, see the loops' comments).
// WT: the tile is stored WRITE-THROUGH (sc1: global_store ... sc1, the agent-scope relaxed atomic store), leaving no dirty line in the XCD's L2.
template <bool SET, bool SEG = false, bool SEGA = false, bool SSQ = false, bool LDSOUT = false, bool ILV = true, int CORE = 2, bool WT = false>
__device__ __forceinline__ void gemm_tile_128(double* C, int64_t ldc, const double* A, int64_t lda, const double* B,
                                              int64_t ldb, int K, double* smem, int64_t brow = 0, int64_t arow = 0, int kt0 = 0,
                                              double* ssq = nullptr, int tid = -1, double* lds_out = nullptr) {
  const int t = tid < 0 ? (int)threadIdx.x : tid, lane = t & 63;   // tid: a 256-thread team inside a larger workgroup
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  const int fk = lane >> 4, fr = lane & 15;
  double* As = smem;
  double* Bs = smem + 2 * G_BUF;

  // C -= A*B^T: the accumulators START as the C tile (its loads fly with the first DMA) and every MFMA
  // subtracts, so the epilogue is stores only.  SET: accumulators start at zero, plain products.
  constexpr int NEG = SET ? 0 : 1;
  double* Cw = C + (wr * 64 + fr) + (int64_t)(wc * 64 + fk) * ldc;
  double4_t acc[4][4];
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int m = 0; m < 4; ++m) acc[m][n][r] = SET ? 0.0 : Cw[m * 16 + (int64_t)(n * 16 + 4 * r) * ldc];

  int64_t ldak, ldbk;
  // kt0 (first k-tile of the pass) addresses the PACKED operands only: a plain strip is handed over already pointing at
  // its first k-tile (the running pointer below restarts from it)
  const double* Ag = strip_ktile<SEGA>(A, lda, arow, SEGA ? kt0 : 0, lane, wave, ldak);  // this lane's 16 bytes of k-slice `wave`
  const double* Bg = strip_ktile<SEG>(B, ldb, brow, SEG ? kt0 : 0, lane, wave, ldbk);
  const int srow = wave * G_LDT;                          // LDS row of that slice (wave-uniform)
  const int foff = fr + fk * G_LDT;                       // this lane's MFMA operand element

  // Software pipeline, operand reads TWO k-steps ahead.  Four named operand sets (one per k-step of a tile).
  // Every k-step is:  s_waitcnt lgkmcnt(0)  ->  issue the reads of step +2  ->  16 MFMAs of this step.
  // The wait therefore only ever covers reads issued one whole MFMA block (>= 1000 cycles) earlier; with the
  // reads issued right in front of the compiler's own lgkmcnt(0) they were waited for on the spot.
  //   step (t,0): reads (t,2)          step (t,1): reads (t,3)   <- last LDS reads of tile t's buffer
  //   step (t,2): vmcnt(0) + barrier [tile t+1 landed, tile t's buffer drained]; DMA tile t+2; reads (t+1,0)
  //   step (t,3): reads (t+1,1)
  // so a DMA has 64 MFMAs (4096 cycles) to land, as before.
  constexpr int LGKM0 = 0xC07F;  // s_waitcnt lgkmcnt(0), vmcnt/expcnt untouched
  const int KT = K / G_KB;
  dma_ktile(Ag, ldak, Bg, ldbk, As + srow, Bs + srow);
  // vmcnt(0) through the BUILTIN, not inline asm, so that the compiler's waitcnt pass knows the C-tile loads
  // above have completed and does not re-wait vmcnt(0) (draining fresh DMAs) inside the loop.  0x0F70 = vmcnt(0).
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __syncthreads();
  if (KT > 1) {
    Ag = strip_ktile<SEGA>(A, lda, arow, (SEGA ? kt0 : 0) + 1, lane, wave, ldak);
    Bg = strip_ktile<SEG>(B, ldb, brow, (SEG ? kt0 : 0) + 1, lane, wave, ldbk);
    dma_ktile(Ag, ldak, Bg, ldbk, As + G_BUF + srow, Bs + G_BUF + srow);
  }
  if constexpr (!SEGA) Ag = A + 2 * lane + (int64_t)(2 * G_KB + wave) * lda;  // next tile to request: kt + 2
  if constexpr (!SEG) Bg = B + 2 * lane + (int64_t)(2 * G_KB + wave) * ldb;
  double a0[4], b0[4], a1[4], b1[4], a2[4], b2[4], a3[4], b3[4];
  read_ops(As + wr * 64 + foff, Bs + wc * 64 + foff, 0, a0, b0);
  read_ops(As + wr * 64 + foff, Bs + wc * 64 + foff, 1, a1, b1);
  if constexpr (ILV && CORE == 2) {
  // ---- Main loop (round 3, second form): no VALU instruction but the MFMAs ------------------------------------------------------
  // An f64 MFMA executes on the SIMD's double-precision lanes, and a VALU instruction issued behind it -- a 32-bit address add as
  // much as an FMA -- takes the pipe away from the next MFMA: tools/microbench/mfma_valu_mix.hip measures 64 cycles per MFMA for a
  // pure stream, +14 with one v_add_u32 behind each MFMA, +18 with two; SALU and LDS instructions cost nothing.  The first
  // interleaved loop still carried ~20 VALU instructions per k-tile and wave (ISA: 8 v_lshl_add_u64 for the LDS-DMA addresses, 12
  // v_add_u32 / v_subrev_u32 for the ds_read2 bases) -- ~5 % of the pipe.  Here the loop has none:
  //   * LDS-DMA with an SGPR base: global_load_lds_dwordx4 v_off, s[base:base+1] -- the k-slice's address is wave-uniform, the lane
  //     contributes a constant 32-bit offset (16 B x lane); the compiler has no such selection for the builtin, hence inline assembly
  //     (m0 = the slice's LDS row, set by s_mov in the same statement);
  //   * operand reads as ds_read_b64 with 16-bit immediate offsets from TWO loop-invariant base registers (one per operand): every
  //     buffer / k-step / block offset is a constant of the instruction once the loop is unrolled by two k-tiles (ds_read2_b64's 8-bit
  //     offsets reach 2 KB only, and the compiler paid a v_add_u32 per pair for them);
  //   * the waits for those reads counted by hand (the compiler does not see assembly loads): the reads of a k-step are issued two
  //     blocks ahead, eight per block, in order: s_waitcnt lgkmcnt(8) in front of a block leaves exactly the next block's in flight.
  // Same products, same k order, same accumulators as before: identical bits.
  const unsigned lane_off = 16u * (unsigned)lane;
  const unsigned ldsA = (unsigned)(uintptr_t)(lptr_t)(As + srow), ldsB = (unsigned)(uintptr_t)(lptr_t)(Bs + srow);                    // wave-uniform
  const unsigned aBase = (unsigned)(uintptr_t)(lptr_t)(As + wr * 64 + foff), bBase = (unsigned)(uintptr_t)(lptr_t)(Bs + wc * 64 + foff);  // per lane
  // next tile to request (k-tile 2): wave-uniform addresses
  int64_t ldas, ldbs;
  const char* Asg = strip_ktile_s<SEGA>(A, lda, arow, (SEGA ? kt0 : 0) + 2, wave, ldas);
  const char* Bsg = strip_ktile_s<SEG>(B, ldb, brow, (SEG ? kt0 : 0) + 2, wave, ldbs);
#define GPRC_SB __builtin_amdgcn_sched_barrier(0);
#define GPRC_M(A_, B_, i) acc[(i) >> 2][(i) & 3] = __builtin_amdgcn_mfma_f64_16x16x4f64(B_[(i) & 3], A_[(i) >> 2], acc[(i) >> 2][(i) & 3], 0, 0, NEG); GPRC_SB
#define GPRC_RD(dst, base, off) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(dst) : "v"(base), "n"(off));
  // two reads (blocks 2r, 2r+1) of k-step kk in buffer buf
#define GPRC_RA(buf, kk, r, A_) GPRC_RD(A_[2 * (r)], aBase, ((buf) * G_BUF + (kk) * 4 * G_LDT + (2 * (r)) * 16) * 8) GPRC_RD(A_[2 * (r) + 1], aBase, ((buf) * G_BUF + (kk) * 4 * G_LDT + (2 * (r) + 1) * 16) * 8) GPRC_SB
#define GPRC_RB(buf, kk, r, B_) GPRC_RD(B_[2 * (r)], bBase, ((buf) * G_BUF + (kk) * 4 * G_LDT + (2 * (r)) * 16) * 8) GPRC_RD(B_[2 * (r) + 1], bBase, ((buf) * G_BUF + (kk) * 4 * G_LDT + (2 * (r) + 1) * 16) * 8) GPRC_SB
#define GPRC_READY(cnt, A_, B_) asm volatile("s_waitcnt lgkmcnt(" #cnt ")" : "+v"(A_[0]), "+v"(A_[1]), "+v"(A_[2]), "+v"(A_[3]), "+v"(B_[0]), "+v"(B_[1]), "+v"(B_[2]), "+v"(B_[3])); GPRC_SB
#define GPRC_BLOCK_R(A_, B_, buf, kk, RA_, RB_, cond)                                                               \
  GPRC_M(A_, B_, 0) GPRC_M(A_, B_, 1) if (cond) { GPRC_RA(buf, kk, 0, RA_) }                                        \
  GPRC_M(A_, B_, 2) GPRC_M(A_, B_, 3) if (cond) { GPRC_RA(buf, kk, 1, RA_) }                                        \
  GPRC_M(A_, B_, 4) GPRC_M(A_, B_, 5) if (cond) { GPRC_RB(buf, kk, 0, RB_) }                                        \
  GPRC_M(A_, B_, 6) GPRC_M(A_, B_, 7) if (cond) { GPRC_RB(buf, kk, 1, RB_) }                                        \
  GPRC_M(A_, B_, 8) GPRC_M(A_, B_, 9) GPRC_M(A_, B_, 10) GPRC_M(A_, B_, 11) GPRC_M(A_, B_, 12) GPRC_M(A_, B_, 13) GPRC_M(A_, B_, 14) GPRC_M(A_, B_, 15)
  // one LDS-DMA: k-slice wave + 4 i of the tile at Asg / Bsg into buffer buf (m0 <- the slice's LDS row; one wait state before its use)
#define GPRC_DMA(i, buf, more2)                                                                                      \
  if (more2) {                                                                                                      \
    if ((i) < 4) asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(lane_off), "s"(Asg + (int64_t)(4 * (i)) * ldas * 8), "s"(ldsA + (unsigned)(((buf) * G_BUF + 4 * (i) * G_LDT) * 8)) : "memory"); \
    else asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(lane_off), "s"(Bsg + (int64_t)(4 * ((i) - 4)) * ldbs * 8), "s"(ldsB + (unsigned)(((buf) * G_BUF + 4 * ((i) - 4) * G_LDT) * 8)) : "memory"); \
    GPRC_SB                                                                                                         \
  }
  // one k-tile in buffer buf (the next one in 1 - buf); more1 / more2: a tile kt+1 / kt+2 exists; kt: this tile's index
#define GPRC_KTILE(buf, more1, more2)                                                                                \
  {                                                                                                                 \
    GPRC_SB                                                                                                         \
    GPRC_READY(8, a0, b0)                                                                                           \
    GPRC_BLOCK_R(a0, b0, buf, 2, a2, b2, true)                                                                      \
    GPRC_READY(8, a1, b1)                                                                                           \
    GPRC_BLOCK_R(a1, b1, buf, 3, a3, b3, true)                                                                      \
    GPRC_READY(8, a2, b2)                                                                                           \
    GPRC_M(a2, b2, 0) GPRC_M(a2, b2, 1) GPRC_M(a2, b2, 2) GPRC_M(a2, b2, 3)                                         \
    if (more1) {                                                                                                    \
      /* this wave's reads of buffer buf have returned (lgkmcnt) and its share of tile kt+1 has landed (vmcnt); after the */ \
      /* barrier that holds for every wave: tile kt+1 may be read and buffer buf overwritten */                     \
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                                   \
      __builtin_amdgcn_s_barrier();                                                                                 \
      GPRC_SB                                                                                                       \
    }                                                                                                               \
    GPRC_M(a2, b2, 4) if (more1) { GPRC_RA(1 - (buf), 0, 0, a0) }                                                   \
    GPRC_M(a2, b2, 5) if (more1) { GPRC_RA(1 - (buf), 0, 1, a0) }                                                   \
    GPRC_M(a2, b2, 6) if (more1) { GPRC_RB(1 - (buf), 0, 0, b0) }                                                   \
    GPRC_M(a2, b2, 7) if (more1) { GPRC_RB(1 - (buf), 0, 1, b0) }                                                   \
    GPRC_M(a2, b2, 8) GPRC_DMA(0, buf, more2) GPRC_M(a2, b2, 9) GPRC_DMA(4, buf, more2) GPRC_M(a2, b2, 10) GPRC_DMA(1, buf, more2) GPRC_M(a2, b2, 11) GPRC_DMA(5, buf, more2) \
    GPRC_M(a2, b2, 12) GPRC_DMA(2, buf, more2) GPRC_M(a2, b2, 13) GPRC_DMA(6, buf, more2) GPRC_M(a2, b2, 14) GPRC_DMA(3, buf, more2) GPRC_M(a2, b2, 15) GPRC_DMA(7, buf, more2) \
    if (more2) {   /* the tile after the one just requested: 16 columns on, or the next panel of a packed strip (scalar arithmetic) */ \
      if constexpr (SEGA) { if (((kt0 + kt + 3) % (NB / 16)) == 0) Asg = strip_ktile_s<true>(A, lda, arow, kt0 + kt + 3, wave, ldas); else Asg += (int64_t)G_KB * ldas * 8; } \
      else Asg += (int64_t)G_KB * ldas * 8;                                                                         \
      if constexpr (SEG) { if (((kt0 + kt + 3) % (NB / 16)) == 0) Bsg = strip_ktile_s<true>(B, ldb, brow, kt0 + kt + 3, wave, ldbs); else Bsg += (int64_t)G_KB * ldbs * 8; } \
      else Bsg += (int64_t)G_KB * ldbs * 8;                                                                         \
      GPRC_SB                                                                                                       \
    }                                                                                                               \
    if (more1) { GPRC_READY(8, a3, b3) } else { GPRC_READY(0, a3, b3) }                                             \
    GPRC_BLOCK_R(a3, b3, 1 - (buf), 1, a1, b1, more1)                                                               \
  }
  {   // KT is even and >= 4: every caller's K is a multiple of 128 (eight k-tiles); launch_gemm_nt, the one launcher with a free K, checks it
    int kt = 0;
    for (; kt + 2 < KT; kt += 2) {
      GPRC_KTILE(0, true, true)
      ++kt;
      GPRC_KTILE(1, true, true)
      --kt;
    }
    GPRC_KTILE(0, true, false)
    ++kt;
    GPRC_KTILE(1, false, false)
  }
#undef GPRC_KTILE
#undef GPRC_DMA
#undef GPRC_BLOCK_R
#undef GPRC_READY
#undef GPRC_RA
#undef GPRC_RB
#undef GPRC_RD
#undef GPRC_M
#undef GPRC_SB
  } else if constexpr (ILV) {
  // ---- Main loop, every non-MFMA instruction in the shadow of an MFMA (round 3, first form) -----------------------------------
  // (Still ~20 VALU instructions per k-tile and wave.  It stays for the K = 512 tiles of the kernels that run BESIDE the factor
  //  service: with the VALU-free loop their tiles are a third faster, the memory system correspondingly busier, and the service's
  //  latency-bound roles -- and with them the whole mid-size factorisation -- slower: n = 12288 13.55 -> 14.66 ms, 16384 27.44 -> 28.27,
  //  same box, profiles/r03_factor_schedules.txt.)
  // Counters on the shipped loop (profiles/r03_c4_core_counters.txt): the MFMA pipes were busy 91.7 % of the kernel's cycles at
  // 2.37 GHz, and per 64 MFMAs a wave issues 73 other instructions -- 16 ds_read2, 8 LDS-DMA with their m0 / address set-up, the
  // s_waitcnt / s_barrier, loop arithmetic.  In the block-structured loop they sat in CLUMPS between the 16-MFMA blocks: four
  // operand-read groups and, once per k-tile, vmcnt(0) + barrier + 8 DMA issues + 4 reads with nothing but the block's last MFMA
  // in flight.  A wave is in order: while it works through a clump it issues no MFMA, and its SIMD's pipe runs dry unless the
  // partner wave happens to be inside a block (a wave alone on its SIMD reached 75 %).  Here every MFMA is followed by at most
  // one other operation (a ds_read2, or one DMA with its set-up), the barrier sits BETWEEN two MFMAs of block 2 with four MFMAs
  // of the same wave still queued on the pipe, and the order is pinned by a sched_barrier after every statement.  The products,
  // their k order and the accumulator each one lands in are unchanged: identical bits.
  //   block 0 (a0,b0): reads (t,2) after MFMAs 1,3,5,7          block 1 (a1,b1): reads (t,3) after 1,3,5,7
  //   block 2 (a2,b2): MFMAs 0-3 | lgkmcnt(0) vmcnt(0) s_barrier | reads (t+1,0) after 4,5,6,7 | DMA slice i of tile t+2 after 8+i
  //   block 3 (a3,b3): reads (t+1,1) after 1,3,5,7
#define GPRC_SB __builtin_amdgcn_sched_barrier(0);
#define GPRC_M(A_, B_, i) acc[(i) >> 2][(i) & 3] = __builtin_amdgcn_mfma_f64_16x16x4f64(B_[(i) & 3], A_[(i) >> 2], acc[(i) >> 2][(i) & 3], 0, 0, NEG); GPRC_SB
  // one ds_read2_b64 each: RA r = 0, 1 -> a[2r], a[2r+1]; RB r = 0, 1 -> b[2r], b[2r+1]
#define GPRC_RA(Ap_, kk, r, A_) A_[2 * (r)] = (Ap_)[(kk) * 4 * G_LDT + (2 * (r)) * 16]; A_[2 * (r) + 1] = (Ap_)[(kk) * 4 * G_LDT + (2 * (r) + 1) * 16]; GPRC_SB
#define GPRC_RB(Bp_, kk, r, B_) B_[2 * (r)] = (Bp_)[(kk) * 4 * G_LDT + (2 * (r)) * 16]; B_[2 * (r) + 1] = (Bp_)[(kk) * 4 * G_LDT + (2 * (r) + 1) * 16]; GPRC_SB
#define GPRC_BLOCK_R(A_, B_, Ap_, Bp_, kk, RA_, RB_, cond)                                                          \
  GPRC_M(A_, B_, 0) GPRC_M(A_, B_, 1) if (cond) { GPRC_RA(Ap_, kk, 0, RA_) }                                        \
  GPRC_M(A_, B_, 2) GPRC_M(A_, B_, 3) if (cond) { GPRC_RA(Ap_, kk, 1, RA_) }                                        \
  GPRC_M(A_, B_, 4) GPRC_M(A_, B_, 5) if (cond) { GPRC_RB(Bp_, kk, 0, RB_) }                                        \
  GPRC_M(A_, B_, 6) GPRC_M(A_, B_, 7) if (cond) { GPRC_RB(Bp_, kk, 1, RB_) }                                        \
  GPRC_M(A_, B_, 8) GPRC_M(A_, B_, 9) GPRC_M(A_, B_, 10) GPRC_M(A_, B_, 11) GPRC_M(A_, B_, 12) GPRC_M(A_, B_, 13) GPRC_M(A_, B_, 14) GPRC_M(A_, B_, 15)
#define GPRC_DMA(i, more2)                                                                                           \
  if (more2) {                                                                                                      \
    if ((i) < 4) __builtin_amdgcn_global_load_lds((gptr_t)(Ag + (int64_t)(4 * (i)) * ldak), (lptr_t)(As + cur + srow + 4 * (i) * G_LDT), 16, 0, 0); \
    else __builtin_amdgcn_global_load_lds((gptr_t)(Bg + (int64_t)(4 * ((i) - 4)) * ldbk), (lptr_t)(Bs + cur + srow + 4 * ((i) - 4) * G_LDT), 16, 0, 0); \
    GPRC_SB                                                                                                         \
  }
  // one k-tile; more1 / more2: a tile kt+1 / kt+2 exists (compile-time true in the steady-state loop, so that it has no branches)
#define GPRC_KTILE(more1, more2)                                                                                     \
  {                                                                                                                 \
    const int cur = (kt & 1) * G_BUF, nxt = G_BUF - cur;                                                            \
    const double* Ac = As + cur + wr * 64 + foff;                                                                   \
    const double* Bc = Bs + cur + wc * 64 + foff;                                                                   \
    const double* An = As + nxt + wr * 64 + foff;                                                                   \
    const double* Bn = Bs + nxt + wc * 64 + foff;                                                                   \
    GPRC_SB                                                                                                         \
    GPRC_BLOCK_R(a0, b0, Ac, Bc, 2, a2, b2, true)                                                                   \
    GPRC_BLOCK_R(a1, b1, Ac, Bc, 3, a3, b3, true)                                                                   \
    GPRC_M(a2, b2, 0) GPRC_M(a2, b2, 1) GPRC_M(a2, b2, 2) GPRC_M(a2, b2, 3)                                         \
    if (more1) {                                                                                                    \
      /* this wave's reads of buffer `cur` have returned (lgkmcnt) and its share of tile kt+1 has landed (vmcnt); after the */ \
      /* barrier that holds for every wave: tile kt+1 may be read and buffer `cur` overwritten */                   \
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                                   \
      __builtin_amdgcn_s_barrier();                                                                                 \
      GPRC_SB                                                                                                       \
      if (more2) {                                                                                                  \
        if constexpr (SEGA || SEG) {                                                                                \
          const bool boundary = ((kt0 + kt + 2) % (NB / 16)) == 0;                                                  \
          if constexpr (SEGA) { if (boundary) Ag = strip_ktile<true>(A, lda, arow, kt0 + kt + 2, lane, wave, ldak); else Ag += (int64_t)G_KB * ldak; } \
          if constexpr (SEG) { if (boundary) Bg = strip_ktile<true>(B, ldb, brow, kt0 + kt + 2, lane, wave, ldbk); else Bg += (int64_t)G_KB * ldbk; } \
        }                                                                                                           \
        GPRC_SB                                                                                                     \
      }                                                                                                             \
    }                                                                                                               \
    GPRC_M(a2, b2, 4) if (more1) { GPRC_RA(An, 0, 0, a0) }                                                          \
    GPRC_M(a2, b2, 5) if (more1) { GPRC_RA(An, 0, 1, a0) }                                                          \
    GPRC_M(a2, b2, 6) if (more1) { GPRC_RB(Bn, 0, 0, b0) }                                                          \
    GPRC_M(a2, b2, 7) if (more1) { GPRC_RB(Bn, 0, 1, b0) }                                                          \
    GPRC_M(a2, b2, 8) GPRC_DMA(0, more2) GPRC_M(a2, b2, 9) GPRC_DMA(4, more2) GPRC_M(a2, b2, 10) GPRC_DMA(1, more2) GPRC_M(a2, b2, 11) GPRC_DMA(5, more2) \
    GPRC_M(a2, b2, 12) GPRC_DMA(2, more2) GPRC_M(a2, b2, 13) GPRC_DMA(6, more2) GPRC_M(a2, b2, 14) GPRC_DMA(3, more2) GPRC_M(a2, b2, 15) GPRC_DMA(7, more2) \
    if (more2) {                                                                                                    \
      if constexpr (!SEGA) Ag += (int64_t)G_KB * lda;                                                               \
      if constexpr (!SEG) Bg += (int64_t)G_KB * ldb;                                                                \
    }                                                                                                               \
    GPRC_BLOCK_R(a3, b3, An, Bn, 1, a1, b1, more1)                                                                  \
  }
  {
    int kt = 0;
    for (; kt + 2 < KT; ++kt) GPRC_KTILE(true, true)
    for (; kt < KT; ++kt) {
      const bool more1 = kt + 1 < KT;
      GPRC_KTILE(more1, false)
    }
  }
#undef GPRC_KTILE
#undef GPRC_DMA
#undef GPRC_BLOCK_R
#undef GPRC_RA
#undef GPRC_RB
#undef GPRC_M
#undef GPRC_SB
  } else {   // the block-structured loop
  for (int kt = 0; kt < KT; ++kt) {
    const int cur = (kt & 1) * G_BUF, nxt = G_BUF - cur;
    const double* Ac = As + cur + wr * 64 + foff;
    const double* Bc = Bs + cur + wc * 64 + foff;
    const double* An = As + nxt + wr * 64 + foff;
    const double* Bn = Bs + nxt + wc * 64 + foff;
    // sched_barrier(0) after every MFMA block: register-only MFMAs otherwise drift across the explicit waits and
    // the compiler merges blocks, putting the reads back in front of a wait
    __builtin_amdgcn_s_waitcnt(LGKM0);
    read_ops(Ac, Bc, 2, a2, b2);
    mma_step<NEG>(a0, b0, acc);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(LGKM0);
    read_ops(Ac, Bc, 3, a3, b3);
    mma_step<NEG>(a1, b1, acc);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(LGKM0);
    if (kt + 1 < KT) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // tile kt+1 has landed (this wave's share)
      __syncthreads();                                   // ... everyone's share; and buffer `cur` is drained
      if (kt + 2 < KT) {
        // packed operands: inside a panel the next k-tile is 16 columns further on (same leading dimension); only at a
        // panel boundary (every NB / 16 k-tiles) is the address rebuilt from the panel geometry -- the full index
        // arithmetic (64-bit multiplies) on every k-tile cost ~2 % of the long-K passes
        if constexpr (SEGA || SEG) {
          const bool boundary = ((kt0 + kt + 2) % (NB / 16)) == 0;
          if constexpr (SEGA) { if (boundary) Ag = strip_ktile<true>(A, lda, arow, kt0 + kt + 2, lane, wave, ldak); else Ag += (int64_t)G_KB * ldak; }
          if constexpr (SEG) { if (boundary) Bg = strip_ktile<true>(B, ldb, brow, kt0 + kt + 2, lane, wave, ldbk); else Bg += (int64_t)G_KB * ldbk; }
        }
        dma_ktile(Ag, ldak, Bg, ldbk, As + cur + srow, Bs + cur + srow);
        if constexpr (!SEGA) Ag += (int64_t)G_KB * lda;
        if constexpr (!SEG) Bg += (int64_t)G_KB * ldb;
      }
      read_ops(An, Bn, 0, a0, b0);
    }
    mma_step<NEG>(a2, b2, acc);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(LGKM0);
    if (kt + 1 < KT) read_ops(An, Bn, 1, a1, b1);
    mma_step<NEG>(a3, b3, acc);
    __builtin_amdgcn_sched_barrier(0);
  }

  }

#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        if constexpr (WT) __hip_atomic_store(&Cw[m * 16 + (int64_t)(n * 16 + 4 * r) * ldc], acc[m][n][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else Cw[m * 16 + (int64_t)(n * 16 + 4 * r) * ldc] = acc[m][n][r];
      }

  if constexpr (LDSOUT) {
    __syncthreads();  // every wave is past its last operand read: the staging buffers are free
    constexpr int LDO = 144;
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const int row = wr * 64 + fr + m * 16, col = wc * 64 + fk + n * 16 + 4 * r;
          lds_out[row + col * LDO] = (row >= col) ? acc[m][n][r] : 0.0;
        }
  }

  if constexpr (SSQ) {
    double rs[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      double q = 0.0;
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) q = fma(acc[m][n][r], acc[m][n][r], q);
      q += __shfl_xor(q, 16, 64);
      q += __shfl_xor(q, 32, 64);
      rs[m] = q;
    }
    __syncthreads();  // every wave is past its last operand read: the staging buffers are free
    if (fk == 0) {
#pragma unroll
      for (int m = 0; m < 4; ++m) smem[wc * 128 + wr * 64 + m * 16 + fr] = rs[m];
    }
    __syncthreads();
    if (t < 128) ssq[t] = smem[t] + smem[128 + t];
  }
}

// blockIdx -> logical id so that each XCD (blocks b, b+8, ... share one) owns a contiguous id range
__device__ __forceinline__ unsigned xcd_remap(unsigned bid, unsigned nwg) {
  const unsigned q = nwg >> 3, r = nwg & 7, x = bid & 7;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}

// Tile of a tiles_m x tiles_n grid visited in groups of `group` tile rows, down the rows inside a group: the tiles an XCD runs
// concurrently then share few operand strips.
__device__ __forceinline__ void group_tile(unsigned id, int tiles_m, int tiles_n, int group, int& tr, int& tc) {
  const int width = group * tiles_n;
  const int g = id / width, first_m = g * group;
  const int gsize = (tiles_m - first_m < group) ? (tiles_m - first_m) : group;
  tr = first_m + (int)(id % width) % gsize;
  tc = (int)(id % width) / gsize;
}

// Lower 128 x 128 tiles of a packed panel's diagonal NB x NB block, by rows: (0,0) (1,0) (1,1) (2,0) ...
constexpr int PANEL_DIAG_TILES = TPP * (TPP + 1) / 2;
__device__ __forceinline__ void diag_tile(int id, int& tr, int& tc) {
  tr = 0;
  while ((tr + 1) * (tr + 2) / 2 <= id) ++tr;
  tc = id - tr * (tr + 1) / 2;
}
// ... and of the whole panel (panel_tiles(P, q) of them): the diagonal block's, then TPP per 128-row strip below it
__device__ __forceinline__ void panel_tile(int id, int& tr, int& tc) {
  if (id < PANEL_DIAG_TILES) diag_tile(id, tr, tc);
  else {
    tr = TPP + (id - PANEL_DIAG_TILES) / TPP;
    tc = (id - PANEL_DIAG_TILES) % TPP;
  }
}
// id over the lower tiles of the target panels q_begin, q_begin + q_stride, ... (n_targets of them) -> the target panel q and, in id,
// the tile's index inside it; false: id lies behind the last target
__device__ __forceinline__ bool target_tile(int& id, int P, int q_begin, int q_stride, int n_targets, int& q) {
  q = q_begin;
  int s = 0;
  for (; s < n_targets; ++s, q += q_stride) {
    const int tq = panel_tiles(P, q);
    if (id < tq) break;
    id -= tq;
  }
  return s < n_targets;
}

}  // namespace
}  // namespace gprc
