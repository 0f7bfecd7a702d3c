// kernels_gemm.hip -- the fp64 Cholesky's kernels WITHOUT flags between workgroups, each with its launcher: every one is a grid of
// independent gemm_tile_128 tiles (chol_tile.h).  The panel solve X := X * Winv^T, in-panel / general C -= A*B^T, the trailing updates
// over the packed block-column layout (lower tiles only; one source panel, or a range of them in one pass), and the predict's
// left-looking and in-panel solve passes.  What shares PanelSync flags and wait records lives in kernels_chol.hip.
#include <algorithm>

#include "chol_tile.h"

namespace gprc {
namespace {

// C[M x N] -= A * B^T, 1-D grid of (M/128)*(N/128) tiles visited in 8-row groups.  ROLE only gives
// each use its own symbol (rocprof / event profiler tell them apart): in-panel update (K = 128),
// predict-side right update (K = 512), posterior-covariance SYRK (K = n).
template <int ROLE>
__global__ __launch_bounds__(256, 2) void gemm_nt_kernel(double* C, int64_t ldc, const double* A, int64_t lda,
                                                         const double* B, int64_t ldb, int tiles_m, int tiles_n, int K,
                                                         int lower, int group) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  // One tile per workgroup (gridDim.x == ntiles); a smaller grid would walk the tile list with its stride (measured 4 % slower with 512
  // workgroups: DESIGN.md 3).
  const unsigned ntiles = (unsigned)tiles_m * (unsigned)tiles_n;
  for (unsigned t = blockIdx.x; t < ntiles; t += gridDim.x) {
    // (PK_INV_GEMM: a tile's length falls with its row, so the ids stay round-robin over the XCDs -- every XCD the same mix, as solve_left_kernel)
    const unsigned id = ROLE == PK_INV_GEMM ? t : xcd_remap(t, ntiles);
    int tr, tc;
    group_tile(id, tiles_m, tiles_n, group, tr, tc);
    if (lower && tc > tr) continue;
    // PK_INV_GEMM (K_y^-1 = L^-T L^-1, A = B = L^-T, lower tiles): rows tr 128.. of an UPPER-triangular matrix are zero left of
    // column tr 128 >= tc 128, so the products start there -- n^3 / 3 instead of n^3; what is skipped is exact zeros
    const int64_t k0 = ROLE == PK_INV_GEMM ? (int64_t)tr * 128 : 0;
    gemm_tile_128<false>(C + (int64_t)tr * 128 + (int64_t)tc * 128 * ldc, ldc, A + (int64_t)tr * 128 + k0 * lda, lda,
                         B + (int64_t)tc * 128 + k0 * ldb, ldb, K - (int)k0, smem);
    __syncthreads();  // every wave has left the tile (LDS reads done) before the next tile's first DMA lands
  }
}

// X[M x 128] := X * W^T (W = inverse of the diagonal block, lower triangular), in place: a workgroup
// owns a full 128-row strip, and every load of it precedes the epilogue stores.
template <bool SSQ>
__global__ __launch_bounds__(256, 2) void trsm_panel_kernel(double* X, int64_t ldx, const double* winv, double* ssq) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* Xs = X + (int64_t)blockIdx.x * 128;
  gemm_tile_128<true, false, false, SSQ>(Xs, ldx, Xs, ldx, winv, 128, 128, smem, 0, 0, 0, SSQ ? ssq + (int64_t)blockIdx.x * 128 : nullptr);
}

// Trailing update over the packed layout: for every target panel q in {q_begin, q_begin+stride, ..}
// C_q -= L_p[rows of q] * L_p[rows of q's diagonal block]^T, lower tiles only.
__global__ __launch_bounds__(256, 2) void trailing_kernel(double* packed, int64_t n_pad, int p, int q_begin, int q_stride,
                                                          int n_targets, int ntiles) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int P = (int)(n_pad / NB);
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {  // as gemm_nt_kernel
    int id = (int)xcd_remap((unsigned)t, (unsigned)ntiles);
    int q, tr, tc;
    if (!target_tile(id, P, q_begin, q_stride, n_targets, q)) continue;
    panel_tile(id, tr, tc);
    const int64_t ldp = panel_ld(n_pad, p), ldq = panel_ld(n_pad, q);
    const double* Lp = packed + panel_offset(n_pad, p) + (int64_t)(q - p) * NB;  // row q*NB of panel p
    double* Cq = packed + panel_offset(n_pad, q);
    gemm_tile_128<false>(Cq + (int64_t)tr * 128 + (int64_t)tc * 128 * ldq, ldq, Lp + (int64_t)tr * 128, ldp,
                         Lp + (int64_t)tc * 128, ldp, NB, smem);
    __syncthreads();
  }
}


// Left-looking step of the predict solve: the columns of panels [j, j + G) of vt receive, in ONE pass with the C tile
// held in the accumulators, everything the right-looking form would have subtracted panel by panel:
//   vt[:, j NB : (j+G) NB] -= vt[:, 0 : j NB] * L[j NB : (j+G) NB, 0 : j NB]^T          (K = j NB).
// Same products in the same order (k ascending from the loaded C value), so the result is bit-identical; what
// changes is that a C tile is loaded and stored once instead of j times -- the per-tile prologue (C preload + first
// DMA, ~7 % of a K = 512 tile during which the tile's waves issue no MFMA) is paid once per j NB of K.
// tri_row0 >= 0 (fit()'s gradient: the rows of vt are rows tri_row0, tri_row0 + 1, ... of the IDENTITY, so row i is zero left of
// column tri_row0 + i and stays zero there): a tile's pass starts at its first row's column instead of column 0 -- the skipped
// products are exact zeros, so the bits are those of the full pass -- and a tile whose rows start right of the pass has nothing to do.
__global__ __launch_bounds__(256, 2) void solve_left_kernel(double* vt, int64_t ldv, const double* packed, int64_t n_pad, int j,
                                                            int tiles_m, int tiles_n, int group, int64_t tri_row0) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const unsigned ntiles = (unsigned)tiles_m * (unsigned)tiles_n;
  // (the triangular form keeps block id -> tile: a tile's length falls with its row, and XCD-contiguous id ranges would hand one XCD
  //  all the long tiles and another none -- measured 27 TFLOP/s; round-robin over the XCDs every one gets the same mix)
  const unsigned id = tri_row0 >= 0 ? blockIdx.x : xcd_remap(blockIdx.x, ntiles);
  int tr, tc;
  group_tile(id, tiles_m, tiles_n, group, tr, tc);
  const int64_t col = (int64_t)j * NB + (int64_t)tc * 128;
  int kt_first = 0;
  const int kt_end = j * (NB / 16);
  if (tri_row0 >= 0) {
    const int64_t first_col = tri_row0 + (int64_t)tr * 128;      // a multiple of 128: whole k-tiles
    if (first_col / 16 > kt_first) kt_first = (int)(first_col / 16);
    if (kt_first >= kt_end) return;
  }
  gemm_tile_128<false, true>(vt + (int64_t)tr * 128 + col * ldv, ldv, vt + (int64_t)tr * 128 + (int64_t)kt_first * 16 * ldv, ldv, packed, n_pad,
                             (kt_end - kt_first) * 16, smem, col, 0, kt_first);
}


// The predict's in-panel solve in ONE launch: panel p of vt := vt L^-T once everything left of the panel has been applied.
// Per 128-row strip of vt the four 128-column sub-steps are C(.,j) -= vt(., panel columns < j) L(j, < j)^T  (K = 128 j), then
// C(.,j) := C(.,j) Winv_j^T [+ the per-row sums of squares of the finished block].  L and Winv are final, so strips are
// independent: what used to be seven dependent launches per panel (each draining the GPU, each latency-bound for the 64-tile
// slices of an 8-rank run) is one workgroup per strip running its seven tiles back to back.  The same gemm_tile_128 calls in the
// same order per strip: bit-identical.
template <bool SSQ>
__global__ __launch_bounds__(256, 2) void solve_panel_fused_kernel(double* vt, int64_t ldv, const double* packed, int64_t n_pad, int p,
                                                                   const double* winv, double* sspart, int64_t m_pad) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int64_t ld = panel_ld(n_pad, p);
  const double* pan = packed + panel_offset(n_pad, p);
  double* strip = vt + (int64_t)blockIdx.x * 128 + (int64_t)p * NB * ldv;   // my 128 rows, first column of the panel
  for (int j = 0; j < TPP; ++j) {
    double* C = strip + (int64_t)j * NBI * ldv;
    if (j > 0) {
      gemm_tile_128<false>(C, ldv, strip, ldv, pan + (int64_t)j * NBI, ld, j * NBI, smem);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the updated block is re-read (LDS-DMA) by all four waves
      __syncthreads();
    }
    const double* wblk = winv + ((int64_t)p * TPP + j) * NBI * NBI;
    double* ssq = SSQ ? sspart + ((int64_t)p * TPP + j) * m_pad + (int64_t)blockIdx.x * 128 : nullptr;
    gemm_tile_128<true, false, false, SSQ>(C, ldv, C, ldv, wblk, 128, 128, smem, 0, 0, 0, ssq);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // block j is an operand of the next sub-step's update
    __syncthreads();
  }
}

// Trailing update by a RANGE of source panels [p_begin, p_end) in one pass: every lower tile of the target panels
// q_begin, q_begin + q_stride, ... (n_targets of them) receives
//   A[R.., C..] -= L[R.., p_begin NB : p_end NB] * L[C.., p_begin NB : p_end NB]^T,
// both operand strips walking through the packed panels.  Same products, same order as the single-panel passes
// p = p_begin .. p_end - 1 (k ascending from the loaded C value): bit-identical, one C load/store and one tile prologue
// instead of p_end - p_begin.  p_begin = 0 is the left-looking sweep of one GPU; the multi-rank driver uses it to apply
// the panels it has received in batches.
__global__ __launch_bounds__(256, 2) void trailing_range_kernel(double* packed, int64_t n_pad, int p_begin, int p_end, int q_begin,
                                                                int q_stride, int n_targets, int ntiles) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int P = (int)(n_pad / NB);
  int id = (int)xcd_remap(blockIdx.x, (unsigned)ntiles);
  int q, tr, tc;
  if (!target_tile(id, P, q_begin, q_stride, n_targets, q)) return;
  panel_tile(id, tr, tc);
  const int64_t ldq = panel_ld(n_pad, q);
  double* Cq = packed + panel_offset(n_pad, q);
  const int64_t row = (int64_t)q * NB + (int64_t)tr * 128, col = (int64_t)q * NB + (int64_t)tc * 128;
  gemm_tile_128<false, true, true>(Cq + (int64_t)tr * 128 + (int64_t)tc * 128 * ldq, ldq, packed, n_pad, packed, n_pad,
                                   (p_end - p_begin) * NB, smem, col, row, p_begin * (NB / 16));
}

}  // namespace

int launch_solve_left(hipStream_t s, double* vt, int64_t ldv, int64_t m_pad, const double* packed, int64_t n_pad, int64_t j, int64_t G,
                      int64_t tri_row0) {
  if (j <= 0 || m_pad <= 0 || G <= 0) return 0;
  if (m_pad % 128) { set_error("solve_left: m_pad must be a multiple of 128"); return GPRC_ERR_ARG; }
  if ((j + G) * NB > n_pad) { set_error("solve_left: panel group beyond the factor"); return GPRC_ERR_ARG; }
  GPRC_TRY(ensure_dynamic_lds<solve_left_kernel>(G_SMEM_BYTES));
  const int64_t N = G * NB, tiles = (m_pad / 128) * (N / 128), K = j * NB;
  double fl = 2.0 * (double)m_pad * N * (double)K;
  if (tri_row0 >= 0) {   // algorithmic work of the triangular form: per 128-row tile only the columns from its first row on
    fl = 0.0;
    for (int64_t tr = 0; tr < m_pad / 128; ++tr) fl += 2.0 * 128.0 * N * (double)std::max<int64_t>(0, K - std::max<int64_t>(0, tri_row0 + tr * 128));
  }
  ProfScope ps(s, PK_SOLVE_LEFT, fl, 8.0 * (2.0 * m_pad * N + (double)m_pad * K + (double)N * K));
  hipLaunchKernelGGL(solve_left_kernel, dim3((unsigned)tiles), dim3(256), G_SMEM_BYTES, s, vt, ldv, packed, n_pad,
                     (int)j, (int)(m_pad / 128), (int)(N / 128), 8, tri_row0);
  GPRC_LAUNCH_CHECK();
  return 0;
}

// ssq != nullptr: also ssq[i] = sum_j X_new[i][j]^2 for the M rows (the predict's fused colSums(v * v) partial of this block column)
// vt[:, panel p] := vt[:, panel p] L_pp^-T (in place; everything left of panel p already applied); sspart (may be null):
// per-row sums of squares of the four finished 128-column blocks at sspart[(4 p + j) * m_pad + row]
int launch_solve_panel_fused(hipStream_t s, double* vt, int64_t ldv, int64_t m_pad, const double* packed, int64_t n_pad, int64_t p,
                             const double* winv, double* sspart, int64_t ss_stride) {
  if (m_pad <= 0) return 0;
  if (ss_stride <= 0) ss_stride = m_pad;
  if (m_pad % 128) { set_error("solve_panel_fused: m_pad must be a multiple of 128"); return GPRC_ERR_ARG; }
  GPRC_TRY(sspart ? ensure_dynamic_lds<solve_panel_fused_kernel<true>>(G_SMEM_BYTES) : ensure_dynamic_lds<solve_panel_fused_kernel<false>>(G_SMEM_BYTES));
  const double M = (double)m_pad;
  ProfScope ps(s, PK_SOLVE_PANEL, M * 128.0 * 128.0 * TPP + 2.0 * M * 128.0 * 128.0 * (TPP * (TPP - 1) / 2), 8.0 * 2.0 * M * NB);
  if (sspart) hipLaunchKernelGGL(solve_panel_fused_kernel<true>, dim3((unsigned)(m_pad / 128)), dim3(256), G_SMEM_BYTES, s, vt, ldv, packed, n_pad, (int)p, winv, sspart, ss_stride);
  else hipLaunchKernelGGL(solve_panel_fused_kernel<false>, dim3((unsigned)(m_pad / 128)), dim3(256), G_SMEM_BYTES, s, vt, ldv, packed, n_pad, (int)p, winv, sspart, ss_stride);
  GPRC_LAUNCH_CHECK();
  return 0;
}

int launch_trsm_panel(hipStream_t s, double* X, int64_t ldx, int64_t M, const double* winv, double* ssq) {
  if (M <= 0) return 0;
  if (M % 128) { set_error("trsm_panel: M must be a multiple of 128"); return GPRC_ERR_ARG; }
  GPRC_TRY(ssq ? ensure_dynamic_lds<trsm_panel_kernel<true>>(G_SMEM_BYTES) : ensure_dynamic_lds<trsm_panel_kernel<false>>(G_SMEM_BYTES));
  ProfScope ps(s, PK_TRSM_PANEL, 1.0 * M * 128 * 128, 8.0 * 2 * M * 128);
  if (ssq) hipLaunchKernelGGL(trsm_panel_kernel<true>, dim3((unsigned)(M / 128)), dim3(256), G_SMEM_BYTES, s, X, ldx, winv, ssq);
  else hipLaunchKernelGGL(trsm_panel_kernel<false>, dim3((unsigned)(M / 128)), dim3(256), G_SMEM_BYTES, s, X, ldx, winv, ssq);
  GPRC_LAUNCH_CHECK();
  return 0;
}

int launch_gemm_nt(hipStream_t s, double* C, int64_t ldc, const double* A, int64_t lda, const double* B, int64_t ldb,
                   int64_t M, int64_t N, int64_t K, int lower, int kind) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  // (K: the tile loop runs two k-tiles of 16 per iteration and needs at least four: every caller's K is a multiple of 128)
  if (M % 128 || N % 128 || K % (2 * G_KB) || K < 4 * G_KB || (lda & 1) || (ldb & 1)) { set_error("gemm_nt: bad shape"); return GPRC_ERR_ARG; }
  const int64_t tiles = (M / 128) * (N / 128);
  if (tiles > 0x7fffffff) { set_error("gemm_nt: too many tiles"); return GPRC_ERR_ARG; }
  if (kind == PK_INV_GEMM && !(lower && M == N && K == M)) { set_error("gemm_nt: the triangular inverse product is square and lower"); return GPRC_ERR_ARG; }
  const double useful = kind == PK_INV_GEMM ? 1.0 / 6.0 : lower ? 0.5 : 1.0;  // algorithmic: the lower triangle only (inverse product: from the diagonal on)
  ProfScope ps(s, kind, 2.0 * M * N * K * useful, 8.0 * (2.0 * M * N * (lower ? 0.5 : 1.0) + (M + N) * (double)K));
  const int tm = (int)(M / 128), tn = (int)(N / 128);
  constexpr int group = 8;  // 8 x 8 concurrent tiles per XCD share 16 strips; 4..32 measured within 0.5 %
  auto launch = [&](auto role) -> int {   // one tile per workgroup
    constexpr int ROLE = decltype(role)::value;
    GPRC_TRY(ensure_dynamic_lds<gemm_nt_kernel<ROLE>>(G_SMEM_BYTES));
    hipLaunchKernelGGL((gemm_nt_kernel<ROLE>), dim3((unsigned)tiles), dim3(256), G_SMEM_BYTES, s, C, ldc, A, lda, B, ldb, tm, tn, (int)K, lower, group);
    GPRC_LAUNCH_CHECK();
    return 0;
  };
  if (kind == PK_SOLVE_UPDATE) return launch(std::integral_constant<int, PK_SOLVE_UPDATE>{});
  if (kind == PK_COV_SYRK) return launch(std::integral_constant<int, PK_COV_SYRK>{});
  if (kind == PK_INV_GEMM) return launch(std::integral_constant<int, PK_INV_GEMM>{});
  return launch(std::integral_constant<int, PK_GEMM_INNER>{});
}

// target panels q_begin, q_begin + q_stride, ... < q_end updated with the factored panel p (K = NB)
int launch_trailing_update(hipStream_t s, double* packed, int64_t n_pad, int64_t p, int64_t q_begin, int64_t q_end,
                           int64_t q_stride) {
  const int64_t P = n_pad / NB;
  if (q_begin <= p || q_stride <= 0) { set_error("trailing_update: bad panel range"); return GPRC_ERR_ARG; }
  if (q_end > P) q_end = P;
  int64_t tiles = 0, nt = 0;
  for (int64_t q = q_begin; q < q_end; q += q_stride) { tiles += panel_tiles(P, q); ++nt; }
  if (tiles <= 0) return 0;
  GPRC_TRY(ensure_dynamic_lds<trailing_kernel>(G_SMEM_BYTES));
  double fl = 0.0, by = 0.0;
  trailing_work(n_pad, q_begin, q_end, q_stride, NB, false, fl, by);
  ProfScope ps(s, PK_TRAILING, fl, by);
  hipLaunchKernelGGL(trailing_kernel, dim3((unsigned)tiles), dim3(256), G_SMEM_BYTES, s, packed, n_pad, (int)p,
                     (int)q_begin, (int)q_stride, (int)nt, (int)tiles);
  GPRC_LAUNCH_CHECK();
  return 0;
}

// target panels q_begin, q_begin + q_stride, ... < q_end updated with the source panels [p_begin, p_end) in one pass
int launch_trailing_range(hipStream_t s, double* packed, int64_t n_pad, int64_t p_begin, int64_t p_end, int64_t q_begin, int64_t q_end,
                          int64_t q_stride) {
  const int64_t P = n_pad / NB;
  if (q_end > P) q_end = P;
  if (p_begin < 0 || p_end <= p_begin || q_stride <= 0) return 0;
  if (q_begin < p_end) { set_error("trailing_range: a target panel is not behind the source range"); return GPRC_ERR_ARG; }
  if (q_begin >= q_end) return 0;
  GPRC_TRY(ensure_dynamic_lds<trailing_range_kernel>(G_SMEM_BYTES));
  int64_t tiles = 0, nt = 0;
  for (int64_t q = q_begin; q < q_end; q += q_stride) { tiles += panel_tiles(P, q); ++nt; }
  double fl = 0.0, by = 0.0;
  trailing_work(n_pad, q_begin, q_end, q_stride, (double)(p_end - p_begin) * NB, false, fl, by);
  ProfScope ps(s, PK_TRAILING_LEFT, fl, by);
  hipLaunchKernelGGL(trailing_range_kernel, dim3((unsigned)tiles), dim3(256), G_SMEM_BYTES, s, packed, n_pad,
                     (int)p_begin, (int)p_end, (int)q_begin, (int)q_stride, (int)nt, (int)tiles);
  GPRC_LAUNCH_CHECK();
  return 0;
}

}  // namespace gprc
