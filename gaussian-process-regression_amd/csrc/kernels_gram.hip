// kernels_gram.hip -- the two reductions over the ROWS of a solved chunk that the sparse GPR's fit adds (gprc_sparse.hip; DESIGN.md
// section 7, "Sparse GPR"), and the elementwise pass that turns the accumulated Gram matrix into B:
//   gram_rows_kernel    packed(lower) += V^T V for a chunk V (rows x n_pad, column-major: one row per training point), straight into
//                       the packed block-column layout, 128 x 128 tiles on v_mfma_f64_16x16x4_f64
//   col_reduce_kernel   out[j] += sum_i V[i, j] w[i]
//   gram_to_b_kernel    packed := I + packed / sigma^2
// Both reductions run over the chunk's rows, the contiguous direction of BOTH MFMA operands, which gemm_tile_128 (A B^T of column-major
// strips, k along the leading dimension) cannot read.  Both are chunk-invariant bit for bit: an output element is the stored value plus
// its rows' terms in ascending row order, in groups whose boundaries are multiples of 256 rows from the first row of the first chunk,
// and no workgroup splits the rows -- so one call with r1 + r2 rows is two calls with r1 and r2 rows.
#include "chol_tile.h"   // double4_t, lptr_t

namespace gprc {

typedef double double2_t __attribute__((ext_vector_type(2)));

namespace {

// ------------------------------------------------------------------------------------------------
// The LDS image of one operand and k-tile: [128 columns of V][GR_KB rows of V + 2 pad] doubles, a column's GR_KB consecutive rows
// contiguous, as they are in memory.  Both MFMA operands of a 16x16x4 step are "16 columns of V x 4 rows of V" with the lane holding
// (column fr = lane & 15, row fk = lane >> 4), so ONE image format serves both roles (and on a diagonal tile one image IS both).
// Bank arithmetic of the operand read (ds_read_b64: two groups of 32 lanes, bank = dword address mod 64): a lane reads the double at
// (c0 + fr) GR_LD + 4 kk + fk, i.e. dword 36 fr + 2 fk + const at GR_LD = 18.  36 fr mod 64 runs over the sixteen multiples of 4
// (36 = 4 x 9, 9 odd), fk in {0, 1} (or {2, 3}) within a 32-lane group adds 0 or 2, the double covers two dwords: the 32 lanes cover
// the 64 banks exactly once.  The staging store is one ds_write_b128 per lane, eight consecutive lanes writing one column's 128
// contiguous bytes = the 32 banks of a store's 8-lane group once.
// ------------------------------------------------------------------------------------------------
constexpr int GR_KB = 16;                       // rows of V per k-tile: 128 contiguous bytes of every column
constexpr int GR_LD = GR_KB + 2;
constexpr int GR_IMG = 128 * GR_LD;             // doubles per operand image
constexpr size_t GR_SMEM_BYTES = 4 * GR_IMG * sizeof(double);   // two operands x two buffers = 73,728 B: two workgroups per CU

// lower tile `id` (row-major over the lower triangle of T x T tiles) -> (tr, tc), tc <= tr
__device__ __forceinline__ void lower_tile(unsigned id, int& tr, int& tc) {
  int r = (int)((sqrt(8.0 * (double)id + 1.0) - 1.0) * 0.5);
  while ((unsigned)(r + 1) * (unsigned)(r + 2) / 2 <= id) ++r;
  while ((unsigned)r * (unsigned)(r + 1) / 2 > id) --r;
  tr = r;
  tc = (int)(id - (unsigned)r * (unsigned)(r + 1) / 2);
}

// One 128 x 128 tile (tr, tc) of the lower triangle per workgroup: C[a, b] += sum_i V[i, 128 tr + a] V[i, 128 tc + b], i ascending,
// four rows per MFMA, the accumulators starting from the stored tile (as gemm_tile_128<SET = false> starts from C).  Four waves, a
// 64 x 64 quadrant each, accumulator layout C[row = 16 m + (lane & 15)][col = 16 n + (lane >> 4) + 4 r] as gemm_tile_128's (sixteen
// consecutive rows of the column-major tile per lane group).  Staging is through registers (global_load_dwordx4 -> ds_write_b128: the
// padded column pitch cannot be written by an LDS-DMA instruction, whose 64 lanes land contiguously), one k-tile ahead: the loads of
// tile kt + 1 are issued before the MFMAs of tile kt and stored to the other buffer after them; one barrier per k-tile.
// The grid is the lower triangle of tiles, row by row.
__global__ __launch_bounds__(256, 2) void gram_rows_kernel(const double* __restrict__ vt, int64_t ld, int rows, double* packed, int64_t n_pad) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  int tr, tc;
  lower_tile(blockIdx.x, tr, tc);
  const bool diag = tr == tc;                   // workgroup-uniform
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  const int fk = lane >> 4, fr = lane & 15;

  const int64_t q = tc / TPP;                   // the panel that holds the tile's columns
  const int64_t ldc = panel_ld(n_pad, q);
  double* C = packed + panel_offset(n_pad, q) + ((int64_t)tr * 128 - q * NB) + (int64_t)(tc % TPP) * 128 * ldc;
  double* Cw = C + (wr * 64 + fr) + (int64_t)(wc * 64 + fk) * ldc;
  double4_t acc[4][4];
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int m = 0; m < 4; ++m) acc[m][n][r] = Cw[m * 16 + (int64_t)(n * 16 + 4 * r) * ldc];

  // staging: eight lanes per column of V (two rows each), 32 columns per pass, four passes per operand
  const int sc = t >> 3, sk = (t & 7) * 2;
  const double* ga = vt + ((int64_t)tr * 128 + sc) * ld + sk;     // the columns of V that are the tile's ROWS
  const double* gb = vt + ((int64_t)tc * 128 + sc) * ld + sk;     // ... its COLUMNS (not read on a diagonal tile)
  const int soff = sc * GR_LD + sk;
  double2_t ra[4], rb[4];
  auto gload = [&](int k0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) ra[j] = *reinterpret_cast<const double2_t*>(ga + (int64_t)(32 * j) * ld + k0);
    if (!diag) {
#pragma unroll
      for (int j = 0; j < 4; ++j) rb[j] = *reinterpret_cast<const double2_t*>(gb + (int64_t)(32 * j) * ld + k0);
    }
  };
  auto sstore = [&](double* buf) {
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<double2_t*>(buf + soff + 32 * j * GR_LD) = ra[j];
    if (!diag) {
#pragma unroll
      for (int j = 0; j < 4; ++j) *reinterpret_cast<double2_t*>(buf + GR_IMG + soff + 32 * j * GR_LD) = rb[j];
    }
  };

#define GR_SB __builtin_amdgcn_sched_barrier(0);
#define GR_RD(dst, base, m, kk) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(dst) : "v"(base), "n"(((m) * 16 * GR_LD + (kk) * 4) * 8));
#define GR_READ(A_, B_, kk) GR_RD(A_[0], aB, 0, kk) GR_RD(A_[1], aB, 1, kk) GR_RD(A_[2], aB, 2, kk) GR_RD(A_[3], aB, 3, kk) \
                            GR_RD(B_[0], bB, 0, kk) GR_RD(B_[1], bB, 1, kk) GR_RD(B_[2], bB, 2, kk) GR_RD(B_[3], bB, 3, kk) GR_SB
#define GR_READY(A_, B_) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(A_[0]), "+v"(A_[1]), "+v"(A_[2]), "+v"(A_[3]), "+v"(B_[0]), "+v"(B_[1]), "+v"(B_[2]), "+v"(B_[3])); GR_SB
#define GR_MMA(A_, B_)                                                                                                  \
  _Pragma("unroll") for (int m = 0; m < 4; ++m)                                                                         \
    _Pragma("unroll") for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(B_[n], A_[m], acc[m][n], 0, 0, 0); \
  GR_SB
  double a0[4], b0[4], a1[4], b1[4];
  const int nkt = rows / GR_KB;
  gload(0);
  sstore(smem);
  // vmcnt(0) through the BUILTIN (0x0F70), as in gemm_tile_128: the compiler's waitcnt pass then knows the C-tile loads have completed
  // and does not wait for the NEXT tile's staging loads in the middle of a tile's MFMAs
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __syncthreads();
  const int aoff = (wr * 64 + fr) * GR_LD + fk;
  const int boff = (diag ? 0 : GR_IMG) + (wc * 64 + fr) * GR_LD + fk;
  // one k-tile's 64 MFMAs from the images at `cur`.  Operand reads as single ds_read_b64 in inline assembly (the image is padded for
  // THAT instruction's banking; the compiler merges plain loads of two k-steps into ds_read2_b64, which has another bank rule and costs
  // eight times the LDS cycles), one k-step ahead of the MFMAs that use them, the waits counted by hand as in gemm_tile_128: everything
  // in flight at a GR_READY is reads.
  auto mma_tile = [&](double* cur) __attribute__((always_inline)) {
    const unsigned aB = (unsigned)(uintptr_t)(lptr_t)(cur + aoff), bB = (unsigned)(uintptr_t)(lptr_t)(cur + boff);
    GR_READ(a0, b0, 0)
    GR_READY(a0, b0) GR_READ(a1, b1, 1) GR_MMA(a0, b0)
    GR_READY(a1, b1) GR_READ(a0, b0, 2) GR_MMA(a1, b1)
    GR_READY(a0, b0) GR_READ(a1, b1, 3) GR_MMA(a0, b0)
    GR_READY(a1, b1) GR_MMA(a1, b1)
  };
  // (the last tile is peeled: no condition on "a next tile exists" inside the loop, so the compiler's wait-count analysis is exact and
  //  the staging loads are waited for only in front of their ds_write)
  int kt = 0;
  for (; kt + 1 < nkt; ++kt) {
    gload((kt + 1) * GR_KB);
    mma_tile(smem + (kt & 1) * 2 * GR_IMG);
    sstore(smem + ((kt + 1) & 1) * 2 * GR_IMG);   // the other buffer: its last readers passed the barrier that ended tile kt - 1
    __syncthreads();
  }
  mma_tile(smem + (kt & 1) * 2 * GR_IMG);
#undef GR_MMA
#undef GR_READY
#undef GR_READ
#undef GR_RD
#undef GR_SB
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int m = 0; m < 4; ++m) Cw[m * 16 + (int64_t)(n * 16 + 4 * r) * ldc] = acc[m][n][r];
}

// out[j] += sum_i vt[i, j] w[i]: a wave per column.  Per block of 256 rows a lane multiplies its four consecutive rows in order (fma
// chain), the 64 lanes are added by a butterfly (xor 1, 2, ..., 32: one fixed tree), and the blocks are added to the running sum, which
// starts from out[j], in ascending order.
__global__ __launch_bounds__(256) void col_reduce_kernel(const double* __restrict__ vt, int64_t ld, int64_t rows, int64_t cols,
                                                         const double* __restrict__ w, double* out) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= cols) return;                        // wave-uniform
  const double* col = vt + j * ld + 4 * lane;
  const double* wl = w + 4 * lane;
  double acc = out[j];
  for (int64_t r0 = 0; r0 < rows; r0 += 256) {
    const double2_t v0 = *reinterpret_cast<const double2_t*>(col + r0), v1 = *reinterpret_cast<const double2_t*>(col + r0 + 2);
    const double2_t w0 = *reinterpret_cast<const double2_t*>(wl + r0), w1 = *reinterpret_cast<const double2_t*>(wl + r0 + 2);
    double s = v0[0] * w0[0];
    s = fma(v0[1], w0[1], s);
    s = fma(v1[0], w1[0], s);
    s = fma(v1[1], w1[1], s);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) s += __shfl_xor(s, off, 64);
    acc += s;
  }
  if (lane == 0) out[j] = acc;
}

// packed := I + packed / sigma^2 over every stored element (the unused upper tiles of the diagonal blocks included: they hold zeros)
__global__ __launch_bounds__(256) void gram_to_b_kernel(double* pan, int64_t ldp, int64_t count, double sigma2) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  const int64_t r = e % ldp, c = e / ldp;       // local row and column of the panel: the diagonal is r == c
  pan[e] = pan[e] / sigma2 + (r == c ? 1.0 : 0.0);
}

__global__ __launch_bounds__(256) void div_vec_kernel(double* x, int64_t n, double f) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] /= f;
}

}  // namespace

int launch_gram_rows(hipStream_t s, const double* vt, int64_t ld, int64_t rows, int64_t n_pad, double* packed) {
  if (rows <= 0) return 0;
  if (!vt || !packed || n_pad <= 0 || n_pad % NB || rows % 256 || ld < rows || (ld & 1) || rows > 0x7fffff00 ||
      ((reinterpret_cast<uintptr_t>(vt) | reinterpret_cast<uintptr_t>(packed)) & 15)) {
    set_error("gram_rows: rows must be a multiple of 256, n_pad a multiple of the panel width, ld even and >= rows, the buffers 16-byte aligned");
    return GPRC_ERR_ARG;
  }
  const int64_t T = n_pad / 128, tiles = T * (T + 1) / 2;
  if (tiles > 0x7fffffff) { set_error("gram_rows: too many tiles"); return GPRC_ERR_ARG; }
  GPRC_TRY(ensure_dynamic_lds<gram_rows_kernel>(GR_SMEM_BYTES));
  ProfScope ps(s, PK_COV_SYRK, (double)rows * n_pad * (double)(n_pad + 128), 8.0 * (2.0 * 128.0 * 128.0 * tiles + (double)rows * n_pad));
  hipLaunchKernelGGL(gram_rows_kernel, dim3((unsigned)tiles), dim3(256), GR_SMEM_BYTES, s, vt, ld, (int)rows, packed, n_pad);
  GPRC_LAUNCH_CHECK();
  return 0;
}

int launch_col_reduce(hipStream_t s, const double* vt, int64_t ld, int64_t rows, int64_t cols, const double* w, double* out) {
  if (rows <= 0 || cols <= 0) return 0;
  if (!vt || !w || !out || rows % 256 || ld < rows || (ld & 1) || ((reinterpret_cast<uintptr_t>(vt) | reinterpret_cast<uintptr_t>(w)) & 15)) {
    set_error("col_reduce: rows must be a multiple of 256, ld even and >= rows, vt and w 16-byte aligned");
    return GPRC_ERR_ARG;
  }
  ProfScope ps(s, PK_ROWREDUCE, 2.0 * rows * cols, 8.0 * rows * cols);
  hipLaunchKernelGGL(col_reduce_kernel, dim3((unsigned)((cols + 3) / 4)), dim3(256), 0, s, vt, ld, rows, cols, w, out);
  GPRC_LAUNCH_CHECK();
  return 0;
}

int launch_gram_to_b(hipStream_t s, double* packed, int64_t n_pad, double sigma2) {
  for (int64_t p = 0; p < n_pad / NB; ++p) {
    const int64_t ldp = panel_ld(n_pad, p), count = ldp * NB;
    hipLaunchKernelGGL(gram_to_b_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, packed + panel_offset(n_pad, p), ldp, count, sigma2);
  }
  GPRC_LAUNCH_CHECK();
  return 0;
}

int launch_div_vec(hipStream_t s, double* x, int64_t n, double f) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(div_vec_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n, f);
  GPRC_LAUNCH_CHECK();
  return 0;
}

}  // namespace gprc
