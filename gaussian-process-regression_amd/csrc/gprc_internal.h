// gprc_internal.h -- shared declarations of the gfx950 implementation behind include/gprc_native.h.
// Host-side launchers live next to their kernels; the host layer only composes them, one unit per job.  What the units share is
// gprc_host.h: the base of every handle that lives on a context with its liveness check and its free (Bound, ctx_gone, free_bound), device
// memory that knows whether its owner is alive (DevMem), the staging types (In, Out, IntOut, finish_sync) and bad(who, msg).
//   gprc_ctx.hip    errors, the event profiler, context lifetime and the registry of live contexts, the block pool, workspace slots,
//                   DevMem's allocation, and the entry points that are only staging around one launcher (kernel matrices, class
//                   probabilities, combine_all)
//   gprc_sched.hip  the factor and solve schedules, chunk workspaces, every schedule knob of the host layer; the layout helpers and
//                   the gprc_dev_* building blocks
//   gprc_model.hip  the model pipelines (GPR, extend, GPC, gradients, predict, MVN, eigen) and their entry points
//   gprc_sparse.hip the sparse GPR with inducing points (fit pass, collapsed bound and its gradient, predict) and its entry points
//   gprc_paths.hip  posterior sample paths by pathwise conditioning (the gprc_paths object, create, eval and eval_grad) and their entry points
//   gprc_iter.hip   the iterative exact GPR (pivoted-Cholesky preconditioner, batched conjugate gradients, fit / solve / predict, and
//                   the stochastic log evidence with its gradient)
//   gprc_batch.hip  small GPs in batches: the batched evidence and gradient, the fitted batch (gprc_batch_model) and its predict; the
//                   classifier batch (the Laplace mode search of kernels_batch_gpc.hip) on the same object and the same predict launch
//   gprc_local.hip  the local GPR: device nearest-neighbour search (one front for both searches), then one batched small model per test
//                   point (on gprc_batch's entry points); the Vecchia likelihood on the same object; the local classifier likewise
//   gprc_mgpu.hip   the multi-GPU layer, on the public ABI only
// Device cores shared between kernel files are headers: chol_tile.h (the Cholesky side: kernels_gemm.hip, kernels_chol.hip),
// small_model.h (built on the other two: what the kernels that run one model of at most 128 points per workgroup share) and
// pair_tile.h (the covariance side: the 128 x 64 pairwise tile of kernels_fill.hip, kernels_grad.hip, kernels_pgrad.hip and
// kernels_sgrad.hip, the kernel-id dispatcher and the set of kernels with an exact gradient; kernels_paths.hip takes the tile
// extents, the staging, the dispatcher and, for its gradient product, pair_weight from it and has its own lane layout, the MFMA
// operand's).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <string>

#include "../../include/gprc_native.h"

namespace gprc {

// ---- geometry (DESIGN.md "Data layout") -------------------------------------------------------
#ifndef GPRC_NB
#define GPRC_NB 512
#endif
constexpr int NB = GPRC_NB;  // outer panel width: K-depth of the trailing update (NB/8 flop per byte of C traffic)
constexpr int NBI = 128;  // inner block: one LDS-resident diagonal factorisation, one GEMM tile edge
constexpr int TPP = NB / NBI;  // 128-wide tile columns per panel
constexpr int MAX_PARAMS = 256;  // kernel parameters travel as kernel arguments; only linear's per-coordinate sigma needs more than 2
constexpr int MAX_DEVICES = 64;  // per-device one-time setup flags
// GPRC_INFO_WAIT_TIMEOUT (-99, include/gprc_native.h): written to the LAPACK-info word by a fused kernel whose device-side dependency
// wait ran out (never seen in practice: it takes a faulted or never-scheduled producer); hosts turn it into GPRC_ERR_HIP instead of
// using the factor
static_assert(NB % NBI == 0 && NB >= NBI, "panel width must be a multiple of the 128 block");

__host__ __device__ static inline int64_t pad_up(int64_t n, int64_t m) { return (n + m - 1) / m * m; }
__host__ __device__ static inline int64_t panel_offset(int64_t n_pad, int64_t p) { return (int64_t)NB * (p * n_pad - (int64_t)NB * p * (p - 1) / 2); }
__host__ __device__ static inline int64_t panel_ld(int64_t n_pad, int64_t p) { return n_pad - p * NB; }
// lower 128 x 128 tiles of packed panel q of P: TPP x TPP per NB rows, less the upper tiles of the diagonal block
template <typename T>
__host__ __device__ constexpr T panel_tiles(T P, T q) { return TPP * TPP * (P - q) - TPP * (TPP - 1) / 2; }
// The factor service's resident workgroups (kernels_chol.hip, a CU each): SERVICE_CORE_WGS roles on the chain and around it, TPP more
// when it also forms the explicit inverses, CHAIN_HELPERS more with the split chain.
constexpr int SERVICE_CORE_WGS = 3 + TPP + TPP * (TPP + 1) / 2;
constexpr int CHAIN_HELPERS = 4;                  // 32-row slices of a 128-row block

// ---- error plumbing ---------------------------------------------------------------------------
void set_error(const std::string& msg);
int hip_fail(hipError_t e, const char* what, const char* file, int line);

#define GPRC_HIP(call)                                                          \
  do {                                                                          \
    hipError_t e__ = (call);                                                    \
    if (e__ != hipSuccess) return ::gprc::hip_fail(e__, #call, __FILE__, __LINE__); \
  } while (0)
#define GPRC_TRY(call)          \
  do {                          \
    int rc__ = (call);          \
    if (rc__ != 0) return rc__; \
  } while (0)
#define GPRC_LAUNCH_CHECK() GPRC_HIP(hipGetLastError())

// Raises Kernel's dynamic-LDS limit to `bytes` (its one launch configuration) once per device: the attribute is per device, one process
// may hold contexts on several, and several host threads may launch at once (a second thread that also sets it does no harm).
template <auto Kernel>
int ensure_dynamic_lds(size_t bytes) {
  static std::atomic<bool> set[MAX_DEVICES];
  int dev = 0;
  GPRC_HIP(hipGetDevice(&dev));
  const bool known = dev >= 0 && dev < MAX_DEVICES;
  if (known && set[dev].load(std::memory_order_acquire)) return 0;
  GPRC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  if (known) set[dev].store(true, std::memory_order_release);
  return 0;
}
// one launch of a kernel that needs the raised limit: the limit, the launch, the launch's error (which names `who`, the caller's kernel)
template <auto Kernel, class... Args>
int launch_with_lds(const char* who, dim3 grid, dim3 block, size_t bytes, hipStream_t s, const Args&... args) {
  GPRC_TRY(ensure_dynamic_lds<Kernel>(bytes));
  hipLaunchKernelGGL(Kernel, grid, block, bytes, s, args...);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : hip_fail(e, who, __FILE__, __LINE__);
}

// ---- in-library event profiler (bench.py's live roofline numbers) ---------------------------------
enum ProfKind { PK_FILL = 0, PK_POTF2 = 1, PK_TRSM_PANEL = 2, PK_GEMM_INNER = 3, PK_TRAILING = 4, PK_SOLVE_UPDATE = 5,
                PK_TRSV = 6, PK_ROWREDUCE = 7, PK_COV_SYRK = 8, PK_DERIV = 9, PK_JACOBI = 10, PK_SOLVE_LEFT = 11, PK_TRAILING_LEFT = 12, PK_PANEL_FUSED = 13, PK_SOLVE_PANEL = 14, PK_INV_GEMM = 15, PK_GRAD_CONTRACT = 16, PK_GPC_GRAD_CONTRACT = 17,
                PK_REVERSE_FACTOR = 18, PK_PRED_GRAD = 19, PK_COUNT = 20 };
bool prof_enabled();
void prof_begin(hipStream_t s, int kind);
void prof_end(hipStream_t s, int kind, double flops, double bytes);
struct ProfScope {  // brackets one launch (or one launch sequence) with a pair of HIP events when profiling is on
  hipStream_t s; int kind; double flops, bytes; bool on;
  ProfScope(hipStream_t s_, int kind_, double flops_, double bytes_) : s(s_), kind(kind_), flops(flops_), bytes(bytes_), on(prof_enabled()) {
    if (on) prof_begin(s, kind);
  }
  ~ProfScope() { if (on) prof_end(s, kind, flops, bytes); }
};

// algorithmic flops and bytes of a trailing update: the lower triangle of the NB-wide diagonal block + everything below it of the target
// panels q0, q0 + stride, ... < q1, K source columns deep; skip_first_diag: without the first target's diagonal block (the factor service's)
inline void trailing_work(int64_t n_pad, int64_t q0, int64_t q1, int64_t stride, double K, bool skip_first_diag, double& fl, double& by) {
  for (int64_t q = q0; q < q1; q += stride) {
    const double rows = (double)(n_pad - q * NB);
    const double elems = rows * NB - 0.5 * NB * (double)(NB - 1) - (skip_first_diag && q == q0 ? 0.5 * NB * (double)(NB + 1) : 0.0);
    fl += 2.0 * elems * K;
    by += 8.0 * (2.0 * elems + rows * K);
  }
}

struct KernelSpec {
  int id;
  int n_params;
  double p[MAX_PARAMS];
};

// how the out-of-range part of a fill is written
enum PadMode { PAD_NONE = 0,      // exact extents, bounds-checked stores (user-facing covariance_matrix)
               PAD_IDENTITY = 1,  // symmetric K + noise*I, identity outside n (the factor's padding)
               PAD_ZERO = 2 };    // zero outside the valid extents (cross-covariance chunks)

// ---- launchers (kernels_fill.hip) --------------------------------------------------------------
// out[(i-row0) + (j-col0)*ld] = k(A_i, B_j) for i in [row0,row0+nrows), j in [col0,col0+ncols)
int launch_fill(hipStream_t s, const KernelSpec& ks, const double* A, int64_t nA, const double* B, int64_t nB, int64_t d,
                double* out, int64_t ld, int64_t row0, int64_t nrows, int64_t col0, int64_t ncols, PadMode mode,
                double noise);
int launch_colwise(hipStream_t s, const KernelSpec& ks, const double* x, const double* y, int64_t d, int64_t m, double* out);
// predict chunk K(X_star, X) with the fused epilogue: per-column-tile partials of K*^T w and an optional column scale
int64_t fill_mean_tiles(int64_t cols);
int launch_fill_cross_fused(hipStream_t s, const KernelSpec& ks, const double* Xs, int64_t m, const double* X, int64_t n, int64_t d,
                            double* vt, int64_t ld, int64_t m_pad, int64_t n_pad, const double* w, double* mpart, const double* colscale);
int launch_set_identity_rows(hipStream_t s, double* vt, int64_t ld, int64_t rows, int64_t cols, int64_t row0);  // vt[i,j] = (row0+i == j)

// ---- launchers (kernels_grad.hip) --------------------------------------------------------------
// S[r + n*i] = sum_c deriv_i(X[,r], X[,c]; v): row sums of the parameter derivatives of K(X,X) as cov_dict$...$deriv
// (R/fit.R:4-31) defines them; n_deriv (1 or 2) components.  Kernels: sqrexp, gammaexp, polynomial, rationalquadratic.
int launch_deriv_rowsum(hipStream_t s, int kernel, double v0, double v1, const double* X, int64_t d, int64_t n, double* S);
// the exact gradient's contraction: one pass over the stored lower triangle of W = -(K + noise I)^-1 (n_pad x n_pad, ld), K and dK/dtheta
// recomputed from X.  part: grad_partial_rows() x (ks.n_params + 1) doubles, row g = what workgroup g summed over its tiles of
//   sum_ij (alpha_i alpha_j + W_ij) dK_ij / dtheta_k   (ARD: times l_k, the host divides)   and, last, of sum_i (alpha_i^2 + W_ii);
// the caller sums the rows in order and halves.  Kernels: sqrexp, gammaexp, rationalquadratic, sqrexp_ard, matern32, matern52, matern32_ard, matern52_ard.
int64_t grad_partial_rows();
int launch_grad_contract(hipStream_t s, const KernelSpec& ks, const double* X, int64_t d, int64_t n, const double* alpha, const double* W,
                         int64_t ld, double* part);
// the Laplace variant (gprc_gpc_logq_grad): W = -B^-1, B = I + sw K sw; part: grad_partial_rows() x ks.n_params doubles, row g = what
// workgroup g summed of   sum_ij (a_i a_j + sw_i sw_j W_ij + u_i g_j + u_j g_i) dK_ij / dtheta_k   (no diagonal sum: dK_ii = 0)
int launch_gpc_grad_contract(hipStream_t s, const KernelSpec& ks, const double* X, int64_t d, int64_t n, const double* a, const double* sw,
                             const double* u, const double* g, const double* W, int64_t ld, double* part);

// ---- launchers (kernels_pgrad.hip) -------------------------------------------------------------
// the prediction gradient's contraction over one chunk of m test points (rows of the chunk, m_pad = pad_up(m, 128)):
//   pmean[(st d + c) m_pad + i] = sum over the columns j of stripe st of alpha_j h_ij (x*_ic - x_jc) t'_c
//   pvar [(st d + c) m_pad + i] = the same with W[i, n_pad - 1 - j] in place of alpha_j   (W: the chunk (V L^-1) J, column-reversed; ld ldw)
// with k and h recomputed from Xs and X; pvar == nullptr: the mean's sums alone (W is not read); pmean may be null when pvar is not.
// pred_grad_stripes(n_pad) stripes of whole 64-column tiles, a function of n_pad only.  launch_pred_grad_sum adds the stripes in order,
// applies the factors that do not depend on (i, j) (variance: times -2) and writes out[c + d i], i < m.
int64_t pred_grad_stripes(int64_t n_pad);
int launch_pred_grad(hipStream_t s, const KernelSpec& ks, const double* Xs, int64_t m, int64_t m_pad, const double* X, int64_t n, int64_t n_pad,
                     int64_t d, const double* alpha, const double* W, int64_t ldw, double* pmean, double* pvar);
int launch_pred_grad_sum(hipStream_t s, const KernelSpec& ks, const double* part, int64_t n_pad, int64_t d, int64_t m_pad, int64_t m, bool variance,
                         double* out);

// ---- launchers (kernels_paths.hip) -------------------------------------------------------------
// the generated-operand GEMM of the posterior sample paths, one chunk of rows (rows_pad = pad_up(rows, 128)):
//   out[i + s ld] = (accumulate ? out[i + s ld] : 0) + scale * sum_j g(a_i, b_j) B[j + s ldb],   i < rows, s < S, j < cols
// ks == nullptr: g = cospi(2 (sum_c Bp[c, j] a_i[c] + phase[j])), Bp the frequencies in cycles; else g = ks's kernel of the points a_i and
// Bp[, j] (those of with_gradient_kernel).  part: gen_gemm_stripes(cols) x S x rows_pad doubles; the stripes are a function of cols only
// and are added in order, so a row's bits do not depend on the other rows of the call.  Profiled as PK_PRED_GRAD.
int64_t gen_gemm_stripes(int64_t cols);
int launch_gen_gemm(hipStream_t s, const KernelSpec* ks, const double* Bp, const double* phase, int64_t cols, const double* A, int64_t rows,
                    int64_t rows_pad, int64_t d, const double* B, int64_t ldb, int64_t S, double scale, bool accumulate, double* part, double* out,
                    int64_t ld);
// its gradient with respect to the row points, one chunk of rows:
//   dout[i + ld (s + S c)] = (accumulate ? dout[.] : 0) + d / da_i[c] of scale * sum_j g(a_i, b_j) B[j + s ldb],   c < d
// part: gen_gemm_stripes(cols) x d x S x rows_pad doubles.  Same stripes, same order of summation, same independence of a row from the
// other rows; the weight per pair is formed once and serves every coordinate (kernels_paths.hip).  Profiled as PK_PRED_GRAD.
int launch_gen_gemm_grad(hipStream_t s, const KernelSpec* ks, const double* Bp, const double* phase, int64_t cols, const double* A, int64_t rows,
                         int64_t rows_pad, int64_t d, const double* B, int64_t ldb, int64_t S, double scale, bool accumulate, double* part, double* dout,
                         int64_t ld);
// vt[s + j ldv] = y_j - F[j + (s0 + s) ldf] - sqn E[j + (s0 + s) lde] for s < scur, j < n, zero up to m_pad x n_pad: the rows of a solve chunk
int launch_paths_residual(hipStream_t s, const double* y, const double* F, int64_t ldf, const double* E, int64_t lde, double sqn, int64_t s0,
                          int64_t scur, int64_t n, int64_t m_pad, int64_t n_pad, double* vt, int64_t ldv);
// U[j + (s0 + s) ldu] = vt[s + (n_pad - 1 - j) ldv], s < scur, j < n: out of the column-reversed solved chunk
int launch_paths_weights(hipStream_t s, const double* vt, int64_t ldv, int64_t n_pad, int64_t s0, int64_t scur, int64_t n, double* U, int64_t ldu);

// ---- launchers (kernels_cg.hip: the iterative exact GPR) ------------------------------------------
// A block of right-hand sides of the conjugate-gradient loop is at most CG_SB columns (the product's sample block); its scalars live in
// `sc`, CG_ROWS rows of CG_SB doubles: |b|^2, the stop threshold tol^2 |b|^2, r^T z, |r|^2 (what the host reads; -1: p^T A p was not
// finite or not positive) and 1 / 0 for running / frozen.  Buffers are n x S with pitch n.  Order of summation: kernels_cg.hip.
constexpr int CG_SB = 64;
enum CgRow { CG_BB = 0, CG_THR2 = 1, CG_RZ = 2, CG_RR = 3, CG_ACT = 4, CG_ROWS = 5 };
// The partial pivoted Cholesky of K(X, X) (k(x, x) = 1: the kernels of with_gradient_kernel), matrix-free, r <= n steps: L (n x r, pitch
// ldl; the columns from the rank on are zero), piv (r), and state[0] = -1 after a full sweep, else the rank at which the largest
// remaining diagonal was <= n 2^-52.  pval (r), dg (n): work.  2 r launches, no host synchronisation.
int launch_pivoted_cholesky(hipStream_t s, const KernelSpec& ks, const double* X, int64_t d, int64_t n, int64_t r, double* L, int64_t ldl, int64_t* piv,
                            double* pval, double* dg, int* state);
int launch_copy_scaled(hipStream_t s, const double* src, int64_t lds, double* dst, int64_t ldd, int64_t rows, int64_t cols, double div);   // dst = src / div
// Z = (V - Q (Q^T V)) / noise: Q n x r, V and Z n x S, T r x S work, all with pitch = rows.  Profiled as PK_ROWREDUCE.
int launch_apply_precond(hipStream_t s, const double* Q, int64_t r, const double* V, int64_t n, int64_t S, double noise, double* T, double* Z);
int launch_cg_init(hipStream_t s, const double* B, int64_t ldb, int64_t n, int64_t S, double tol, double* R, double* X, double* sc);   // r = b, x = 0
// AP = K P on entry: AP += noise P, alpha, x += alpha p, r -= alpha Ap, |r|^2, freeze.  hist: null, or max_iter x CG_SB x 2 doubles that
// get every running column's coefficients, alpha of step it (from 0) at hist[(it CG_SB + s) 2] (cg_step) and the beta that follows it at
// hist[(it CG_SB + s) 2 + 1] (cg_direction, not `first`); x, r, p and the scalars have the same bits with and without it.
int launch_cg_step(hipStream_t s, const double* P, double* AP, double* X, double* R, int64_t n, int64_t S, double noise, double* sc, double* hist = nullptr,
                   int it = 0);
int launch_cg_direction(hipStream_t s, const double* R, const double* Z, double* P, int64_t n, int64_t S, bool first, double* sc, double* hist = nullptr,
                        int it = 0);   // beta, p = z + beta p
// AX = K X on entry: out[s] = |b_s - (K + noise I) x_s| / |b_s|
int launch_cg_residual(hipStream_t s, const double* B, int64_t ldb, const double* AX, const double* X, int64_t n, int64_t S, double noise, const double* sc,
                       double* out);
int launch_cg_var(hipStream_t s, const double* A, const double* W, int64_t n, int64_t S, double* out);   // out[s] = 1 - a_s . w_s
// F = (y 1^T - F) - sqn E in place: the right-hand sides of the sample paths from the prior term
int launch_paths_rhs(hipStream_t s, const double* y, double* F, int64_t ldf, const double* E, int64_t lde, double sqn, int64_t n, int64_t S);

// ---- launchers (kernels_igrad.hip: the iterative GPR's evidence gradient) -------------------------
// the low-rank-weighted contraction: per workgroup (stripe of 64-row tiles x 64-column tile) `part` gets the ks.n_params sums
//   sum_ij (sum_{r < R} A[i + r lda] B[j + r ldb]) (integrand of theta_k at (x_i, x_j)),   i, j < n,   1 <= R <= IG_RMAX,
// without the factors that do not depend on (i, j) -- those of cross_grad_finish; lowrank_grad_wgs(n) rows of n_params, to be added in
// order.  The weight is formed on the f64 MFMA and never stored.  Kernels: those of with_gradient_kernel.  Profiled as PK_GRAD_CONTRACT.
constexpr int IG_RMAX = 64;
int64_t lowrank_grad_wgs(int64_t n);
int launch_lowrank_grad(hipStream_t s, const KernelSpec& ks, const double* X, int64_t d, int64_t n, const double* A, int64_t lda, const double* B,
                        int64_t ldb, int64_t R, double* part);
// out[s] = sum_i U[i + s ldu] V[i + s ldv], s < S: one workgroup a column, kernels_cg.hip's order of summation
int launch_col_dots(hipStream_t s, const double* U, int64_t ldu, const double* V, int64_t ldv, int64_t n, int64_t S, double* out);
// Z[i + s ldz] = fma(sigma, G2[i + s ldg2], sum_{a < r} L[i + a n] G1[a + s ldg1]) (a ascending), i < n, s < T; r = 0: Z = G2
int launch_igpr_probes(hipStream_t s, const double* L, int64_t r, const double* G1, int64_t ldg1, const double* G2, int64_t ldg2, double sigma,
                       int64_t n, int64_t T, double* Z, int64_t ldz);

// ---- launchers (kernels_batch.hip: small GPs in batches) -------------------------------------------
// One model of n_b <= GPRC_BATCH_MAX_N points per workgroup: fill, factor, solve and (want_grad) the gradient's sums in one launch of
// `models` <= GPRC_BATCH_LAUNCH workgroups; workgroup g handles model b0 + g.  Per model b (all DEVICE memory):
//   prm + b prm_stride   np_store doubles of make_deriv_spec(ks).p, then the noise, then n_b as a double
//   X + b x_stride, y + b y_stride   its points (point-major, d coordinates each) and targets; entries from n_b on are never read
//   out + b out_stride   logp, then (want_grad) the n_params sums WITHOUT the factors that do not depend on (i, j) -- the host halves
//                        them and applies cross_grad_finish -- and sum_i M_ii
//   alpha + b 128        alpha, zero from n_b on;   info + b: 0 or the first non-positive pivot, 1-based (zeroed by the caller)
// slab: batch_scratch_doubles(models) doubles, L and L^-1 of workgroup g at slab + g 2 128^2.  Kernels: those of with_gradient_kernel.
constexpr int GPRC_BATCH_LAUNCH = 256;
struct BatchArgs {
  const double* X;
  const double* y;
  const double* prm;
  double* slab;
  double* out;
  double* alpha;
  int* info;
  int64_t x_stride, y_stride, d, b0;
  int prm_stride, np_store, n_params, out_stride, want_grad;
  // where L^-1 goes: null -- behind L in the slab, as above; else model b's at w + b w_stride (128^2 doubles, column-major, zero above the
  // diagonal), and the slab is batch_scratch_doubles(models, true) doubles, L of workgroup g at slab + g 128^2.  No output depends on it.
  double* w = nullptr;
  int64_t w_stride = 0;
};
size_t batch_scratch_doubles(int64_t models, bool keep_w = false);
int launch_batch_logp_grad(hipStream_t s, int kernel, const BatchArgs& a, int64_t models);

// ---- launchers (kernels_batch_predict.hip: predictions from a fitted batch) ------------------------
// Posterior mean and latent variance of `models` fitted small models at their own (or one shared) set of test points, one launch:
// workgroup (sp, g) of a (split, models) grid handles the 16-point tiles sp 8 + wave, + split 8, ... of model b0 + g.  Per model b (all
// DEVICE memory): prm, X as BatchArgs'; alpha + b 128; W + b 128^2 (BatchArgs::w's layout); info + b (not 0: NaN is written);
// Xs + b xs_stride its test points (point-major), ns_each[b] of them (null: ns_max); mean / var + b ld_out (either may be null).
constexpr int BATCH_PREDICT_TILE = 16;    // test points per wave
constexpr int BATCH_PREDICT_WAVES = 8;    // waves per workgroup: a workgroup takes 128 points per turn
struct BatchPredictArgs {
  const double* X;
  const double* prm;
  const double* alpha;
  const double* W;
  const int* info;
  const double* Xs;
  const int64_t* ns_each;
  double* mean;
  double* var;
  int64_t x_stride, xs_stride, d, ns_max, ld_out, b0;
  int prm_stride, np_store, n_params;
  // launch_batch_predict_grad only: model b's gradients of test point j with respect to coordinate c at dmean / dvar + b ld_grad + d j + c
  // (either may be null; with both null the launch is launch_batch_predict's work and bits), ld_grad >= d ns_max
  double* dmean = nullptr;
  double* dvar = nullptr;
  int64_t ld_grad = 0;
};
int launch_batch_predict(hipStream_t s, int kernel, const BatchPredictArgs& a, int64_t models, int split);
// The same launch with the gradients with respect to the test points (the same kernel body behind a template flag: mean and var keep
// launch_batch_predict's bits):  dmean = -t_c sum_k alpha_k h_k (x*_c - x_kc),  dvar = 2 t_c sum_k u_k h_k (x*_c - x_kc),  u = W^T (W k*).
int launch_batch_predict_grad(hipStream_t s, int kernel, const BatchPredictArgs& a, int64_t models, int split);

// ---- launchers (kernels_batch_gpc.hip: small Laplace classifiers in batches) -----------------------
// One classifier of n_b <= GPRC_BATCH_MAX_N points per workgroup: K, the whole Newton loop of the mode search and the final factorisation
// in one launch of `models` <= GPRC_BATCH_LAUNCH workgroups; workgroup g handles model b0 + g.  Per model b (all DEVICE memory):
//   prm, X, y            as BatchArgs' (the record's noise slot is not read; y in {-1, +1})
//   logq + b, iters + b (iters may be null), info + b (zeroed by the caller): the Laplace evidence, the iterations, and 0, the first
//                        non-positive pivot (1-based), GPRC_BATCH_GPC_MAXITER or GPRC_BATCH_GPC_NONFINITE; a flagged model's logq is NaN
//   alpha + b 128        g = (y + 1) / 2 - pi at the mode;   fhat + b 128: the mode (both zero from n_b on, NaN when flagged)
//   w + b 128^2          L^-1 diag(sw) of B = I + sw K sw = L L^T in BatchArgs::w's layout: launch_batch_predict on (alpha, w) is the
//                        latent prediction of gprc_gpc_predict_latent
// slab: batch_gpc_scratch_doubles(models) doubles, K of workgroup g at slab + g 128^2.  Kernels: those of with_gradient_kernel.
constexpr int GPRC_BATCH_GPC_MAX_ITER = 1000;   // the loop is bounded on the device: the host refuses more
struct BatchGpcArgs {
  const double* X;
  const double* y;
  const double* prm;
  double* slab;
  double* logq;
  int* iters;
  double* alpha;
  double* fhat;
  double* w;
  int* info;
  int64_t x_stride, y_stride, d, b0;
  int prm_stride, np_store, n_params, max_iter;
  double epsilon;
};
size_t batch_gpc_scratch_doubles(int64_t models);
int launch_batch_gpc_fit(hipStream_t s, int kernel, const BatchGpcArgs& a, int64_t models);

// ---- launchers (kernels_batch_loo.hip: leave-one-out from a fitted batch) --------------------------
// One workgroup per model, model b0 + g: p_i = sum_{k >= i} W[k + 128 i]^2, mean_i = y_i - alpha_i / p_i, var_i = 1 / p_i,
// logdens_i = 1/2 log p_i - alpha_i^2 / (2 p_i) - 1/2 log 2 pi at mean / var / dens + b ld_out + i, i < n_b (each may be null), and
// score[b] = sum_i logdens_i (may be null).  A flagged model (info != 0) gets NaN.  All DEVICE memory; prm, alpha, W, info as above.
struct BatchLooArgs {
  const double* W;
  const double* alpha;
  const double* y;
  const double* prm;
  const int* info;
  double* mean;
  double* var;
  double* dens;
  double* score;
  int64_t y_stride, ld_out, b0;
  int prm_stride, np_store;
};
int launch_batch_loo(hipStream_t s, const BatchLooArgs& a, int64_t models);

// ---- launchers (kernels_knn.hip: exact nearest neighbours, the front of the local GPR) -------------
// Per query j < ns the m <= 128 candidates i < n with the smallest key (dist2, i), lexicographic, ascending, at idx / dist + j ld (dist may
// be null; ld >= m), dist2 = sum_c ((xs_jc - x_ic) scale_c)^2 with c ascending (scale null: 1).  All DEVICE memory, points point-major.
// knn_split chooses, from n, ns and the CU count only, into how many parts the candidates are cut (few queries: so that every CU has
// work); the parts' lists are merged on the same key, so no output bit depends on the split.  work: knn_workspace_doubles() doubles.
void knn_split(int64_t n, int64_t ns, int cus, int* parts, int64_t* part_len);
size_t knn_workspace_doubles(int64_t ns, int m, int parts);
int launch_knn(hipStream_t s, const double* X, int64_t d, int64_t n, const double* Xs, int64_t ns, const double* scale, int m, int* idx, double* dist,
               int64_t ld, int parts, int64_t part_len, double* work);
// The predecessor-constrained search (gprc_dev_knn_before): query j < count is column first + j of X itself and its candidates are the
// columns i < first + j only; ranks that no candidate fills report -1 and +inf.  Same key, tie rule, layout, split and merge; the split
// is knn_split(first + count, count, ...).
int launch_knn_before(hipStream_t s, const double* X, int64_t d, int64_t first, int64_t count, const double* scale, int m, int* idx, double* dist, int64_t ld,
                      int parts, int64_t part_len, double* work);
// the neighbours as the slabs gprc_gpr_batch_fit reads: Xg + j d m the m points of query j (point-major, in idx's order), yg + j m their
// targets; an index < 0 (an empty rank) gives NaN
int launch_knn_gather(hipStream_t s, const int* idx, int64_t ld, const double* X, const double* y, int64_t d, int64_t ns, int64_t m, double* Xg, double* yg);

// ---- launchers (kernels_vecchia.hip: the conditionals of the Vecchia likelihood) -------------------
// One conditional log p(y_i | y_N(i)) per workgroup, `count` <= GPRC_VECCHIA_CHUNK points i0 .. i0 + count - 1 per launch, i0 a multiple of
// 256.  All DEVICE memory: X (d x n, point-major), y (n), nbr (n rows of m ranks, pitch m: the neighbours of gprc_dev_knn_before, the first
// rank of -1 ends the model; m = 0: not read), ks (make_deriv_spec of the caller's spec), and per point j = i - i0 of the launch
//   out + j out_stride   cond_i, then (want_grad) the n_params sums WITHOUT the factors that do not depend on the pair -- the host halves
//                        them after the sum over points and applies cross_grad_finish -- and sum_r G_rr;  out_stride = n_params + 2
//   info + j             0, or the first non-positive pivot, 1-based: cond_i and the sums of such a point are NaN
// launch_vecchia_reduce: row g of grp (out_stride + 1 doubles) = the columns of the points [256 g, 256 g + 256) of the launch added in a
// fixed order (want_grad: all of them, else the first alone) and, last, the number of flagged points among them; cond (may be null) + j
// gets cond_i.  Kernels: those of with_gradient_kernel.
struct VecchiaArgs {
  const double* X;
  const double* y;
  const int* nbr;
  const KernelSpec* ks;
  double* out;
  int* info;
  int64_t d, i0;
  double noise;
  int m, n_params, out_stride, want_grad;
};
struct VecchiaReduceArgs {
  const double* out;
  const int* info;
  double* grp;
  double* cond;
  int64_t count;
  int out_stride, want_grad;
};
int launch_vecchia(hipStream_t s, int kernel, const VecchiaArgs& a, int64_t count);
int launch_vecchia_reduce(hipStream_t s, const VecchiaReduceArgs& a);

// ---- launchers (kernels_sgrad.hip) -------------------------------------------------------------
// the sparse bound gradient's contraction over G (rows_pad x cols_pad, column-major, pitch ld; rows_pad % 128 == 0, cols_pad % 64 == 0),
// k and its derivatives recomputed from the row points A (d x rows) and the column points Z (d x cols); rows >= rows and columns >= cols
// of G are never used.  Per workgroup (stripe of row tiles x column tile) `part` gets the n_params sums
//   sum_ij G_ij (integrand of theta_k)      without the factors that do not depend on (i, j): cross_grad_wgs() rows of n_params,
// and, pz != nullptr, per (stripe, coordinate, column)   pz[(st d + c) cols_pad + j] = sum_i G_ij h_ij (a_ic - z_jc)   (ARD: the scaled
// difference).  cross_grad_stripes(rows_pad) stripes, a function of rows_pad only; cross_grad_partials / _zpartials: the doubles of
// part / pz that serve every rows_pad.
// cross_grad_add_partials: acc[k] += f * (the sum of a launch's partials, copied to the host, in workgroup order);  cross_grad_finish:
// grad_out[k] = factor_k * acc[k];  launch_cross_grad_sum: dZ[c + d j] += f * factor_c * (the stripes of pz in order), j < cols.
// Kernels: those of with_gradient_kernel.  Profiled as PK_GRAD_CONTRACT.
int64_t cross_grad_stripes(int64_t rows_pad);
int64_t cross_grad_wgs(int64_t rows_pad, int64_t cols_pad);
int64_t cross_grad_partials(int64_t cols_pad, int n_params);
int64_t cross_grad_zpartials(int64_t cols_pad, int64_t d);
int launch_cross_grad(hipStream_t s, const KernelSpec& ks, const double* G, int64_t ld, const double* A, int64_t rows, int64_t rows_pad,
                      const double* Z, int64_t cols, int64_t cols_pad, int64_t d, double* part, double* pz);
int launch_cross_grad_sum(hipStream_t s, const KernelSpec& ks, const double* pz, int64_t rows_pad, int64_t cols_pad, int64_t cols, int64_t d, double f,
                          double* dZ);
void cross_grad_add_partials(const double* part_host, int64_t rows_pad, int64_t cols_pad, int n_params, long double f, long double* acc);
void cross_grad_finish(const KernelSpec& ks, const long double* acc, double* grad_out);
int launch_rank_one(hipStream_t s, double* C, int64_t ld, int64_t rows, int64_t cols, const double* u, const double* v, double sign);   // C[i,j] = sign u_i v_j
// from the lower triangles of W = -B^-1 and of B (n x n, pitch n), in place, both triangles written:  W := I + W,  B := 2 I + W - B
int launch_sgrad_mid(hipStream_t s, double* W, double* B, int64_t n);

// ---- launchers (kernels_gemm.hip: no flags between workgroups) ---------------------------------
// the predict's in-panel solve of panel p in one launch (see solve_panel_fused_kernel)
int launch_solve_panel_fused(hipStream_t s, double* vt, int64_t ldv, int64_t m_pad, const double* packed, int64_t n_pad, int64_t p,
                             const double* winv, double* sspart, int64_t ss_stride = 0);   // ss_stride: rows per block of sspart (0: m_pad)
// X[M x 128] := X * W^T for lower-triangular 128x128 W (= inverse of a diagonal block of L)
int launch_trsm_panel(hipStream_t s, double* X, int64_t ldx, int64_t M, const double* winv, double* ssq = nullptr);
// C[M x N] -= A[M x K] * B[N x K]^T; lower_diag >= 0: row tile r / col tile c with r + lower_diag < c is skipped
// kind PK_INV_GEMM (square, lower, A and B upper triangular): the tile of row tile r starts its products at column r 128
int launch_gemm_nt(hipStream_t s, double* C, int64_t ldc, const double* A, int64_t lda, const double* B, int64_t ldb,
                   int64_t M, int64_t N, int64_t K, int lower, int kind);
// left-looking predict-solve step: vt[:, j NB:(j+G) NB] -= vt[:, 0:j NB] * L[j NB:(j+G) NB, 0:j NB]^T   (L packed)
// tri_row0 >= 0: the rows of vt are rows tri_row0.. of the identity (zero left of their own column): per tile the pass starts there
int launch_solve_left(hipStream_t s, double* vt, int64_t ldv, int64_t m_pad, const double* packed, int64_t n_pad, int64_t j, int64_t G,
                      int64_t tri_row0 = -1);
// trailing update of packed panels q_begin, q_begin+q_stride, ... < q_end with factored panel p
int launch_trailing_update(hipStream_t s, double* packed, int64_t n_pad, int64_t p, int64_t q_begin, int64_t q_end,
                           int64_t q_stride);
// ... with the source panels [p_begin, p_end) in one pass (p_begin = 0, p_end = q_begin: the left-looking update of a group)
int launch_trailing_range(hipStream_t s, double* packed, int64_t n_pad, int64_t p_begin, int64_t p_end, int64_t q_begin, int64_t q_end,
                          int64_t q_stride);

// ---- launchers (kernels_gram.hip: the sparse GPR's reductions over the rows of a solved chunk) ----
// packed(lower) += vt[0:rows, 0:n_pad]^T vt[0:rows, 0:n_pad], straight into the packed block-column layout (128 x 128 tiles on or below
// the block diagonal; a diagonal tile is written whole).  vt: column-major, ld even; rows % 256 == 0.  An element is the stored value
// plus its rows' products in ascending row order: a call with r1 + r2 rows gives the bits of two calls with r1, then r2 rows.
int launch_gram_rows(hipStream_t s, const double* vt, int64_t ld, int64_t rows, int64_t n_pad, double* packed);
// out[j] += sum_i vt[i, j] w[i], j < cols; rows % 256 == 0, w: `rows` doubles (zero where vt's rows are padding); the same invariance
int launch_col_reduce(hipStream_t s, const double* vt, int64_t ld, int64_t rows, int64_t cols, const double* w, double* out);
int launch_gram_to_b(hipStream_t s, double* packed, int64_t n_pad, double sigma2);   // packed := I + packed / sigma2 (every stored element)
int launch_div_vec(hipStream_t s, double* x, int64_t n, double f);                    // x /= f

// ---- launchers (kernels_chol.hip: PanelSync flags, the wait records) --------------------------
// (what they are told -- trace, split, part, forced, wgs, core, head_slices -- is decided in gprc_sched.hip)
// factor the 128x128 diagonal block at A (ld) in LDS, write L in place and its inverse to winv
int launch_potf2_inv(hipStream_t s, double* A, int64_t lda, double* winv, int* info_dev, int col0);
// the whole of panel p (four diagonal blocks, panel solves, in-panel updates) in ONE launch; sync16: 64 bytes of device
// memory the launch may use for its flags (zeroed by the launcher, stream-ordered: one buffer serves a whole stream)
int launch_panel_fused(hipStream_t s, double* packed, int64_t n_pad, int64_t p, double* winv, int* info_dev, void* sync16, int trace);
// factor service (one-GPU right-looking sweep): the dependent chain of all panels in one persistent launch (side stream) + per panel
// the ordinary strips and the trailing update without the next diagonal block (caller's stream)
size_t panel_service_sync_bytes(int64_t P);
int launch_panel_service(hipStream_t s, double* packed, int64_t n_pad, double* winv, int* info_dev, void* sync, void* trace, double* inv,
                         int64_t p_begin, int64_t p_end, bool split, int part);
// inv (n_pad x NB doubles): per panel the explicit inverse of its NB x NB diagonal block, transposed -- what the vector solves use
int launch_inv512(hipStream_t s, const double* packed, int64_t n_pad, const double* winv, double* inv, int64_t p_begin, int64_t p_end);
int launch_service_gate(hipStream_t s, int64_t n_pad, int* info_dev, void* sync, int launches, bool forced);
int launch_panel_strips(hipStream_t s, double* packed, int64_t n_pad, int64_t p, double* winv, int* info_dev, void* sync, void* trace);
int launch_trailing_service(hipStream_t s, double* packed, int64_t n_pad, int64_t p, double* winv, int* info_dev, void* sync, void* trace, int64_t q_end);
int launch_trailing_sweep(hipStream_t s, double* packed, int64_t n_pad, int64_t g0, int64_t g1, double* winv, int* info_dev, void* sync, void* trace,
                          int wgs, int core, int head_slices);
std::string wait_timeout_report();   // who gave up first in the last timed-out factorisation, "" if nobody

// ---- launchers (kernels_vec.hip) ---------------------------------------------------------------
// vector solves: inv = the explicit diagonal-block inverses (launch_inv512 / the factor service), work = gprc_trsv_work_size doubles
int launch_trsv_step(hipStream_t s, const double* packed, const double* inv, int64_t n_pad, double* b, int transpose, int p, double* work);
int launch_trsv(hipStream_t s, const double* packed, const double* inv, int64_t n_pad, double* b, int transpose, double* work);
int64_t rowreduce_splits(int64_t cols);
int launch_row_reduce(hipStream_t s, const double* vt, int64_t ld, int64_t rows, int64_t cols, const double* w, double* out,
                      double* work);
// out[0] = -0.5*y.alpha - sum(log(diag L)) - n/2 log(2 pi)   (R/GPRclass.R:153); n valid entries
int launch_logp(hipStream_t s, const double* packed, int64_t n_pad, int64_t n, const double* y, const double* alpha, double* out);
// extend (gpr_extend): panels [0, n0 / NB) of the factor in layout n_pad_new from the old factor (layout n_pad_old: its rows < n0) and
// the solved tail rows vt (t_pad x n0, ld ldv; t valid rows = global rows n0 .. n0 + t - 1), zero below; bandwidth-bound
int launch_extend_merge(hipStream_t s, const double* old_packed, int64_t n_pad_old, const double* vt, int64_t ldv, int64_t t_pad, int64_t t,
                        int64_t n0, int64_t n_pad_new, double* packed);
// the reversed factor M = J L^T J (J: reversal of n_pad indices; M is lower triangular) in L's packed layout, zero above the diagonal,
// and the matching diagonal-block inverses J winv_block(B - 1 - b)^T J: solve_rows with them computes (V J) M^-T = (V L^-1) J
int launch_reverse_factor(hipStream_t s, const double* packed, const double* winv, int64_t n_pad, double* packed_rev, double* winv_rev);
// vt[:, j] <-> vt[:, cols - 1 - j] in place, rows [0, rows)
int launch_reverse_cols(hipStream_t s, double* vt, int64_t ld, int64_t rows, int64_t cols);
// unpack the factor into a dense n x n lower matrix (upper = 0)
int launch_unpack_L(hipStream_t s, const double* packed, int64_t n_pad, int64_t n, double* out, int64_t ld_out);
// out[i] = (minuend ? minuend[i] : 0) -/+ sum_{t < nparts} part[t * stride + i], summed in t order: the tail of the fused
// predict epilogues (mean = sum of the fill's partials; var = k(x*,x*) - sum of the solve's per-block sums of squares)
int launch_sum_partials(hipStream_t s, const double* part, int64_t nparts, int64_t stride, int64_t rows, const double* minuend, double* out);
// GPC vector stages (R/GPCclass.R:78-86, 99-103, 110-114)
int launch_gpc_pre(hipStream_t s, const double* f, const double* y, int64_t n, double* sw, double* b);
int launch_gpc_scale(hipStream_t s, const double* sw, const double* v, double* out, int64_t n);                   // out = sw*v
int launch_gpc_a(hipStream_t s, const double* b, const double* sw, const double* t, double* a, int64_t n);        // a = b - sw*t
int launch_gpc_objective(hipStream_t s, const double* a, const double* f, const double* y, int64_t n, double* out);
int launch_gpc_build_B(hipStream_t s, const double* Kfull, int64_t n_pad, const double* sw, double* packed);
int launch_gpc_grad(hipStream_t s, const double* f, const double* y, int64_t n, double* g, double* sw);           // g=(y+1)/2-P
int launch_gpc_class_prob(hipStream_t s, const double* fs, const double* vf, double* out, int64_t n);              // R/GPCclass.R:116-117
// evidence gradient (gprc_gpc_logq_grad): s2_i = 1/2 Sigma_ii d3_i with Sigma_ii = (1 - (B^-1)_ii) / W_ii from the diagonal of
// negBinv = -B^-1 (n_pad x n_pad, ld) and d3_i = W_i (2 pi_i - 1); zero in the padding.  W_i cancels: 1/2 (1 + negBinv_ii) (2 pi_i - 1)
int launch_gpc_s2(hipStream_t s, const double* f, const double* negBinv, int64_t ld, int64_t n, double* s2);
int launch_diag_log_sum(hipStream_t s, const double* packed, int64_t n_pad, int64_t n, double* out);              // sum(log(diag(L)))
// leave-one-out cross-validation (gprc_gpr_loo, gprc_gpr_loo_grad).  launch_loo_point: per point i < n the LOO mean, variance and log
// density from alpha and p_i = (K_y^-1)_ii (pdiag, or the diagonal of negKinv = -K_y^-1 with leading dimension ld: exactly one of the
// two); null outputs are skipped; w, sc, mask (all three or none, n_pad entries, zero in the padding): alpha_i / p_i, sqrt(c_i), 1
int launch_loo_point(hipStream_t s, const double* alpha, const double* y, const double* pdiag, const double* negKinv, int64_t ld, int64_t n,
                     int64_t n_pad, double* mean, double* var, double* ell, double* w, double* sc, double* mask);
// Q = P diag(sc), the full n_pad x n_pad matrix (ld n_pad), from the lower 128-tiles of negP = -P (ld n_pad); bandwidth-bound
int launch_loo_q(hipStream_t s, const double* negP, const double* sc, int64_t n_pad, double* Q);
// out[i] = u_i alpha_i + 1/2 S_ii, i < n: the terms of d LOO / d noise
int launch_loo_noise_terms(hipStream_t s, const double* u, const double* alpha, const double* S, int64_t ld, int64_t n, double* out);
// sampling support (kernels_eig.hip)
int launch_pack_dense(hipStream_t s, const double* A, int64_t lda, int64_t m, int64_t n_pad, double* packed);
int launch_sym_absmax(hipStream_t s, const double* A, int64_t lda, int m, double* mx);
int launch_sym_copy(hipStream_t s, const double* A, int64_t lda, int64_t m, double scale, double* W, double* V);
int launch_jacobi_sweep(hipStream_t s, double* W, double* V, int m, double* cs);
int launch_jacobi_offnorm(hipStream_t s, const double* W, int m, double* off, double* dg);
int launch_gather_scale_cols(hipStream_t s, const double* V, int m, const int* perm, const double* scale, double* out, int64_t ldo);
int launch_affine_lz(hipStream_t s, const double* L, int64_t ldl, int64_t m, const double* mean, const double* Z, int64_t ldz,
                     int64_t ndraws, double* out, int64_t ldo, int lower);
int launch_combine_all(hipStream_t s, const double* vals_dev, const int64_t* lengths, int d, double* out);
int launch_diag_sum(hipStream_t s, const double* packed, int64_t n_pad, int64_t n, double* out);                  // sum(diag(L))

}  // namespace gprc
