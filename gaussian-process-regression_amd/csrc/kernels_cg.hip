// kernels_cg.hip -- the kernels of the iterative exact GPR for gfx950 (gprc_iter.hip; DESIGN.md section 7, "Iterative GPR"): everything of a
// preconditioned conjugate-gradient solve with K_y = K(X,X) + noise I except the product K P itself, which is gen_gemm_kernel's
// (kernels_paths.hip).
//   pchol_argmax_kernel / pchol_column_kernel   the partial pivoted Cholesky of K(X,X), matrix-free: one arg-max and one column per step
//   qtv_kernel / apply_precond_kernel            T = Q^T V (r x S) and Z = (V - Q T) / noise: the preconditioner P^-1 = (I - Q Q^T) / noise
//   cg_init / cg_step / cg_direction / cg_residual / cg_var_kernel   the vector steps, one workgroup per right-hand side
// Order of summation, everywhere: row i of a column belongs to thread i mod 256 of its workgroup, a thread adds its rows in ascending
// order (one fma chain), the 64 lanes of a wave are added by a butterfly (xor 1, 2, ..., 32) and the four waves in wave order.  It is a
// function of n alone.  Every right-hand side has its own workgroup (or its own accumulators) and its own scalars in device memory, so a
// column's bits do not depend on which other columns are in the call.  No atomics.
//
// The scalars of a block of at most CG_SB right-hand sides: rows of CG_SB doubles, see CgRow.  alpha and beta never leave the device;
// the host reads the row CG_RR per iteration and nothing else.
#include "pair_tile.h"

namespace gprc {

namespace {

// sum over the workgroup's 256 threads in the fixed order above; every thread gets it.  red: 4 doubles of LDS
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();   // the readers of an earlier sum are done with red
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- partial pivoted Cholesky ----------------------------------------------------------------------------------------------------------
// state[0]: -1 while running, else the rank at which the sweep stopped (dg_p <= thresh).  A chosen point's dg is -1: never a maximum again.
__global__ __launch_bounds__(1024) void pchol_argmax_kernel(const double* dg, int64_t n, double thresh, int64_t j, int64_t* piv, double* pval, int* state) {
  __shared__ double bv[1024];
  __shared__ int64_t bi[1024];
  const int t = threadIdx.x;
  double best = -2.0;
  int64_t idx = n;
  for (int64_t i = t; i < n; i += 1024) {   // ascending: a strict > keeps the lowest index among equals
    const double v = dg[i];
    if (v > best) { best = v; idx = i; }
  }
  bv[t] = best; bi[t] = idx;
  __syncthreads();
  for (int half = 512; half > 0; half >>= 1) {
    if (t < half) {
      const double v = bv[t + half];
      const int64_t i = bi[t + half];
      if (v > bv[t] || (v == bv[t] && i < bi[t])) { bv[t] = v; bi[t] = i; }
    }
    __syncthreads();
  }
  if (t == 0 && state[0] < 0) {
    if (!(bv[0] > thresh)) state[0] = (int)j;
    else { piv[j] = bi[0]; pval[j] = bv[0]; }
  }
}

// column j of L from the pivot piv[j]: L[p, j] = sqrt(dg_p); L[i, j] = (k(x_i, x_p) - sum_{t < j} L[i, t] L[p, t]) / L[p, j], t ascending, for
// the points not yet chosen; 0 for the earlier pivots; dg_i = max(dg_i - L[i, j]^2, 0)
template <int KID>
__global__ __launch_bounds__(256) void pchol_column_kernel(const double* X, int64_t d, int64_t n, KernelSpec ks, int64_t j, const int64_t* piv,
                                                           const double* pval, const int* state, double* L, int64_t ldl, double* dg) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (state[0] >= 0 || i >= n) return;
  const int64_t p = piv[j];
  const double dgi = dg[i];
  if (dgi < 0.0) { L[i + j * ldl] = 0.0; return; }
  const double lpj = sqrt(pval[j]);
  if (i == p) { L[i + j * ldl] = lpj; dg[i] = -1.0; return; }
  double s = 0.0;
  for (int64_t c = 0; c < d; ++c) {
    double a = X[i * d + c], b = X[p * d + c];
    if constexpr (is_ard(KID)) { a *= ks.p[c]; b *= ks.p[c]; }   // the coordinates divided by their length scale, as the product stages them
    const double t = a - b;
    s = fma(t, t, s);
  }
  double acc = kernel_value<KID>(s, ks);
  for (int64_t t = 0; t < j; ++t) acc = fma(-L[i + t * ldl], L[p + t * ldl], acc);
  const double l = acc / lpj;
  L[i + j * ldl] = l;
  dg[i] = fmax(dgi - l * l, 0.0);
}

__global__ __launch_bounds__(256) void fill_value_kernel(double* x, int64_t n, double v) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = v;
}

// dst[i + a ldd] = src[i + a lds] / div, i < rows, a < cols
__global__ __launch_bounds__(256) void copy_scaled_kernel(const double* src, int64_t lds, double* dst, int64_t ldd, int64_t rows, int64_t cols, double div) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * cols) return;
  const int64_t a = idx / rows, i = idx - a * rows;
  dst[i + a * ldd] = src[i + a * lds] / div;
}

// ---- the preconditioner's two tall-skinny products ----------------------------------------------------------------------------------------
constexpr int QT_A = 8, QT_S = 8;   // columns of Q x columns of V per workgroup

// T[a + s ldt] = sum_i Q[i + a ldq] V[i + s ldv], a < r, s < S
__global__ __launch_bounds__(256) void qtv_kernel(const double* __restrict__ Q, int64_t ldq, int64_t r, const double* __restrict__ V, int64_t ldv, int64_t S,
                                                  int64_t n, double* T, int64_t ldt) {
  __shared__ double red[4][QT_A * QT_S];
  const int t = threadIdx.x;
  const int64_t a0 = (int64_t)blockIdx.x * QT_A, s0 = (int64_t)blockIdx.y * QT_S;
  const double *qc[QT_A], *vc[QT_S];
#pragma unroll
  for (int a = 0; a < QT_A; ++a) qc[a] = Q + ((a0 + a < r) ? a0 + a : r - 1) * ldq;   // past the edge: a valid column, its sums dropped
#pragma unroll
  for (int s = 0; s < QT_S; ++s) vc[s] = V + ((s0 + s < S) ? s0 + s : S - 1) * ldv;
  double acc[QT_A][QT_S];
#pragma unroll
  for (int a = 0; a < QT_A; ++a)
#pragma unroll
    for (int s = 0; s < QT_S; ++s) acc[a][s] = 0.0;
  for (int64_t i = t; i < n; i += 256) {
    double q[QT_A], v[QT_S];
#pragma unroll
    for (int a = 0; a < QT_A; ++a) q[a] = qc[a][i];
#pragma unroll
    for (int s = 0; s < QT_S; ++s) v[s] = vc[s][i];
#pragma unroll
    for (int a = 0; a < QT_A; ++a)
#pragma unroll
      for (int s = 0; s < QT_S; ++s) acc[a][s] = fma(q[a], v[s], acc[a][s]);
  }
#pragma unroll
  for (int a = 0; a < QT_A; ++a)
#pragma unroll
    for (int s = 0; s < QT_S; ++s) {
      double v = acc[a][s];
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
      if ((t & 63) == 0) red[t >> 6][a * QT_S + s] = v;
    }
  __syncthreads();
  if (t < QT_A * QT_S) {
    const int a = t / QT_S, s = t - a * QT_S;
    if (a0 + a < r && s0 + s < S) T[(a0 + a) + (s0 + s) * ldt] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
  }
}

// Z[i + s ldz] = (V[i + s ldv] - sum_a Q[i + a ldq] T[a + s ldt]) / noise, a ascending
__global__ __launch_bounds__(256) void apply_precond_kernel(const double* __restrict__ V, int64_t ldv, const double* __restrict__ Q, int64_t ldq,
                                                            const double* __restrict__ T, int64_t ldt, int64_t r, int64_t S, int64_t n, double noise,
                                                            double* Z, int64_t ldz) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t s0 = (int64_t)blockIdx.y * QT_S;
  if (i >= n) return;
  const double* tc[QT_S];
#pragma unroll
  for (int s = 0; s < QT_S; ++s) tc[s] = T + ((s0 + s < S) ? s0 + s : S - 1) * ldt;
  double acc[QT_S];
#pragma unroll
  for (int s = 0; s < QT_S; ++s) acc[s] = 0.0;
  for (int64_t a = 0; a < r; ++a) {
    const double q = Q[i + a * ldq];
#pragma unroll
    for (int s = 0; s < QT_S; ++s) acc[s] = fma(q, tc[s][a], acc[s]);
  }
#pragma unroll
  for (int s = 0; s < QT_S; ++s)
    if (s0 + s < S) Z[i + (s0 + s) * ldz] = (V[i + (s0 + s) * ldv] - acc[s]) / noise;
}

// ---- the vector steps: workgroup s = right-hand side s, buffers n x S with pitch n --------------------------------------------------------
// r = b, x = 0, bb = |b|^2, thr2 = tol^2 bb; a column with bb <= thr2 (b = 0) is frozen from the start
__global__ __launch_bounds__(256) void cg_init_kernel(const double* B, int64_t ldb, int64_t n, double tol, double* R, double* X, double* sc) {
  __shared__ double red[4];
  const int64_t s = blockIdx.x;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const double b = B[i + s * ldb];
    R[i + s * n] = b;
    X[i + s * n] = 0.0;
    acc = fma(b, b, acc);
  }
  const double bb = block_sum(acc, red);
  if (threadIdx.x == 0) {
    const double thr2 = (tol * tol) * bb;
    sc[CG_BB * CG_SB + s] = bb;
    sc[CG_THR2 * CG_SB + s] = thr2;
    sc[CG_RR * CG_SB + s] = bb;
    sc[CG_ACT * CG_SB + s] = (bb <= thr2) ? 0.0 : 1.0;
    sc[CG_RZ * CG_SB + s] = 0.0;
  }
}

// Ap += noise p;  alpha = r^T z / p^T A p;  x += alpha p;  r -= alpha Ap;  rr = |r|^2;  frozen when rr <= thr2.
// p^T A p not finite or not positive: the column is frozen and its rr reads -1 (the host's GPRC_ERR_NOT_PD).  A frozen column is skipped.
// hist != nullptr: alpha of this step (it, from 0) goes to hist[(it CG_SB + s) 2]; x, r and the scalars have the same bits either way.
__global__ __launch_bounds__(256) void cg_step_kernel(const double* P, double* AP, double* X, double* R, int64_t n, double noise, double* sc, double* hist,
                                                      int it) {
  __shared__ double red[4];
  const int64_t s = blockIdx.x;
  if (sc[CG_ACT * CG_SB + s] == 0.0) return;   // workgroup-uniform
  const double rz = sc[CG_RZ * CG_SB + s], thr2 = sc[CG_THR2 * CG_SB + s];
  const double* p = P + s * n;
  double *ap = AP + s * n, *x = X + s * n, *r = R + s * n;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const double pi = p[i], a = fma(noise, pi, ap[i]);
    ap[i] = a;
    acc = fma(pi, a, acc);
  }
  const double pap = block_sum(acc, red);
  if (!(pap > 0.0) || !isfinite(pap)) {   // workgroup-uniform
    if (threadIdx.x == 0) { sc[CG_ACT * CG_SB + s] = 0.0; sc[CG_RR * CG_SB + s] = -1.0; }
    return;
  }
  const double alpha = rz / pap;
  if (hist && threadIdx.x == 0) hist[((int64_t)it * CG_SB + s) * 2] = alpha;
  acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) {   // a thread reads back the Ap it wrote itself
    x[i] = fma(alpha, p[i], x[i]);
    const double ri = fma(-alpha, ap[i], r[i]);
    r[i] = ri;
    acc = fma(ri, ri, acc);
  }
  const double rr = block_sum(acc, red);
  if (threadIdx.x == 0) {
    sc[CG_RR * CG_SB + s] = rr;
    if (rr <= thr2) sc[CG_ACT * CG_SB + s] = 0.0;
  }
}

// rz' = r^T z;  beta = rz' / rz (first: 0);  p = z + beta p.  A frozen column is skipped (first: its p is zero).
// hist != nullptr and not first: beta, which follows step `it`, goes to hist[(it CG_SB + s) 2 + 1].
__global__ __launch_bounds__(256) void cg_direction_kernel(const double* R, const double* Z, double* P, int64_t n, int first, double* sc, double* hist,
                                                           int it) {
  __shared__ double red[4];
  const int64_t s = blockIdx.x;
  const double *r = R + s * n, *z = Z + s * n;
  double* p = P + s * n;
  if (sc[CG_ACT * CG_SB + s] == 0.0) {   // workgroup-uniform
    if (first)
      for (int64_t i = threadIdx.x; i < n; i += 256) p[i] = 0.0;
    return;
  }
  const double rz_old = sc[CG_RZ * CG_SB + s];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) acc = fma(r[i], z[i], acc);
  const double rz = block_sum(acc, red);   // (its barriers order every thread's read of rz_old before the write below)
  const double beta = first ? 0.0 : rz / rz_old;
  if (hist && !first && threadIdx.x == 0) hist[((int64_t)it * CG_SB + s) * 2 + 1] = beta;
  for (int64_t i = threadIdx.x; i < n; i += 256) p[i] = first ? z[i] : fma(beta, p[i], z[i]);
  if (threadIdx.x == 0) sc[CG_RZ * CG_SB + s] = rz;
}

// the true residual: AX = K x on entry; out[s] = |b - (K x + noise x)| / |b|, 0 for b = 0
__global__ __launch_bounds__(256) void cg_residual_kernel(const double* B, int64_t ldb, const double* AX, const double* X, int64_t n, double noise,
                                                          const double* sc, double* out) {
  __shared__ double red[4];
  const int64_t s = blockIdx.x;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const double t = B[i + s * ldb] - fma(noise, X[i + s * n], AX[i + s * n]);
    acc = fma(t, t, acc);
  }
  const double tt = block_sum(acc, red), bb = sc[CG_BB * CG_SB + s];
  if (threadIdx.x == 0) out[s] = bb > 0.0 ? sqrt(tt / bb) : 0.0;
}

// out[s] = 1 - sum_i A[i + s n] W[i + s n]: the pointwise variance of a kernel with k(x, x) = 1
__global__ __launch_bounds__(256) void cg_var_kernel(const double* A, const double* W, int64_t n, double* out) {
  __shared__ double red[4];
  const int64_t s = blockIdx.x;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) acc = fma(A[i + s * n], W[i + s * n], acc);
  const double q = block_sum(acc, red);
  if (threadIdx.x == 0) out[s] = 1.0 - q;
}

// F[j + s ldf] = (y[j] - F[j + s ldf]) - sqn E[j + s lde]: the right-hand sides of the sample paths (paths_residual_kernel's expression)
__global__ __launch_bounds__(256) void paths_rhs_kernel(const double* y, double* F, int64_t ldf, const double* E, int64_t lde, double sqn, int64_t n,
                                                        int64_t S) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * S) return;
  const int64_t s = idx / n, j = idx - s * n;
  F[j + s * ldf] = (y[j] - F[j + s * ldf]) - sqn * E[j + s * lde];
}

unsigned blocks_of(int64_t count) { return (unsigned)((count + 255) / 256); }

}  // namespace

int launch_pivoted_cholesky(hipStream_t s, const KernelSpec& ks, const double* X, int64_t d, int64_t n, int64_t r, double* L, int64_t ldl, int64_t* piv,
                            double* pval, double* dg, int* state) {
  if (!X || !L || !piv || !pval || !dg || !state || d < 1 || n < 1 || r < 1 || r > n || ldl < n) { set_error("pivoted_cholesky: bad arguments"); return GPRC_ERR_ARG; }
  GPRC_TRY(check_grad_kernel("pivoted_cholesky", ks.id));
  const KernelSpec ds = make_deriv_spec(ks);
  const double thresh = (double)n * 0x1p-52;
  GPRC_HIP(hipMemset2DAsync(L, sizeof(double) * ldl, 0, sizeof(double) * n, (size_t)r, s));   // the columns beyond the rank stay zero
  GPRC_HIP(hipMemsetAsync(state, 0xff, sizeof(int), s));                                      // -1: running
  hipLaunchKernelGGL(fill_value_kernel, dim3(blocks_of(n)), dim3(256), 0, s, dg, n, 1.0);
  GPRC_LAUNCH_CHECK();
  for (int64_t j = 0; j < r; ++j) {
    hipLaunchKernelGGL(pchol_argmax_kernel, dim3(1), dim3(1024), 0, s, dg, n, thresh, j, piv, pval, state);
    with_gradient_kernel(ks.id, [&](auto kid) {
      hipLaunchKernelGGL((pchol_column_kernel<decltype(kid)::value>), dim3(blocks_of(n)), dim3(256), 0, s, X, d, n, ds, j, piv, pval, state, L, ldl, dg);
    });
  }
  GPRC_LAUNCH_CHECK();
  return 0;
}

int launch_copy_scaled(hipStream_t s, const double* src, int64_t lds, double* dst, int64_t ldd, int64_t rows, int64_t cols, double div) {
  if (rows <= 0 || cols <= 0) return 0;
  hipLaunchKernelGGL(copy_scaled_kernel, dim3(blocks_of(rows * cols)), dim3(256), 0, s, src, lds, dst, ldd, rows, cols, div);
  GPRC_LAUNCH_CHECK();
  return 0;
}

int launch_apply_precond(hipStream_t s, const double* Q, int64_t r, const double* V, int64_t n, int64_t S, double noise, double* T, double* Z) {
  if (r < 1 || S < 1 || n < 1 || !Q || !V || !T || !Z) { set_error("apply_precond: bad arguments"); return GPRC_ERR_ARG; }
  ProfScope ps(s, PK_ROWREDUCE, 4.0 * n * r * S, 8.0 * ((double)n * r * ((S + QT_S - 1) / QT_S) * 2.0 + 3.0 * n * S));
  hipLaunchKernelGGL(qtv_kernel, dim3((unsigned)((r + QT_A - 1) / QT_A), (unsigned)((S + QT_S - 1) / QT_S)), dim3(256), 0, s, Q, n, r, V, n, S, n, T, r);
  GPRC_LAUNCH_CHECK();
  hipLaunchKernelGGL(apply_precond_kernel, dim3(blocks_of(n), (unsigned)((S + QT_S - 1) / QT_S)), dim3(256), 0, s, V, n, Q, n, T, r, r, S, n, noise, Z, n);
  GPRC_LAUNCH_CHECK();
  return 0;
}

int launch_cg_init(hipStream_t s, const double* B, int64_t ldb, int64_t n, int64_t S, double tol, double* R, double* X, double* sc) {
  hipLaunchKernelGGL(cg_init_kernel, dim3((unsigned)S), dim3(256), 0, s, B, ldb, n, tol, R, X, sc);
  GPRC_LAUNCH_CHECK();
  return 0;
}

int launch_cg_step(hipStream_t s, const double* P, double* AP, double* X, double* R, int64_t n, int64_t S, double noise, double* sc, double* hist, int it) {
  hipLaunchKernelGGL(cg_step_kernel, dim3((unsigned)S), dim3(256), 0, s, P, AP, X, R, n, noise, sc, hist, it);
  GPRC_LAUNCH_CHECK();
  return 0;
}

int launch_cg_direction(hipStream_t s, const double* R, const double* Z, double* P, int64_t n, int64_t S, bool first, double* sc, double* hist, int it) {
  hipLaunchKernelGGL(cg_direction_kernel, dim3((unsigned)S), dim3(256), 0, s, R, Z, P, n, first ? 1 : 0, sc, hist, it);
  GPRC_LAUNCH_CHECK();
  return 0;
}

int launch_cg_residual(hipStream_t s, const double* B, int64_t ldb, const double* AX, const double* X, int64_t n, int64_t S, double noise, const double* sc,
                       double* out) {
  hipLaunchKernelGGL(cg_residual_kernel, dim3((unsigned)S), dim3(256), 0, s, B, ldb, AX, X, n, noise, sc, out);
  GPRC_LAUNCH_CHECK();
  return 0;
}

int launch_cg_var(hipStream_t s, const double* A, const double* W, int64_t n, int64_t S, double* out) {
  hipLaunchKernelGGL(cg_var_kernel, dim3((unsigned)S), dim3(256), 0, s, A, W, n, out);
  GPRC_LAUNCH_CHECK();
  return 0;
}

int launch_paths_rhs(hipStream_t s, const double* y, double* F, int64_t ldf, const double* E, int64_t lde, double sqn, int64_t n, int64_t S) {
  hipLaunchKernelGGL(paths_rhs_kernel, dim3(blocks_of(n * S)), dim3(256), 0, s, y, F, ldf, E, lde, sqn, n, S);
  GPRC_LAUNCH_CHECK();
  return 0;
}

}  // namespace gprc
