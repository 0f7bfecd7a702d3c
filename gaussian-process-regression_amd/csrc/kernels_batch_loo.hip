// kernels_batch_loo.hip -- leave-one-out cross-validation of a fitted batch of small GPs for gfx950 (gprc_gpr_batch_loo; DESIGN.md
// section 7, "Batched prediction gradients and LOO"), in closed form from what the fit keeps: W = L^-1 (128 x 128, column-major,
// W[k][i] at k + 128 i, zero above the diagonal), alpha and y.  With p_i = (K_y^-1)_ii = sum_{k >= i} W[k][i]^2:
//   mean_i = y_i - alpha_i / p_i,     var_i = 1 / p_i (of the noisy y_i),     logdens_i = 1/2 log p_i - alpha_i^2 / (2 p_i) - 1/2 log 2 pi.
//
// ONE WORKGROUP (four waves) per model, one launch for the batch.  Column i of W is contiguous; wave w owns the columns i = w, w + 4, ...
// < n_b, lane l reads its rows l and l + 64 (512 contiguous bytes a wave and load; rows above the diagonal and from n_b on are not
// read).  A bandwidth kernel: half of 128 KiB a model.
//
// Order of summation, fixed and a function of n_b alone -- a model's bits do not depend on the batch or on which outputs are asked for:
//   p_i        lane l: W[l][i]^2, then fma of W[l + 64][i]^2 (a row outside i .. n_b - 1 counts as 0); then the 64 lanes by xor-shuffles
//              32, 16, 8, 4, 2, 1 (every lane ends with the same bits)
//   the score  logdens_i to LDS (0 from n_b on); wave 0, lane l: logdens_l + logdens_(l + 64); the same six shuffles
// No atomics, no scratch.  A model whose factorisation was flagged (info != 0) gets NaN and reads nothing but its info word and count.
#include "gprc_internal.h"

namespace gprc {

namespace {

constexpr int BL_N = 128;          // GPRC_BATCH_MAX_N: the extent of W
constexpr int BL_WAVES = 4;
constexpr int BL_THREADS = 64 * BL_WAVES;
constexpr double BL_HALF_LOG_2PI = 0.91893853320467274178;

__device__ __forceinline__ double wave_sum_fixed(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(BL_THREADS) void batch_loo_kernel(BatchLooArgs a) {
  __shared__ double dl[BL_N];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int64_t b = a.b0 + blockIdx.x;
  const int nb = (int)a.prm[b * a.prm_stride + a.np_store + 1];
  double* mean = a.mean ? a.mean + b * a.ld_out : nullptr;
  double* var = a.var ? a.var + b * a.ld_out : nullptr;
  double* dens = a.dens ? a.dens + b * a.ld_out : nullptr;

  if (a.info[b] != 0) {                 // not positive definite: flagged by the fit, NaN here
    const double qnan = __builtin_nan("");
    for (int i = t; i < nb; i += BL_THREADS) {
      if (mean) mean[i] = qnan;
      if (var) var[i] = qnan;
      if (dens) dens[i] = qnan;
    }
    if (t == 0 && a.score) a.score[b] = qnan;
    return;
  }

  const double* W = a.W + b * (int64_t)(BL_N * BL_N);
  for (int i = wave; i < BL_N; i += BL_WAVES) {            // uniform over the wave
    if (i >= nb) {
      if (lane == 0) dl[i] = 0.0;
      continue;
    }
    const double* col = W + (int64_t)BL_N * i;
    const int k0 = lane, k1 = lane + 64;
    const double w0 = (k0 >= i && k0 < nb) ? col[k0] : 0.0;
    const double w1 = (k1 >= i && k1 < nb) ? col[k1] : 0.0;
    const double p = wave_sum_fixed(fma(w1, w1, w0 * w0));
    if (lane == 0) {
      const double al = a.alpha[b * BL_N + i], yi = a.y[b * a.y_stride + i];
      const double e = 0.5 * log(p) - (al * al) / (2.0 * p) - BL_HALF_LOG_2PI;
      dl[i] = e;
      if (mean) mean[i] = yi - al / p;
      if (var) var[i] = 1.0 / p;
      if (dens) dens[i] = e;
    }
  }
  __syncthreads();
  if (wave == 0 && a.score) {
    const double sc = wave_sum_fixed(dl[lane] + dl[lane + 64]);
    if (lane == 0) a.score[b] = sc;
  }
}

}  // namespace

int launch_batch_loo(hipStream_t s, const BatchLooArgs& a, int64_t models) {
  if (models < 1 || models > 0x7fffffff || !a.W || !a.alpha || !a.y || !a.prm || !a.info || (!a.mean && !a.var && !a.dens && !a.score) ||
      ((a.mean || a.var || a.dens) && a.ld_out < 1) || a.y_stride < 0) {
    set_error("batch_loo: bad launch arguments");
    return GPRC_ERR_ARG;
  }
  hipLaunchKernelGGL(batch_loo_kernel, dim3((unsigned)models), dim3(BL_THREADS), 0, s, a);
  GPRC_LAUNCH_CHECK();
  return 0;
}

}  // namespace gprc
