// kernels_batch_predict.hip -- predictions from a fitted batch of small GPs for gfx950 (gprc_gpr_batch_predict; DESIGN.md section 7,
// "Batched predict"): posterior mean and latent variance of B models of n_b <= 128 points at each model's test points, one launch.
//
// What a fitted batch keeps per model (gprc_batch.hip): the points, alpha, W = L^-1 as potf2_blocked_body stores it (chol_tile.h: 128 x 128
// doubles, column-major, W[k][i] at k + 128 i, zero above the diagonal, the identity in rows and columns >= n_b) and the parameter
// record of kernels_batch.hip (the constants of make_deriv_spec, the noise, n_b).  With K*[k][j] = k(x_k, x*_j):
//   mean_j = sum_k K*[k][j] alpha_k,     var_j = k(x*_j, x*_j) - sum_i V[i][j]^2,   V = W K*.
//
// ONE WAVE owns 16 test points of one model and needs no other wave.  Lane (lc = lane & 15, lr = lane >> 4) holds column lc of K*: the
// entries k = 4 m + lr, m = 0 .. 31, each formed ONCE -- kernel_value<KID> of the squared distance, coordinates ascending in one fma chain,
// ARD coordinates scaled by bt_scaled_diff as the fit kernel scales them (a test point equal to a training point gives s = 0 exactly) --
// and kept in registers: entry m is exactly the B operand of the v_mfma_f64_16x16x4_f64 whose contraction index runs over 4 m .. 4 m + 3.
// The A operand is W[16 I + lc][4 m + lr], read from an LDS image of the model's W (leading dimension 144, as the factor body's image:
// the operand read is conflict-free).  Row block I of V contracts k only up to the end of block I -- W is triangular -- and the blocks stop
// at the last 16-row block that holds points: 4 + 8 + ... + 32 = 144 MFMAs per 16 points at n_b = 128.  Entries k >= n_b of K* are zero
// (their points are never read), so the identity rows of W add nothing.  Without var_out neither the image nor the products exist.
//
// A workgroup (eight waves) loads one model's alpha and W once (at most 128 KB) and loops over tiles of test points: workgroup (sp, g) of
// the (split, models) grid takes tiles sp 8 + wave, + 8 split, ...; the host picks the split so that a small batch still fills the CUs.
// LDS: 128 x 144 doubles of W, 128 of alpha, the KernelSpec: 150 536 B of the 163 840 B a workgroup may have, one workgroup per CU.
//
// Order of summation, fixed and a function of (n_b, d, kernel) alone -- a test point's bits depend on its model and its coordinates, not on
// its tile, the split, the batch, the other test points or which outputs are asked for:
//   squared distance   coordinates ascending, one fma chain
//   mean_j             lane (lc = j, lr): k = lr, 4 + lr, 8 + lr, ... < 16 ceil(n_b / 16) in one fma chain from 0; then the four lr groups
//                      as (q0 + q1) + (q2 + q3) (two xor-shuffles, 16 then 32; every lane of the column ends with the same bits)
//   V block            the MFMA's own chain over k ascending from 0
//   sum_i V[i][j]^2    lane (lc = j, lr): block I ascending, register g ascending (row 16 I + lr + 4 g), one fma chain from 0; the same
//                      two shuffles;   var_j = k(x*, x*) - that sum, unclamped
// No atomics; no register spills and no scratch (profiles/batch_predict_isa.txt).  A model whose factorisation was flagged (info != 0) gets
// NaN in both outputs and reads nothing but its info word.
#include "chol_tile.h"
#include "pair_tile.h"

namespace gprc {

namespace {

constexpr int BP_WAVES = BATCH_PREDICT_WAVES;
constexpr int BP_THREADS = 64 * BP_WAVES;
constexpr int BP_SPEC_DOUBLES = (sizeof(KernelSpec) + 7) / 8;
constexpr size_t BP_SMEM_BYTES = sizeof(double) * (PB * BLD + PB + BP_SPEC_DOUBLES);
static_assert(BP_SMEM_BYTES <= 163840, "the batched predict kernel's LDS must fit a workgroup's 160 KiB");
static_assert(BATCH_PREDICT_TILE == 16 && PB == 128 && BLD % 2 == 0, "the lane layout is the 16 x 16 x 4 MFMA's");

typedef double v4d __attribute__((ext_vector_type(4)));

template <int KID>
__global__ __launch_bounds__(BP_THREADS) void batch_predict_kernel(BatchPredictArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  constexpr bool ARD = is_ard(KID);
  double* Wl = sm;                      // PB x BLD: W[i][c] at i + c BLD
  double* av = sm + PB * BLD;           // alpha
  KernelSpec& ks = *reinterpret_cast<KernelSpec*>(av + PB);
  const int t = threadIdx.x, lane = t & 63, lc = lane & 15, lr0 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int64_t b = a.b0 + blockIdx.y;
  const int64_t ns = a.ns_each ? a.ns_each[b] : a.ns_max;
  const int64_t tiles = (ns + BATCH_PREDICT_TILE - 1) / BATCH_PREDICT_TILE;
  const int64_t first = (int64_t)blockIdx.x * BP_WAVES, step = (int64_t)gridDim.x * BP_WAVES;
  if (first >= tiles) return;           // the whole workgroup: this model has fewer tiles than the widest one
  double* mean = a.mean ? a.mean + b * a.ld_out : nullptr;
  double* var = a.var ? a.var + b * a.ld_out : nullptr;

  if (a.info[b] != 0) {                 // not positive definite: flagged by the fit, NaN here
    const double qnan = __builtin_nan("");
    for (int64_t tile = first + wave; tile < tiles; tile += step) {
      const int64_t j = tile * BATCH_PREDICT_TILE + lc;
      if (lr0 == 0 && j < ns) {
        if (mean) mean[j] = qnan;
        if (var) var[j] = qnan;
      }
    }
    return;
  }

  const double* prm = a.prm + b * a.prm_stride;
  const double* X = a.X + b * a.x_stride;
  const double* Xs = a.Xs + b * a.xs_stride;
  const int nb = (int)prm[a.np_store + 1];
  const int nblk = (nb + 15) >> 4, kend = 16 * nblk;
  const int64_t d = a.d;

  // ---- load: the spec, alpha, and (variance) rows and columns < kend of W, two rows a thread and load
  if (t == 0) { ks.id = KID; ks.n_params = a.n_params; }
  for (int k = t; k < a.np_store; k += BP_THREADS) ks.p[k] = prm[k];
  if (t < PB) av[t] = a.alpha[b * PB + t];
  if (var) {
    const double* W = a.W + b * (PB * PB);
    const int i2 = 2 * (t & 63);
    if (i2 < kend) {
#pragma unroll 4
      for (int c = t >> 6; c < kend; c += BP_WAVES)
        *reinterpret_cast<double2*>(Wl + i2 + c * BLD) = *reinterpret_cast<const double2*>(W + i2 + c * PB);
    }
  }
  __syncthreads();

  const double kss = kernel_value<KID>(0.0, ks);
  for (int64_t tile = first + wave; tile < tiles; tile += step) {
    const int64_t j = tile * BATCH_PREDICT_TILE + lc;
    const double* xs = Xs + (j < ns ? j : ns - 1) * d;   // a column past the count repeats the last point and is not stored
    // lr as this turn's own value: what hangs on it (32 row pointers, 32 alphas, the operand addresses) is formed where it is used, not
    // kept in 130 registers across the turns -- the registers are K*'s
    int lr = lr0;
    asm volatile("" : "+v"(lr));
    double kst[32];
    double mu = 0.0, ss = 0.0;
#pragma unroll
    for (int I = 0; I < 8; ++I) {
      if (I < nblk) {                                     // uniform over the workgroup
        // ---- entries 4 I .. 4 I + 3 of the lane's column of K*: k = 16 I + 4 u + lr
        const double* xk[4];
        double s[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = 16 * I + 4 * u + lr;
          xk[u] = X + (int64_t)(k < nb ? k : nb - 1) * d;
          s[u] = 0.0;
        }
        for (int64_t r = 0; r < d; ++r) {
          const double xr = xs[r];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            double df;
            if constexpr (ARD) df = bt_scaled_diff(xk[u][r], xr, ks.p[r]);
            else df = xk[u][r] - xr;
            s[u] = fma(df, df, s[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = 16 * I + 4 * u + lr;
          const double v = k < nb ? kernel_value<KID>(s[u], ks) : 0.0;
          kst[4 * I + u] = v;
          mu = fma(v, av[k], mu);
        }
        // ---- row block I of V = W K*: k up to the end of block I
        if (var) {
          v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int m = 0; m < 4 * (I + 1); ++m) {
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Wl[(16 * I + lc) + (4 * m + lr) * BLD], kst[m], acc, 0, 0, 0);
          }
#pragma unroll
          for (int g = 0; g < 4; ++g) ss = fma(acc[g], acc[g], ss);
        }
      }
    }
    mu += __shfl_xor(mu, 16, 64);
    mu += __shfl_xor(mu, 32, 64);
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);
    if (lr == 0 && j < ns) {
      if (mean) mean[j] = mu;
      if (var) var[j] = kss - ss;
    }
  }
}

}  // namespace

int launch_batch_predict(hipStream_t s, int kernel, const BatchPredictArgs& a, int64_t models, int split) {
  GPRC_TRY(check_grad_kernel("batch_predict", kernel));
  if (models < 1 || models > 65535 || split < 1 || split > 65535 || !a.X || !a.prm || !a.alpha || !a.W || !a.info || !a.Xs || (!a.mean && !a.var) ||
      a.d < 1 || a.ns_max < 1 || a.ld_out < a.ns_max || a.np_store < a.n_params || a.np_store > MAX_PARAMS || a.n_params < 1) {
    set_error("batch_predict: bad launch arguments");
    return GPRC_ERR_ARG;
  }
  int rc = 0;
  hipError_t e = hipSuccess;
  with_gradient_kernel(kernel, [&](auto kid) {
    constexpr int KID = decltype(kid)::value;
    rc = ensure_dynamic_lds<batch_predict_kernel<KID>>(BP_SMEM_BYTES);
    if (rc != 0) return;
    hipLaunchKernelGGL((batch_predict_kernel<KID>), dim3((unsigned)split, (unsigned)models), dim3(BP_THREADS), BP_SMEM_BYTES, s, a);
    e = hipGetLastError();
  });
  GPRC_TRY(rc);
  GPRC_HIP(e);
  return 0;
}

}  // namespace gprc
