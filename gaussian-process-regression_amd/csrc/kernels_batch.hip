// kernels_batch.hip -- small GPs in batches for gfx950 (gprc_gpr_batch_logp_grad; DESIGN.md section 7, "Small models in batches"): the log
// marginal likelihood, alpha and the exact evidence gradient of one model of n_b <= 128 points PER WORKGROUP, B models in one launch.
//
// Workgroup b (512 threads: the factor body wants eight waves) runs, back to back and without leaving its CU,
//   load     its record of the parameter array (the constants of make_deriv_spec, formed once per model by the host, then the noise and
//            n_b) into a KernelSpec in LDS; y, zero from n_b on;
//   fill     K_y = K + noise I straight into the LDS image potf2_blocked_body works on (leading dimension BLD): kernel_value<KID> of the
//            squared distance, ARD coordinates multiplied by 1 / l_k first, as in the contraction kernels; rows and columns >= n_b are
//            the identity (they add nothing to the log-determinant), everything above the diagonal is zero;
//   factor   potf2_blocked_body<8>(preloaded), unchanged: L and W = L^-1 go to the workgroup's slab in device memory (2 x 128^2 doubles;
//            BatchArgs::w set: W goes to w + b w_stride instead, the store of a fitted batch, and the slab is L's 128^2 alone),
//            info (first non-positive pivot, 1-based) to the model's own word; a bad model finishes its arithmetic and is only flagged;
//   solve    z = W y, alpha = W^T z, logp = -1/2 y.alpha - sum log L_ii - n_b / 2 log 2 pi;
//   gradient (when asked for) M = alpha alpha^T - W^T W, one 16 x 16 block of the lower triangle at a time on v_mfma_f64_16x16x4_f64: the
//            accumulator starts as alpha_i alpha_j and every MFMA subtracts (the negate bit); the contraction index runs from the block
//            row's first column on -- W is triangular -- and stops at the last 16-row block that holds points, so no block of structural
//            zeros is multiplied.  A block is consumed in the accumulator's lanes (col = lane & 15, row = (lane >> 4) + 4 reg) against
//            cross_weight<KID> of the pair's squared distance, as kernels_igrad.hip does, and never stored.  Pairs below the diagonal
//            count twice, the diagonal's integrands are zero (gammaexp's weight is 0 at s = 0) and its M_ii give d / d noise = 1/2 sum
//            M_ii.  The ARD kernels keep weight x h of a lane's pairs in registers and take a second pass over the coordinates.  What the
//            device leaves is the sum WITHOUT the factors that do not depend on (i, j): the host applies 1/2 and cross_grad_finish.
//
// LDS: the factor body's PB_SMEM_BYTES = 152 576 B, then BT_EXTRA doubles (y, z / the diagonal of M, alpha, the wave partials, ARD's sums,
// the KernelSpec): 160 784 B of the 163 840 B a workgroup may have, one workgroup per CU.  After the factorisation the image is NOT
// reused for staging: it still holds L (lower) and W^T (strictly upper, its diagonal in the side array), and the solves and the MFMA
// operands read W from there, not from the slab.  The coordinates are never staged: a model has at most 128 x d doubles of them and the
// fill, the contraction and ARD's second pass read them from memory through L1 / L2 (points >= n_b are never read, whatever the
// caller's padding holds).
//
// Order of summation, fixed and a function of (n_b, d, kernel) alone -- a model's bits do not depend on its place in the batch, on the
// batch, or on which outputs are asked for:
//   squared distance   coordinates ascending, one fma chain
//   z_k                thread (k, q), q < 4: i = q, q + 4, ... < k in one fma chain; (q0 + q1) + (q2 + q3); last fma(W_kk, y_k, .)
//   alpha_i            thread (i, q): k = i + 1 + q, i + 5 + q, ... < n_b in one fma chain; the same tree; last fma(W_ii, z_i, .)
//   y.alpha, sum log L_ii, sum M_ii    entry t to thread t < 128; each of the two waves by wave_sum; wave 0 + wave 1
//   M block            the MFMA's own chain over k ascending from alpha_i alpha_j
//   theta sums         block b of the lower triangle (by rows: (0,0) (1,0) (1,1) (2,0) ...) belongs to wave b mod 8; a lane's pairs in
//                      block order, register ascending, in one fma chain; the 64 lanes by wave_sum; the eight waves as
//                      ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7))  (ARD: the same per coordinate)
// No atomics except the factor body's one compare-and-swap on the model's info word; no register spills (the 8 bytes of scratch a lane that
// the compiler reports are the frame of the call into the factor body, which is not inlined: profiles/batch_isa.txt).
// The squared distance, the spec load, the image's entry rule, the two products with W and the 128-entry sums are small_model.h's, shared
// with the other kernels that run one small model per workgroup; what a pair adds to the theta sums is pair_tile.h's theta_terms.
#include "small_model.h"

namespace gprc {

namespace {

constexpr int BT_WAVES = 8;
constexpr int BT_MAXBLK = 5;                              // 36 blocks of the lower triangle over eight waves: at most five a wave
constexpr int BT_EXTRA = 3 * PB + BT_WAVES * PT_D + MAX_PARAMS + SPEC_DOUBLES;   // y, z, alpha; red; gacc; the spec
constexpr size_t BT_SMEM_BYTES = PB_SMEM_BYTES + sizeof(double) * BT_EXTRA;
static_assert(BT_SMEM_BYTES <= 163840, "the batch kernel's LDS must fit a workgroup's 160 KiB");

typedef double v4d __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double bt_sum8(const double* r, int stride) {
  return sum4_pairs(r[0], r[stride], r[2 * stride], r[3 * stride]) + sum4_pairs(r[4 * stride], r[5 * stride], r[6 * stride], r[7 * stride]);
}

template <int KID>
__global__ __launch_bounds__(512) void batch_logp_grad_kernel(BatchArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  constexpr bool ARD = is_ard(KID);
  double* S = sm;
  const double* Wdiag = pb_wdiag(sm);
  double* yv = sm + PB_SMEM_DOUBLES;
  double* zv = yv + PB;                 // z = W y, later the diagonal of M
  double* av = zv + PB;                 // alpha
  double* red = av + PB;                // BT_WAVES x PT_D
  double* gacc = red + BT_WAVES * PT_D; // ARD's sums per coordinate
  KernelSpec& ks = *reinterpret_cast<KernelSpec*>(gacc + MAX_PARAMS);
  const int t = threadIdx.x, lane = t & 63, lc = lane & 15, lr = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int64_t b = a.b0 + blockIdx.x;
  const double* prm = a.prm + b * a.prm_stride;
  const double* X = a.X + b * a.x_stride;
  const double* y = a.y + b * a.y_stride;
  double* out = a.out + b * a.out_stride;
  const double noise = prm[a.np_store];
  const int nb = (int)prm[a.np_store + 1];
  const int64_t d = a.d;

  // ---- load
  load_spec<KID>(ks, prm, a.np_store, a.n_params, t, 512);
  if (t < PB) yv[t] = t < nb ? y[t] : 0.0;
  __syncthreads();

  // ---- fill: row i = t & 127, columns (t >> 7) + 4 c
  for (int e = t; e < PB * PB; e += 512) {
    const int i = e & (PB - 1), j = e >> 7;
    S[i + j * BLD] = image_entry(i, j, nb, noise, [=, &ks] { return kernel_value<KID>(sqdist<ARD>(X + (int64_t)i * d, X + (int64_t)j * d, d, ks.p), ks); });
  }
  __syncthreads();

  // ---- factor and invert
  // L goes to the launch's scratch; W beside it, or (a.w: a fitted batch keeps it) to the model's own place in the caller's store
  double* slab = a.slab + (int64_t)blockIdx.x * (a.w ? PB * PB : 2 * PB * PB);
  potf2_blocked_body<8>(sm, slab, PB, a.w ? a.w + b * a.w_stride : slab + PB * PB, a.info + b, 0, nullptr, true);
  __syncthreads();

  // ---- solve
  winv_forward(S, Wdiag, yv, nb, t, [zv](int k, double z) { zv[k] = z; });
  __syncthreads();
  winv_transposed(S, Wdiag, zv, nb, t, [av, al_out = a.alpha + b * PB](int i, double al) {
    av[i] = al;
    al_out[i] = al;
  });
  __syncthreads();
  {
    double ya = 0.0, lg = 0.0;
    if (t < nb) { ya = yv[t] * av[t]; lg = log(S[t + t * BLD]); }
    sum128(ya, lg, red, wave, lane);
    __syncthreads();
    if (t == 0) out[0] = -0.5 * (red[0] + red[1]) - (red[2] + red[3]) - 0.5 * (double)nb * LOG_2PI;
  }
  if (!a.want_grad) return;
  __syncthreads();   // red is written again below

  // ---- gradient
  const int nblk = (nb + 15) >> 4, total = nblk * (nblk + 1) / 2, kend = 16 * nblk;
  double wh[BT_MAXBLK][4];   // ARD: twice M_ij h_ij of the lane's pairs
  int bi0[BT_MAXBLK], bj0[BT_MAXBLK];
  double a0 = 0.0, a1 = 0.0;
#pragma unroll
  for (int kb = 0; kb < BT_MAXBLK; ++kb) {
    const int bid = wave + BT_WAVES * kb;
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= bid) ++I;
    const int i0 = 16 * I, j0 = 16 * (bid - I * (I + 1) / 2);
    bi0[kb] = i0;
    bj0[kb] = j0;
#pragma unroll
    for (int g = 0; g < 4; ++g) wh[kb][g] = 0.0;
    if (bid < total) {   // wave-uniform
      v4d m;
#pragma unroll
      for (int g = 0; g < 4; ++g) m[g] = av[i0 + lr + 4 * g] * av[j0 + lc];
      for (int k0 = i0; k0 < kend; k0 += 4)
        m = __builtin_amdgcn_mfma_f64_16x16x4f64(pb_w(S, Wdiag, k0 + lr, i0 + lc), pb_w(S, Wdiag, k0 + lr, j0 + lc), m, 0, 0, 1);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int i = i0 + lr + 4 * g, j = j0 + lc;
        if (i == j && i < nb) zv[i] = m[g];
        if (i < nb && i > j) theta_terms<KID>(2.0 * m[g], sqdist<ARD>(X + (int64_t)i * d, X + (int64_t)j * d, d, ks.p), ks, a0, a1, wh[kb][g]);
      }
    }
  }

  const int np = a.n_params;
  if constexpr (ARD) {
    for (int64_t r0 = 0; r0 < d; r0 += PT_D) {
      const int dc = (int)((d - r0 < PT_D) ? (d - r0) : PT_D);
      for (int rr = 0; rr < dc; ++rr) {
        const int64_t r = r0 + rr;
        const double pr = ks.p[r];
        double acc = 0.0;
#pragma unroll
        for (int kb = 0; kb < BT_MAXBLK; ++kb) {
          if (wave + BT_WAVES * kb < total) {
            const int j = bj0[kb] + lc;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const int i = bi0[kb] + lr + 4 * g;
              if (i < nb && i > j) {
                const double df = bt_scaled_diff(X[(int64_t)i * d + r], X[(int64_t)j * d + r], pr);
                acc = fma(wh[kb][g], df * df, acc);
              }
            }
          }
        }
        const double v = wave_sum(acc);
        if (lane == 0) red[wave * PT_D + rr] = v;
      }
      __syncthreads();
      if (t < dc) gacc[r0 + t] = bt_sum8(red + t, PT_D);
      __syncthreads();
    }
    for (int k = t; k < np; k += 512) out[1 + k] = gacc[k];
  } else {
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
    if (lane == 0) { red[wave * PT_D] = a0; red[wave * PT_D + 1] = a1; }
    __syncthreads();
    if (t < np) out[1 + t] = bt_sum8(red + t, PT_D);
    __syncthreads();
  }

  // ---- d / d noise: the diagonal of M (the barriers above stand between its writes and these reads)
  {
    double dm = t < nb ? zv[t] : 0.0;
    sum128(dm, red, wave, lane);
    __syncthreads();
    if (t == 0) out[1 + np] = red[0] + red[1];
  }
}

}  // namespace

size_t batch_scratch_doubles(int64_t models, bool keep_w) { return (size_t)models * (keep_w ? 1 : 2) * PB * PB; }

int launch_batch_logp_grad(hipStream_t s, int kernel, const BatchArgs& a, int64_t models) {
  GPRC_TRY(check_grad_kernel("batch_logp_grad", kernel));
  if (models < 1 || models > GPRC_BATCH_LAUNCH || !a.X || !a.y || !a.prm || !a.slab || !a.out || !a.alpha || !a.info || a.d < 1 ||
      a.np_store < a.n_params || a.np_store > MAX_PARAMS || a.n_params < 1) {
    set_error("batch_logp_grad: bad launch arguments");
    return GPRC_ERR_ARG;
  }
  int rc = 0;
  with_gradient_kernel(kernel, [&](auto kid) {
    rc = launch_with_lds<batch_logp_grad_kernel<decltype(kid)::value>>("batch_logp_grad_kernel", dim3((unsigned)models), dim3(512), BT_SMEM_BYTES, s, a);
  });
  return rc;
}

}  // namespace gprc
