// kernels_batch_gpc.hip -- small Laplace classifiers in batches for gfx950 (gprc_gpc_batch_fit; DESIGN.md section 7, "Batched and local
// GPC"): the Newton / IRLS mode search of gpc_mode_search (gprc_model.hip, flags = 0; R/GPCclass.R:73-102) of one model of n_b <= 128
// points PER WORKGROUP, B models in one launch, the whole loop without leaving the CU and without the host.
//
// Workgroup b (512 threads: the factor body wants eight waves) runs
//   load     its record of the parameter array (the constants of make_deriv_spec, an unused slot where the regression record keeps the
//            noise, n_b) into a KernelSpec in LDS; y, zero from n_b on; f = 0;
//   fill     K, WITHOUT a noise term, whole and symmetric into the workgroup's 128^2 slab in device memory (L2-resident; the LDS cannot
//            hold K beside the image of B): kernel_value<KID> of the squared distance of the pair (larger index first), ARD coordinates
//            scaled by bt_scaled_diff (small_model.h's sqdist, the one every small model takes); rows and columns >= n_b are zero;
//   loop     it = 1, 2, ...:  pi = sigmoid(f), W = pi (1 - pi), sw = sqrt(W), b = W f + (y + 1) / 2 - pi  (zero from n_b on);
//            the image S = I + (sw_i sw_j) K_ij (lower triangle, zero above, the identity from n_b on); potf2_blocked_body<8, false>
//            (preloaded; nothing is stored: L stays in the lower triangle of the image, W_B = L^-1 transposed above it, its diagonal in
//            the side array); t = K b; u = sw o t; z = W_B u; v = W_B^T z (the two triangular solves as products with the explicit
//            inverse: small_model.h's winv_forward and winv_transposed); a = b - sw o v; f = K a;
//            objective = -1/2 a.f - sum log(1 + exp(-y_i f_i)).  Thread 0 forms the objective and the verdict -- converged (it > 1 and
//            |objective - last| < epsilon), a non-positive pivot (the model's info word, read back past L1), a non-finite objective,
//            the cap (it = max_iter), or go on -- and writes both to LDS; after the barrier every thread reads the same bits and the
//            whole workgroup leaves the loop at that one place or not at all: there is no other exit and no barrier inside a branch;
//   final    pi, sw and g = (y + 1) / 2 - pi at the last f, one more factorisation of B (R/GPCclass.R:99-102),
//            logq = objective - sum log L_ii;  g goes to the alpha slot, Wt[k][i] = W_B[k][i] sw_i to the model's 128^2 slot in
//            BatchArgs::w's layout (column-major, zero above the diagonal and, sw being zero there, in rows and columns >= n_b): with
//            these two kernels_batch_predict.hip computes fs_bar = k*^T g and Vfs = k** - |L^-1 (sw o k*)|^2 unchanged.
// info: 0 converged; k > 0 the first non-positive pivot, 1-based (B has eigenvalues >= 1: only non-finite input gives one);
// GPRC_BATCH_GPC_MAXITER the cap; GPRC_BATCH_GPC_NONFINITE the objective.  A flagged model stops at once, is not retried, and gets NaN
// for logq, f_hat and g; it disturbs nobody.  The caller zeroes the info words.  The body's compare-and-swap only replaces a zero, and the
// first flagged factorisation ends the loop, so the word cannot carry a flag from one factorisation into a later verdict; the final
// factorisation of a model that left the loop flagged finds the word taken and leaves it.
//
// LDS: the factor body's PB_SMEM_BYTES = 152 576 B, then GC_EXTRA doubles (y, f, sw, b, u, z, a, the control words and wave partials,
// the KernelSpec): 161 864 B of the 163 840 B a workgroup may have, one workgroup per CU.  The four partial sums per row of a product
// with K live in the body's two 16 x 16 buffers (512 doubles), which are free between its calls.  The coordinates are never staged.
//
// Order of summation, fixed and a function of (n_b, d, kernel) alone -- a model's bits do not depend on its place in the batch, on the
// batch (how long the others iterate included), on strides, or on which outputs are asked for:
//   squared distance   coordinates ascending, one fma chain
//   (K v)_i            thread (i, q), q < 4: j = q, q + 4, ... < n_b in one fma chain; (q0 + q1) + (q2 + q3)
//   z_k                thread (k, q), q < 4: i = q, q + 4, ... < k in one fma chain; (q0 + q1) + (q2 + q3); last fma(W_kk, u_k, .)
//   v_i                thread (i, q): k = i + 1 + q, i + 5 + q, ... < n_b in one fma chain; the same tree; last fma(W_ii, z_i, .)
//   a.f, sum log(1 + exp(-y f)), sum log L_ii    entry t to thread t < 128; each of the two waves by wave_sum; wave 0 + wave 1
// No atomics on memory except the factor body's one compare-and-swap on the model's info word (and the load that reads it back); no
// register spills: the scratch the compiler reports is the frame of the call into the factor body (profiles/batch_gpc_isa.txt).
#include "small_model.h"

namespace gprc {

namespace {

constexpr int GC_CTL = 8;                                    // objective, verdict, 2 x 2 wave partials
constexpr int GC_EXTRA = 7 * PB + GC_CTL + SPEC_DOUBLES;  // y, f, sw, b, u, z, a; control; the spec
constexpr size_t GC_SMEM_BYTES = PB_SMEM_BYTES + sizeof(double) * GC_EXTRA;
static_assert(GC_SMEM_BYTES <= 163840, "the batched classifier's LDS must fit a workgroup's 160 KiB");
static_assert(4 * PB <= 512, "the partial sums of a product with K live in the factor body's two 16 x 16 buffers");
constexpr int GC_CONTINUE = -1000;                           // the verdict that keeps the loop going: no info code

__device__ __forceinline__ double gc_sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }   // R/GPCclass.R:63

// part[q][i] = sum over j = q, q + 4, ... < nb of K[i][j] v[j]: a wave reads 64 consecutive rows of one column of the slab
__device__ __forceinline__ void gc_kv_partials(const double* K, const double* v, int nb, double* part, int t) {
  const int i = t & (PB - 1), q = t >> 7;
  double acc = 0.0;
  if (i < nb)
    for (int j = q; j < nb; j += 4) acc = fma(K[i + j * PB], v[j], acc);
  part[q * PB + i] = acc;
}

// the image of B = I + sw K sw the factor body works on: lower triangle, zero above, the identity from nb on
__device__ __forceinline__ void gc_image(double* S, const double* K, const double* sw, int nb, int t) {
  for (int e = t; e < PB * PB; e += 512) {
    const int i = e & (PB - 1), j = e >> 7;
    double v = 0.0;
    if (i >= j) {
      v = i == j ? 1.0 : 0.0;
      if (i < nb) v = fma(sw[i] * sw[j], K[e], v);
    }
    S[i + j * BLD] = v;
  }
}

// the model's info word as the factor body's compare-and-swap left it: read at the device's L2, not from this CU's L1
__device__ __forceinline__ int gc_read_info(int* info) { return __hip_atomic_load(info, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <int KID>
__global__ __launch_bounds__(512) void batch_gpc_fit_kernel(BatchGpcArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  constexpr bool ARD = is_ard(KID);
  double* S = sm;
  double* part = pb_work(sm);                   // 4 x PB: the body's Wd buffers between its calls
  const double* Wdiag = pb_wdiag(sm);
  double* yv = sm + PB_SMEM_DOUBLES;
  double* fv = yv + PB;
  double* swv = fv + PB;
  double* bv = swv + PB;                        // b; g in the final stage
  double* uv = bv + PB;                         // sw o (K b)
  double* zv = uv + PB;                         // W_B u
  double* av = zv + PB;                         // a
  double* ctl = av + PB;                        // [0] objective, [1] verdict, [2..3] and [4..5] the two waves' partial sums
  KernelSpec& ks = *reinterpret_cast<KernelSpec*>(ctl + GC_CTL);
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int64_t b = a.b0 + blockIdx.x;
  const double* prm = a.prm + b * a.prm_stride;
  const double* X = a.X + b * a.x_stride;
  const double* y = a.y + b * a.y_stride;
  double* K = a.slab + (int64_t)blockIdx.x * (PB * PB);
  int* info = a.info + b;
  const int nb = (int)prm[a.np_store + 1];
  const int64_t d = a.d;
  const double qnan = __builtin_nan("");

  // ---- load
  load_spec<KID>(ks, prm, a.np_store, a.n_params, t, 512);
  if (t < PB) { yv[t] = t < nb ? y[t] : 0.0; fv[t] = 0.0; }
  __syncthreads();

  // ---- fill: K whole into the slab, row i = e & 127, column e >> 7; the pair's larger index first, so K is symmetric to the bit
  for (int e = t; e < PB * PB; e += 512) {
    const int i = e & (PB - 1), j = e >> 7;
    double v = 0.0;
    if (i < nb && j < nb) v = kernel_value<KID>(sqdist<ARD>(X + (int64_t)(i > j ? i : j) * d, X + (int64_t)(i > j ? j : i) * d, d, ks.p), ks);
    K[e] = v;
  }
  __syncthreads();

  // ---- the mode search.  `verdict` and `objective` are read from LDS behind a barrier: uniform over the workgroup by construction
  int it = 0, verdict = GC_CONTINUE;
  double objective = 0.0, last = 0.0;
  for (;;) {
    ++it;
    if (t < PB) {                                           // R/GPCclass.R:78-81
      double sw = 0.0, bb = 0.0;
      if (t < nb) {
        const double f = fv[t], P = gc_sigmoid(f), W = (1.0 - P) * P;
        sw = sqrt(W);
        bb = W * f + (yv[t] + 1.0) / 2.0 - P;
      }
      swv[t] = sw;
      bv[t] = bb;
    }
    __syncthreads();
    gc_image(S, K, swv, nb, t);
    __syncthreads();
    potf2_blocked_body<8, false>(sm, nullptr, PB, nullptr, info, 0, nullptr, true);
    __syncthreads();
    gc_kv_partials(K, bv, nb, part, t);                     // K b
    __syncthreads();
    if (t < PB) uv[t] = swv[t] * sum4_pairs(part[t], part[PB + t], part[2 * PB + t], part[3 * PB + t]);
    __syncthreads();
    // z = W_B u  (:82);  v = W_B^T z  (:83),  a = b - sw o v  (:84)
    winv_forward(S, Wdiag, uv, nb, t, [zv](int k, double z) { zv[k] = z; });
    __syncthreads();
    winv_transposed(S, Wdiag, zv, nb, t, [=](int i, double v) { av[i] = i < nb ? bv[i] - swv[i] * v : 0.0; });
    __syncthreads();
    gc_kv_partials(K, av, nb, part, t);                     // f = K a  (:85)
    __syncthreads();
    {
      double af = 0.0, ll = 0.0;
      if (t < PB) {
        const double f = sum4_pairs(part[t], part[PB + t], part[2 * PB + t], part[3 * PB + t]);
        fv[t] = f;
        if (t < nb) { af = av[t] * f; ll = log(1.0 + exp(-yv[t] * f)); }
      }
      sum128<2>(af, ll, ctl, wave, lane);
    }
    __syncthreads();
    if (t == 0) {                                           // :86-90, and what ends a model early
      const double obj = -(ctl[2] + ctl[3]) / 2.0 - (ctl[4] + ctl[5]);
      const int pivot = gc_read_info(info);
      int v = GC_CONTINUE;
      if (pivot != 0) v = pivot;
      else if (!(fabs(obj) <= 1.79769313486231570815e308)) v = GPRC_BATCH_GPC_NONFINITE;
      else if (it > 1 && fabs(obj - last) < a.epsilon) v = 0;
      else if (it >= a.max_iter) v = GPRC_BATCH_GPC_MAXITER;
      ctl[0] = obj;
      ctl[1] = (double)v;
    }
    __syncthreads();
    objective = ctl[0];
    verdict = (int)ctl[1];
    last = objective;
    if (verdict != GC_CONTINUE) break;                      // every thread, here and nowhere else
  }

  // ---- final: g and sw at the last f, B factored once more (:99-102)
  if (t < PB) {
    double sw = 0.0, g = 0.0;
    if (t < nb) {
      const double P = gc_sigmoid(fv[t]);
      sw = sqrt(P * (1.0 - P));
      g = (yv[t] + 1.0) / 2.0 - P;
    }
    swv[t] = sw;
    bv[t] = g;
  }
  __syncthreads();
  gc_image(S, K, swv, nb, t);
  __syncthreads();
  potf2_blocked_body<8, false>(sm, nullptr, PB, nullptr, info, 0, nullptr, true);
  __syncthreads();
  {
    double lg = t < nb ? log(S[t + t * BLD]) : 0.0;
    sum128<2>(lg, ctl, wave, lane);
  }
  __syncthreads();
  if (t == 0) {
    const int code = verdict != 0 ? verdict : gc_read_info(info);
    a.logq[b] = code == 0 ? objective - (ctl[2] + ctl[3]) : qnan;
    if (a.iters) a.iters[b] = it;
    *info = code;
    ctl[1] = (double)code;
  }
  __syncthreads();
  const bool ok = (int)ctl[1] == 0;
  if (t < PB) {
    a.alpha[b * PB + t] = t < nb ? (ok ? bv[t] : qnan) : 0.0;
    a.fhat[b * PB + t] = t < nb ? (ok ? fv[t] : qnan) : 0.0;
  }
  {                                                         // Wt = W_B diag(sw): row k = t & 127, columns (t >> 7) + 4 c
    double* Wt = a.w + b * (int64_t)(PB * PB);
    const int k = t & (PB - 1), ty = t >> 7;
    const double wd = Wdiag[k];
    constexpr int BATCH = 8;
    for (int c0 = 0; c0 < PB / 4; c0 += BATCH) {
      double wv[BATCH];
#pragma unroll
      for (int u = 0; u < BATCH; ++u) {
        const int c = ty + 4 * (c0 + u);
        wv[u] = (k > c ? S[c + k * BLD] : (k == c ? wd : 0.0)) * swv[c];   // (pb_w, W[k][k] read once)
      }
#pragma unroll
      for (int u = 0; u < BATCH; ++u) Wt[k + (ty + 4 * (c0 + u)) * PB] = wv[u];
    }
  }
}

}  // namespace

size_t batch_gpc_scratch_doubles(int64_t models) { return (size_t)models * PB * PB; }

int launch_batch_gpc_fit(hipStream_t s, int kernel, const BatchGpcArgs& a, int64_t models) {
  GPRC_TRY(check_grad_kernel("gpc_batch_fit", kernel));
  if (models < 1 || models > GPRC_BATCH_LAUNCH || !a.X || !a.y || !a.prm || !a.slab || !a.logq || !a.alpha || !a.fhat || !a.w || !a.info ||
      a.d < 1 || a.np_store < a.n_params || a.np_store > MAX_PARAMS || a.n_params < 1 || !(a.epsilon > 0.0) || a.max_iter < 1 ||
      a.max_iter > GPRC_BATCH_GPC_MAX_ITER) {
    set_error("gpc_batch_fit: bad launch arguments");
    return GPRC_ERR_ARG;
  }
  int rc = 0;
  with_gradient_kernel(kernel, [&](auto kid) {
    rc = launch_with_lds<batch_gpc_fit_kernel<decltype(kid)::value>>("batch_gpc_fit_kernel", dim3((unsigned)models), dim3(512), GC_SMEM_BYTES, s, a);
  });
  return rc;
}

}  // namespace gprc
