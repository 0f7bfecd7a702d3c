// gprc_batch.hip -- small GPs in batches ("Small models in batches"): the host side of gprc_gpr_batch_logp_grad.
// The argument checks, one record of derived constants per model (make_deriv_spec, once per model), the staging of host arrays, the
// launches of kernels_batch.hip -- at most GPRC_BATCH_LAUNCH models each, on one set of scratch slabs from the context's pool -- and the
// tail every exact gradient has: the sums that the device leaves get 1/2 and the factors of cross_grad_finish, a model that is not
// positive definite gets NaN.  A model's record, its launch and its tail do not look at any other model: its bits do not depend on the batch.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "gprc_host.h"
#include "pair_tile.h"

using namespace gprc;

static_assert(GPRC_BATCH_MAX_N == NBI, "a batched model is one LDS-resident diagonal block");

namespace {

int bad(const std::string& msg) { set_error("batch_logp_grad: " + msg); return GPRC_ERR_ARG; }

}  // namespace

extern "C" {

int gprc_gpr_batch_logp_grad(gprc_ctx* ctx, int kernel, int64_t B, const double* params, int n_params, int64_t ld_params, const double* noise,
                             const double* X, int64_t d, int64_t n_max, int64_t x_stride, const double* y, int64_t y_stride, const int64_t* n_each,
                             double* logp_out, double* grad_out, double* alpha_out, int* info_out) {
  if (!ctx) return bad("null context");
  GPRC_TRY(check_grad_kernel("batch_logp_grad", kernel));
  if (B < 0) return bad("B < 0");
  if (B == 0) return 0;
  if (n_max > GPRC_BATCH_MAX_N)
    return bad("n_max = " + std::to_string(n_max) + " > " + std::to_string(GPRC_BATCH_MAX_N) +
               ": a batched model is at most 128 points, use the single-model entry points (gprc_gpr_logp_grad) for larger ones");
  if (n_max < 1 || d < 1) return bad("n_max < 1 or d < 1");
  if (!params || !noise || !X || !y) return bad("null input pointer (params, noise, X, y)");
  if (!logp_out || !info_out) return bad("null output pointer (logp_out, info_out)");
  if (n_params < 1 || ld_params < n_params) return bad("n_params < 1 or ld_params < n_params");
  if (x_stride != 0 && x_stride < d * n_max) return bad("x_stride must be 0 (shared) or >= d * n_max");
  if (y_stride != 0 && y_stride < n_max) return bad("y_stride must be 0 (shared) or >= n_max");
  for (int64_t b = 0; b < B; ++b) {
    if (!(noise[b] >= 0.0) || !std::isfinite(noise[b])) return bad("noise of model " + std::to_string(b) + " must be finite and >= 0");
    if (n_each && (n_each[b] < 1 || n_each[b] > n_max)) return bad("n_each of model " + std::to_string(b) + " is outside 1 .. n_max");
  }
  // one record per model: the derived constants, the noise, n_b
  const int np_store = std::max(n_params, 4);   // gammaexp's derived constants are p[2], p[3]
  const int prm_stride = np_store + 2, out_stride = n_params + 2;
  std::vector<double> hprm((size_t)(B * prm_stride));
  std::vector<KernelSpec> specs;
  if (grad_out) specs.resize((size_t)B);
  {
    KernelSpec ks;
    for (int64_t b = 0; b < B; ++b) {
      GPRC_TRY(make_spec(kernel, params + b * ld_params, n_params, d, &ks));
      if (grad_out) specs[(size_t)b] = ks;
      const KernelSpec g = make_deriv_spec(ks);
      double* r = hprm.data() + b * prm_stride;
      for (int k = 0; k < np_store; ++k) r[k] = g.p[k];
      r[np_store] = noise[b];
      r[np_store + 1] = (double)(n_each ? n_each[b] : n_max);
    }
  }
  GPRC_TRY(use_device(ctx));
  hipStream_t s = ctx->stream;
  In xin, yin;
  GPRC_TRY(xin.set(s, X, (x_stride ? (B - 1) * x_stride : 0) + d * n_max));
  GPRC_TRY(yin.set(s, y, (y_stride ? (B - 1) * y_stride : 0) + n_max));
  const int64_t launch = std::min<int64_t>(B, GPRC_BATCH_LAUNCH);
  DevMem prm, out, alpha, info, slab;
  GPRC_TRY(prm.alloc(B * prm_stride));
  GPRC_TRY(out.alloc(B * out_stride));
  GPRC_TRY(alpha.alloc(B * NBI));
  GPRC_TRY(info.alloc((B + 1) / 2));
  if (int rc = slab.alloc((int64_t)batch_scratch_doubles(launch))) {
    if (rc == GPRC_ERR_NOMEM)
      set_error("batch_logp_grad: the factors of one launch, " + std::to_string((batch_scratch_doubles(launch) * sizeof(double)) >> 20) +
                " MiB of device memory, could not be allocated");
    return rc;
  }
  GPRC_HIP(hipMemcpyAsync(prm.p, hprm.data(), sizeof(double) * hprm.size(), hipMemcpyHostToDevice, s));
  GPRC_HIP(hipMemsetAsync(info.p, 0, sizeof(int) * (size_t)B, s));
  BatchArgs a{xin.dev, yin.dev, prm.p, slab.p, out.p, alpha.p, reinterpret_cast<int*>(info.p), x_stride, y_stride, d, 0,
              prm_stride, np_store, n_params, out_stride, grad_out ? 1 : 0};
  for (int64_t b0 = 0; b0 < B; b0 += launch) {
    a.b0 = b0;
    GPRC_TRY(launch_batch_logp_grad(s, kernel, a, std::min<int64_t>(launch, B - b0)));
  }
  std::vector<double> hout((size_t)(B * out_stride)), halpha(alpha_out ? (size_t)(B * NBI) : 0);
  GPRC_HIP(hipMemcpyAsync(hout.data(), out.p, sizeof(double) * hout.size(), hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipMemcpyAsync(info_out, info.p, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, s));
  if (alpha_out) GPRC_HIP(hipMemcpyAsync(halpha.data(), alpha.p, sizeof(double) * halpha.size(), hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipStreamSynchronize(s));
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  std::vector<long double> acc((size_t)n_params);
  for (int64_t b = 0; b < B; ++b) {
    const double* r = hout.data() + b * out_stride;
    const bool ok = info_out[b] == 0;
    logp_out[b] = ok ? r[0] : qnan;
    if (grad_out) {
      double* g = grad_out + b * (n_params + 1);
      if (ok) {
        for (int k = 0; k < n_params; ++k) acc[(size_t)k] = 0.5L * (long double)r[1 + k];
        cross_grad_finish(specs[(size_t)b], acc.data(), g);
        g[n_params] = (double)(0.5L * (long double)r[1 + n_params]);
      } else {
        for (int k = 0; k <= n_params; ++k) g[k] = qnan;
      }
    }
    if (alpha_out) {
      const int64_t nb = n_each ? n_each[b] : n_max;
      for (int64_t i = 0; i < n_max; ++i) alpha_out[b * n_max + i] = ok ? halpha[(size_t)(b * NBI + i)] : (i < nb ? qnan : 0.0);
    }
  }
  return 0;
}

}  // extern "C"
