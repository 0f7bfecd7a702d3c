// gprc_batch.hip -- small GPs in batches ("Small models in batches" and "Batched predict"): the host side of
// gprc_gpr_batch_logp_grad, gprc_gpr_batch_fit, gprc_gpr_batch_predict, gprc_gpr_batch_predict_grad and gprc_gpr_batch_loo, and
// ("Batched and local GPC") of the classifier batch: gprc_gpc_batch_fit (kernels_batch_gpc.hip) and its predictions, which are the
// regression batch's predict launch on what that fit stores.
// The argument checks, one record of derived constants per model (make_deriv_spec, once per model), the staging of host arrays, the
// launches of kernels_batch.hip -- at most GPRC_BATCH_LAUNCH models each, on one set of scratch slabs from the context's pool -- and the
// tail every exact gradient has (half_theta_grad, gprc_host.h): the sums that the device leaves get 1/2 and the factors of
// cross_grad_finish, a model that is not positive definite gets NaN.  A model's record, its launch and its tail do not look at any other
// model: its bits do not depend on the batch.
// The two fitting entry points share every step up to the launches (batch_checks, batch_records, batch_launches): the fitted batch differs
// only in where the buffers live -- the gprc_batch_model owns them -- and in where the kernel puts W = L^-1 (BatchArgs::w).
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "gprc_host.h"
#include "pair_tile.h"

using namespace gprc;

static_assert(GPRC_BATCH_MAX_N == NBI, "a batched model is one LDS-resident diagonal block");

// A fitted batch: what gprc_gpr_batch_predict, _predict_grad and _loo read again, all in device memory from the context's pool.
enum BatchKind { BATCH_GPR = 0, BATCH_GPC = 1 };
struct gprc_batch_model : Bound {
  int kind = BATCH_GPR;
  int kernel = 0, n_params = 0, np_store = 0, prm_stride = 0;
  int64_t B = 0, d = 0, n_max = 0, x_stride = 0, y_stride = 0;
  bool uneven = false;   // fitted with n_each: a model may have fewer than n_max points
  DevMem X;       // the points: d * n_max doubles (shared) or B strides of the caller's x_stride
  DevMem y;       // the targets: n_max doubles (shared) or B strides of the caller's y_stride (gprc_gpr_batch_loo reads them)
  DevMem alpha;   // B x 128, zero from n_b on (BATCH_GPC: g = (y + 1) / 2 - pi at the mode)
  DevMem W;       // B x 128^2: L^-1 of every model (BatchArgs::w; BATCH_GPC: L^-1 diag(sw) of B = I + sw K sw)
  DevMem fhat;    // BATCH_GPC: B x 128, the modes
  DevMem prm;     // B records: the derived constants, the noise (BATCH_GPC: unused, 0), n_b
  DevMem info;    // B ints
};

namespace {

// the checks the fitting entry points make, in one order; *empty: B = 0, nothing to do.  classifier: there is no noise, and the context is
// looked at LAST, so that an argument error is reported whether or not a device is there
int batch_checks(const char* who, gprc_ctx* ctx, int kernel, int64_t B, const double* params, int n_params, int64_t ld_params, const double* noise,
                 const double* X, int64_t d, int64_t n_max, int64_t x_stride, const double* y, int64_t y_stride, const int64_t* n_each,
                 const void* out0, const double* logp_out, const int* info_out, const char* outputs, bool* empty, bool classifier = false) {
  *empty = false;
  if (!ctx && !classifier) return bad(who, "null context");
  GPRC_TRY(check_grad_kernel(who, kernel));
  if (B < 0) return bad(who, "B < 0");
  if (B == 0) { *empty = true; return ctx ? 0 : bad(who, "null context"); }
  if (n_max > GPRC_BATCH_MAX_N)
    return bad(who, "n_max = " + std::to_string(n_max) + " > " + std::to_string(GPRC_BATCH_MAX_N) +
                        ": a batched model is at most 128 points, use the single-model entry points (gprc_gpr_logp_grad) for larger ones");
  if (n_max < 1 || d < 1) return bad(who, "n_max < 1 or d < 1");
  if (!params || (!noise && !classifier) || !X || !y) return bad(who, classifier ? "null input pointer (params, X, y)" : "null input pointer (params, noise, X, y)");
  if (!out0 || !logp_out || !info_out) return bad(who, std::string("null output pointer (") + outputs + ")");
  if (n_params < 1 || ld_params < n_params) return bad(who, "n_params < 1 or ld_params < n_params");
  if (x_stride != 0 && x_stride < d * n_max) return bad(who, "x_stride must be 0 (shared) or >= d * n_max");
  if (y_stride != 0 && y_stride < n_max) return bad(who, "y_stride must be 0 (shared) or >= n_max");
  for (int64_t b = 0; b < B; ++b) {
    if (!classifier && (!(noise[b] >= 0.0) || !std::isfinite(noise[b]))) return bad(who, "noise of model " + std::to_string(b) + " must be finite and >= 0");
    if (n_each && (n_each[b] < 1 || n_each[b] > n_max)) return bad(who, "n_each of model " + std::to_string(b) + " is outside 1 .. n_max");
  }
  if (!ctx) return bad(who, "null context");
  return 0;
}

// one record per model: the derived constants, the noise (null: 0), n_b
struct BatchRecords {
  int np_store = 0, prm_stride = 0, out_stride = 0;
  std::vector<double> hprm;
  std::vector<KernelSpec> specs;   // the callers' specs, kept for the gradient's tail
};

int batch_records(int kernel, int64_t B, const double* params, int n_params, int64_t ld_params, const double* noise, int64_t d, int64_t n_max,
                  const int64_t* n_each, bool keep_specs, BatchRecords* r) {
  r->np_store = std::max(n_params, 4);   // gammaexp's derived constants are p[2], p[3]
  r->prm_stride = r->np_store + 2;
  r->out_stride = n_params + 2;
  r->hprm.resize((size_t)(B * r->prm_stride));
  if (keep_specs) r->specs.resize((size_t)B);
  KernelSpec ks;
  for (int64_t b = 0; b < B; ++b) {
    GPRC_TRY(make_spec(kernel, params + b * ld_params, n_params, d, &ks));
    if (keep_specs) r->specs[(size_t)b] = ks;
    const KernelSpec g = make_deriv_spec(ks);
    double* rec = r->hprm.data() + b * r->prm_stride;
    for (int k = 0; k < r->np_store; ++k) rec[k] = g.p[k];
    rec[r->np_store] = noise ? noise[b] : 0.0;
    rec[r->np_store + 1] = (double)(n_each ? n_each[b] : n_max);
  }
  return 0;
}

// the records to the device, the info words zeroed, then the launches: at most GPRC_BATCH_LAUNCH models each on one set of slabs.
// prm, out, alpha, info: allocated here (the caller owns them); w: null, or the fitted batch's store of B x 128^2 doubles
int batch_launches(const char* who, hipStream_t s, int kernel, int64_t B, const BatchRecords& r, int n_params, const double* xdev, int64_t x_stride,
                   const double* ydev, int64_t y_stride, int64_t d, bool want_grad, double* w, DevMem& prm, DevMem& out, DevMem& alpha, DevMem& info) {
  const int64_t launch = std::min<int64_t>(B, GPRC_BATCH_LAUNCH);
  DevMem slab;
  GPRC_TRY(prm.alloc(B * r.prm_stride));
  GPRC_TRY(out.alloc(B * r.out_stride));
  GPRC_TRY(alpha.alloc(B * NBI));
  GPRC_TRY(info.alloc((B + 1) / 2));
  const size_t slab_doubles = batch_scratch_doubles(launch, w != nullptr);
  if (int rc = slab.alloc((int64_t)slab_doubles)) {
    if (rc == GPRC_ERR_NOMEM)
      set_error(std::string(who) + ": the factors of one launch, " + std::to_string((slab_doubles * sizeof(double)) >> 20) +
                " MiB of device memory, could not be allocated");
    return rc;
  }
  GPRC_HIP(hipMemcpyAsync(prm.p, r.hprm.data(), sizeof(double) * r.hprm.size(), hipMemcpyHostToDevice, s));
  GPRC_HIP(hipMemsetAsync(info.p, 0, sizeof(int) * (size_t)B, s));
  BatchArgs a{xdev, ydev, prm.p, slab.p, out.p, alpha.p, reinterpret_cast<int*>(info.p), x_stride, y_stride, d, 0,
              r.prm_stride, r.np_store, n_params, r.out_stride, want_grad ? 1 : 0};
  a.w = w;
  a.w_stride = (int64_t)NBI * NBI;
  for (int64_t b0 = 0; b0 < B; b0 += launch) {
    a.b0 = b0;
    GPRC_TRY(launch_batch_logp_grad(s, kernel, a, std::min<int64_t>(launch, B - b0)));
  }
  return 0;
}

// a row of alpha_out: the model's alpha; NaN for a flagged model's points, zero behind n_b
void expand_alpha(const double* alpha_b, bool ok, int64_t nb, int64_t n_max, double* row) {
  for (int64_t i = 0; i < n_max; ++i) row[i] = ok ? alpha_b[i] : (i < nb ? std::numeric_limits<double>::quiet_NaN() : 0.0);
}

// a regression call on a classifier batch, or the other way round
int batch_kind(const char* who, const gprc_batch_model& m, int kind) {
  if (m.kind == kind) return 0;
  return bad(who, kind == BATCH_GPC ? "the batch is a regression batch (gprc_gpr_batch_fit): use the gprc_gpr_batch_* calls"
                                    : "the batch is a classifier batch (gprc_gpc_batch_fit): use the gprc_gpc_batch_* calls");
}

// gprc_gpr_batch_predict, gprc_gpr_batch_predict_grad and gprc_gpc_batch_predict_latent: one set of checks, one staging, one split rule; grad: the gradient entry point
int batch_predict_any(const char* who, bool grad, int kind, gprc_batch_model* m, const double* X_star, int64_t ns_max, int64_t xs_stride, const int64_t* ns_each,
                      double* mean_out, double* var_out, int64_t ld_out, double* dmean_out, double* dvar_out, int64_t ld_grad) {
  if (!m) return bad(who, "null model");
  GPRC_TRY(ctx_gone(who, *m));
  GPRC_TRY(batch_kind(who, *m, kind));
  if (!X_star) return bad(who, "null input pointer (X_star)");
  if (!grad && !mean_out && !var_out) return bad(who, "null output pointers (mean_out and var_out: one of them may be NULL, not both)");
  if (grad && !mean_out && !var_out && !dmean_out && !dvar_out)
    return bad(who, "null output pointers (mean_out, var_out, dmean_out, dvar_out: not all four may be NULL)");
  if (ns_max < 1) return bad(who, "ns_max < 1");
  if (xs_stride != 0 && xs_stride < m->d * ns_max) return bad(who, "xs_stride must be 0 (shared) or >= d * ns_max");
  if (ld_out < ns_max) return bad(who, "ld_out < ns_max");
  if ((dmean_out || dvar_out) && ld_grad < m->d * ns_max) return bad(who, "ld_grad < d * ns_max");
  const int64_t B = m->B;
  if (ns_each)
    for (int64_t b = 0; b < B; ++b)
      if (ns_each[b] < 1 || ns_each[b] > ns_max) return bad(who, "ns_each of model " + std::to_string(b) + " is outside 1 .. ns_max");
  gprc_ctx* ctx = m->ctx;
  GPRC_TRY(use_device(ctx));
  hipStream_t s = ctx->stream;
  In xs;
  GPRC_TRY(xs.set(s, X_star, (xs_stride ? (B - 1) * xs_stride : 0) + m->d * ns_max));
  DevMem counts;
  if (ns_each) {
    static_assert(sizeof(int64_t) == sizeof(double), "the counts travel in a block of doubles");
    GPRC_TRY(counts.alloc(B));
    GPRC_HIP(hipMemcpyAsync(counts.p, ns_each, sizeof(int64_t) * (size_t)B, hipMemcpyHostToDevice, s));
  }
  // A host output goes through a temporary of the same pitch.  Where the launch does not write every entry of it -- counts, or a pitch
  // beyond ns_max -- the temporary starts as the caller's array: what lies behind a model's count comes back as it was.
  const int64_t out_count = (B - 1) * ld_out + ns_max;
  const bool gaps = ns_each != nullptr || (ld_out > ns_max && B > 1);
  const int64_t grad_count = (B - 1) * ld_grad + m->d * ns_max;
  const bool grad_gaps = ns_each != nullptr || (ld_grad > m->d * ns_max && B > 1);
  Out mean, var, dmean, dvar;
  GPRC_TRY(mean.set_keeping(mean_out, out_count, gaps, s));
  GPRC_TRY(var.set_keeping(var_out, out_count, gaps, s));
  GPRC_TRY(dmean.set_keeping(dmean_out, grad_count, grad_gaps, s));
  GPRC_TRY(dvar.set_keeping(dvar_out, grad_count, grad_gaps, s));
  // the split: whole turns of a workgroup (BATCH_PREDICT_WAVES tiles) over enough workgroups for every CU, when the batch alone has fewer
  int cus = 0;
  GPRC_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  const int64_t tiles = (ns_max + BATCH_PREDICT_TILE - 1) / BATCH_PREDICT_TILE;
  const int64_t turns = (tiles + BATCH_PREDICT_WAVES - 1) / BATCH_PREDICT_WAVES;
  const int split = (int)std::min<int64_t>(std::min<int64_t>(turns, 65535), std::max<int64_t>(1, (cus + B - 1) / B));
  BatchPredictArgs a{m->X.p, m->prm.p, m->alpha.p, m->W.p, reinterpret_cast<const int*>(m->info.p), xs.dev,
                     ns_each ? reinterpret_cast<const int64_t*>(counts.p) : nullptr, mean.dev, var.dev, m->x_stride, xs_stride, m->d, ns_max, ld_out, 0,
                     m->prm_stride, m->np_store, m->n_params, dmean.dev, dvar.dev, ld_grad};
  constexpr int64_t GRID_Y = 65535;
  for (int64_t b0 = 0; b0 < B; b0 += GRID_Y) {
    a.b0 = b0;
    GPRC_TRY((grad ? launch_batch_predict_grad : launch_batch_predict)(s, m->kernel, a, std::min<int64_t>(GRID_Y, B - b0), split));
  }
  return finish_sync(s, mean, var, dmean, dvar);
}

}  // namespace

extern "C" {

int gprc_gpr_batch_logp_grad(gprc_ctx* ctx, int kernel, int64_t B, const double* params, int n_params, int64_t ld_params, const double* noise,
                             const double* X, int64_t d, int64_t n_max, int64_t x_stride, const double* y, int64_t y_stride, const int64_t* n_each,
                             double* logp_out, double* grad_out, double* alpha_out, int* info_out) {
  const char* who = "batch_logp_grad";
  bool empty = false;
  GPRC_TRY(batch_checks(who, ctx, kernel, B, params, n_params, ld_params, noise, X, d, n_max, x_stride, y, y_stride, n_each, logp_out, logp_out,
                        info_out, "logp_out, info_out", &empty));
  if (empty) return 0;
  BatchRecords r;
  GPRC_TRY(batch_records(kernel, B, params, n_params, ld_params, noise, d, n_max, n_each, grad_out != nullptr, &r));
  const std::vector<KernelSpec>& specs = r.specs;
  const int out_stride = r.out_stride;
  GPRC_TRY(use_device(ctx));
  hipStream_t s = ctx->stream;
  In xin, yin;
  GPRC_TRY(xin.set(s, X, (x_stride ? (B - 1) * x_stride : 0) + d * n_max));
  GPRC_TRY(yin.set(s, y, (y_stride ? (B - 1) * y_stride : 0) + n_max));
  DevMem prm, out, alpha, info;
  GPRC_TRY(batch_launches(who, s, kernel, B, r, n_params, xin.dev, x_stride, yin.dev, y_stride, d, grad_out != nullptr, nullptr, prm, out, alpha, info));
  std::vector<double> hout((size_t)(B * out_stride)), halpha(alpha_out ? (size_t)(B * NBI) : 0);
  GPRC_HIP(hipMemcpyAsync(hout.data(), out.p, sizeof(double) * hout.size(), hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipMemcpyAsync(info_out, info.p, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, s));
  if (alpha_out) GPRC_HIP(hipMemcpyAsync(halpha.data(), alpha.p, sizeof(double) * halpha.size(), hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipStreamSynchronize(s));
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  std::vector<long double> sums((size_t)n_params + 1);
  for (int64_t b = 0; b < B; ++b) {
    const double* rr = hout.data() + b * out_stride;
    const bool ok = info_out[b] == 0;
    logp_out[b] = ok ? rr[0] : qnan;
    if (grad_out) {
      for (int k = 0; k <= n_params; ++k) sums[(size_t)k] = (long double)rr[1 + k];
      half_theta_grad(specs[(size_t)b], sums.data(), sums[(size_t)n_params], ok, n_params, grad_out + b * (n_params + 1));
    }
    if (alpha_out) expand_alpha(halpha.data() + b * NBI, ok, n_each ? n_each[b] : n_max, n_max, alpha_out + b * n_max);
  }
  return 0;
}

int gprc_gpr_batch_fit(gprc_ctx* ctx, int kernel, int64_t B, const double* params, int n_params, int64_t ld_params, const double* noise,
                       const double* X, int64_t d, int64_t n_max, int64_t x_stride, const double* y, int64_t y_stride, const int64_t* n_each,
                       gprc_batch_model** model_out, double* logp_out, int* info_out) {
  const char* who = "batch_fit";
  if (model_out) *model_out = nullptr;
  bool empty = false;
  GPRC_TRY(batch_checks(who, ctx, kernel, B, params, n_params, ld_params, noise, X, d, n_max, x_stride, y, y_stride, n_each, model_out, logp_out,
                        info_out, "model_out, logp_out, info_out", &empty));
  if (empty) return 0;   // no models: no object (*model_out stays NULL, which gprc_batch_model_free accepts)
  BatchRecords r;
  GPRC_TRY(batch_records(kernel, B, params, n_params, ld_params, noise, d, n_max, n_each, false, &r));
  GPRC_TRY(use_device(ctx));
  hipStream_t s = ctx->stream;
  std::unique_ptr<gprc_batch_model, BoundDelete> m(new gprc_batch_model);
  m->ctx = ctx;
  m->ctx_id = ctx->id;
  m->kernel = kernel;
  m->n_params = n_params;
  m->np_store = r.np_store;
  m->prm_stride = r.prm_stride;
  m->B = B;
  m->d = d;
  m->n_max = n_max;
  m->x_stride = x_stride;
  m->y_stride = y_stride;
  m->uneven = n_each != nullptr;
  // the model's own copies of the points and the targets: the kernel reads them now, gprc_gpr_batch_predict and gprc_gpr_batch_loo again
  GPRC_TRY(m->X.copy_from(s, X, (x_stride ? (B - 1) * x_stride : 0) + d * n_max));
  GPRC_TRY(m->y.copy_from(s, y, (y_stride ? (B - 1) * y_stride : 0) + n_max));
  if (int rc = m->W.alloc(B * (int64_t)NBI * NBI)) {
    if (rc == GPRC_ERR_NOMEM)
      set_error(std::string(who) + ": L^-1 of every model, " + std::to_string((B * (int64_t)NBI * NBI * 8) >> 20) + " MiB of device memory, could not be allocated");
    return rc;
  }
  DevMem out;
  GPRC_TRY(batch_launches(who, s, kernel, B, r, n_params, m->X.p, x_stride, m->y.p, y_stride, d, false, m->W.p, m->prm, out, m->alpha, m->info));
  std::vector<double> hout((size_t)(B * r.out_stride));
  GPRC_HIP(hipMemcpyAsync(hout.data(), out.p, sizeof(double) * hout.size(), hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipMemcpyAsync(info_out, m->info.p, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipStreamSynchronize(s));
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  for (int64_t b = 0; b < B; ++b) logp_out[b] = info_out[b] == 0 ? hout[(size_t)(b * r.out_stride)] : qnan;
  *model_out = m.release();
  return 0;
}

int gprc_gpr_batch_get_alpha(gprc_batch_model* m, double* alpha_out) {
  const char* who = "batch_get_alpha";
  if (!m) return bad(who, "null model");
  GPRC_TRY(ctx_gone(who, *m));
  GPRC_TRY(batch_kind(who, *m, BATCH_GPR));
  if (!alpha_out) return bad(who, "null output pointer (alpha_out)");
  GPRC_TRY(use_device(m->ctx));
  hipStream_t s = m->ctx->stream;
  std::vector<double> halpha((size_t)(m->B * NBI)), hprm((size_t)(m->B * m->prm_stride));
  std::vector<int> hinfo((size_t)m->B);
  GPRC_HIP(hipMemcpyAsync(halpha.data(), m->alpha.p, sizeof(double) * halpha.size(), hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipMemcpyAsync(hprm.data(), m->prm.p, sizeof(double) * hprm.size(), hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipMemcpyAsync(hinfo.data(), m->info.p, sizeof(int) * hinfo.size(), hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipStreamSynchronize(s));
  for (int64_t b = 0; b < m->B; ++b) {   // as gprc_gpr_batch_logp_grad's alpha_out
    const int64_t nb = (int64_t)hprm[(size_t)(b * m->prm_stride + m->np_store + 1)];
    expand_alpha(halpha.data() + b * NBI, hinfo[(size_t)b] == 0, nb, m->n_max, alpha_out + b * m->n_max);
  }
  return 0;
}

int gprc_gpr_batch_predict(gprc_batch_model* m, const double* X_star, int64_t ns_max, int64_t xs_stride, const int64_t* ns_each, double* mean_out,
                           double* var_out, int64_t ld_out) {
  return batch_predict_any("batch_predict", false, BATCH_GPR, m, X_star, ns_max, xs_stride, ns_each, mean_out, var_out, ld_out, nullptr, nullptr, 0);
}

int gprc_gpr_batch_predict_grad(gprc_batch_model* m, const double* X_star, int64_t ns_max, int64_t xs_stride, const int64_t* ns_each,
                                double* mean_out, double* var_out, int64_t ld_out, double* dmean_out, double* dvar_out, int64_t ld_grad) {
  return batch_predict_any("batch_predict_grad", true, BATCH_GPR, m, X_star, ns_max, xs_stride, ns_each, mean_out, var_out, ld_out, dmean_out, dvar_out, ld_grad);
}

int gprc_gpr_batch_loo(gprc_batch_model* m, double* mean_out, double* var_out, double* logdens_out, int64_t ld_out, double* loo_out) {
  const char* who = "batch_loo";
  if (!m) return bad(who, "null model");
  GPRC_TRY(ctx_gone(who, *m));
  GPRC_TRY(batch_kind(who, *m, BATCH_GPR));
  if (!mean_out && !var_out && !logdens_out && !loo_out) return bad(who, "null output pointers (mean_out, var_out, logdens_out, loo_out: not all four may be NULL)");
  if ((mean_out || var_out || logdens_out) && ld_out < m->n_max) return bad(who, "ld_out < n_max");
  const int64_t B = m->B;
  gprc_ctx* ctx = m->ctx;
  GPRC_TRY(use_device(ctx));
  hipStream_t s = ctx->stream;
  // host outputs as gprc_gpr_batch_predict's: where the launch leaves entries alone the temporary starts as the caller's array
  const int64_t out_count = (B - 1) * ld_out + m->n_max;
  const bool gaps = m->uneven || (ld_out > m->n_max && B > 1);
  Out mean, var, dens;
  GPRC_TRY(mean.set_keeping(mean_out, out_count, gaps, s));
  GPRC_TRY(var.set_keeping(var_out, out_count, gaps, s));
  GPRC_TRY(dens.set_keeping(logdens_out, out_count, gaps, s));
  DevMem score;
  if (loo_out) GPRC_TRY(score.alloc(B));
  BatchLooArgs a{m->W.p, m->alpha.p, m->y.p, m->prm.p, reinterpret_cast<const int*>(m->info.p), mean.dev, var.dev, dens.dev, score.p,
                 m->y_stride, ld_out, 0, m->prm_stride, m->np_store};
  constexpr int64_t GRID_X = int64_t(1) << 30;
  for (int64_t b0 = 0; b0 < B; b0 += GRID_X) {
    a.b0 = b0;
    GPRC_TRY(launch_batch_loo(s, a, std::min<int64_t>(GRID_X, B - b0)));
  }
  if (loo_out) GPRC_HIP(hipMemcpyAsync(loo_out, score.p, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, s));
  return finish_sync(s, mean, var, dens);
}

int gprc_gpc_batch_fit(gprc_ctx* ctx, int kernel, int64_t B, const double* params, int n_params, int64_t ld_params, const double* X, int64_t d,
                       int64_t n_max, int64_t x_stride, const double* y, int64_t y_stride, const int64_t* n_each, double epsilon, int max_iter,
                       gprc_batch_model** model_out, double* logq_out, int* iters_out, int* info_out) {
  const char* who = "gpc_batch_fit";
  if (model_out) *model_out = nullptr;
  if (!(epsilon > 0.0)) return bad(who, "epsilon must be > 0");
  if (max_iter > GPRC_BATCH_GPC_MAX_ITER) return bad(who, "max_iter = " + std::to_string(max_iter) + " > 1000: the loop on the device is bounded");
  if (max_iter <= 0) max_iter = 100;
  bool empty = false;
  GPRC_TRY(batch_checks(who, ctx, kernel, B, params, n_params, ld_params, nullptr, X, d, n_max, x_stride, y, y_stride, n_each, model_out, logq_out,
                        info_out, "model_out, logq_out, info_out", &empty, true));
  if (empty) return 0;   // no models: no object
  BatchRecords r;
  GPRC_TRY(batch_records(kernel, B, params, n_params, ld_params, nullptr, d, n_max, n_each, false, &r));
  GPRC_TRY(use_device(ctx));
  hipStream_t s = ctx->stream;
  std::unique_ptr<gprc_batch_model, BoundDelete> m(new gprc_batch_model);
  m->ctx = ctx;
  m->ctx_id = ctx->id;
  m->kind = BATCH_GPC;
  m->kernel = kernel;
  m->n_params = n_params;
  m->np_store = r.np_store;
  m->prm_stride = r.prm_stride;
  m->B = B;
  m->d = d;
  m->n_max = n_max;
  m->x_stride = x_stride;
  m->y_stride = y_stride;
  m->uneven = n_each != nullptr;
  GPRC_TRY(m->X.copy_from(s, X, (x_stride ? (B - 1) * x_stride : 0) + d * n_max));
  GPRC_TRY(m->y.copy_from(s, y, (y_stride ? (B - 1) * y_stride : 0) + n_max));
  if (int rc = m->W.alloc(B * (int64_t)NBI * NBI)) {
    if (rc == GPRC_ERR_NOMEM)
      set_error(std::string(who) + ": L^-1 diag(sqrt(W)) of every model, " + std::to_string((B * (int64_t)NBI * NBI * 8) >> 20) + " MiB of device memory, could not be allocated");
    return rc;
  }
  const int64_t launch = std::min<int64_t>(B, GPRC_BATCH_LAUNCH);
  DevMem slab, logq, iters;
  GPRC_TRY(m->prm.alloc(B * r.prm_stride));
  GPRC_TRY(m->alpha.alloc(B * NBI));
  GPRC_TRY(m->fhat.alloc(B * NBI));
  GPRC_TRY(m->info.alloc((B + 1) / 2));
  GPRC_TRY(logq.alloc(B));
  GPRC_TRY(iters.alloc((B + 1) / 2));
  GPRC_TRY(slab.alloc((int64_t)batch_gpc_scratch_doubles(launch)));
  GPRC_HIP(hipMemcpyAsync(m->prm.p, r.hprm.data(), sizeof(double) * r.hprm.size(), hipMemcpyHostToDevice, s));
  GPRC_HIP(hipMemsetAsync(m->info.p, 0, sizeof(int) * (size_t)B, s));
  BatchGpcArgs a{m->X.p, m->y.p, m->prm.p, slab.p, logq.p, reinterpret_cast<int*>(iters.p), m->alpha.p, m->fhat.p, m->W.p, reinterpret_cast<int*>(m->info.p),
                 x_stride, y_stride, d, 0, r.prm_stride, r.np_store, n_params, max_iter, epsilon};
  for (int64_t b0 = 0; b0 < B; b0 += launch) {
    a.b0 = b0;
    GPRC_TRY(launch_batch_gpc_fit(s, kernel, a, std::min<int64_t>(launch, B - b0)));
  }
  GPRC_HIP(hipMemcpyAsync(logq_out, logq.p, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipMemcpyAsync(info_out, m->info.p, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, s));
  if (iters_out) GPRC_HIP(hipMemcpyAsync(iters_out, iters.p, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipStreamSynchronize(s));
  *model_out = m.release();
  return 0;
}

int gprc_gpc_batch_predict_latent(gprc_batch_model* m, const double* X_star, int64_t ns_max, int64_t xs_stride, const int64_t* ns_each, double* fs_bar_out,
                                  double* Vfs_out, int64_t ld_out) {
  return batch_predict_any("gpc_batch_predict_latent", false, BATCH_GPC, m, X_star, ns_max, xs_stride, ns_each, fs_bar_out, Vfs_out, ld_out, nullptr, nullptr, 0);
}

int gprc_gpc_batch_predict_class(gprc_batch_model* m, const double* X_star, int64_t ns_max, int64_t xs_stride, const int64_t* ns_each, double* prob_out,
                                 int64_t ld_out) {
  const char* who = "gpc_batch_predict_class";
  if (!m) return bad(who, "null model");
  GPRC_TRY(ctx_gone(who, *m));
  GPRC_TRY(batch_kind(who, *m, BATCH_GPC));
  if (!prob_out) return bad(who, "null output pointer (prob_out)");
  if (ns_max < 1) return bad(who, "ns_max < 1");
  if (ld_out < ns_max) return bad(who, "ld_out < ns_max");
  const int64_t B = m->B;
  GPRC_TRY(use_device(m->ctx));
  hipStream_t s = m->ctx->stream;
  // the latent prediction into pool memory with the caller's pitch (its remaining checks are made there), then the integral where the
  // latent call wrote: one launch over everything when the rows leave no gaps, else a launch per model over its own points
  const int64_t count = (B - 1) * ld_out + ns_max;
  DevMem fs, vf;
  GPRC_TRY(fs.alloc(count));
  GPRC_TRY(vf.alloc(count));
  GPRC_TRY(batch_predict_any(who, false, BATCH_GPC, m, X_star, ns_max, xs_stride, ns_each, fs.p, vf.p, ld_out, nullptr, nullptr, 0));
  const bool gaps = ns_each != nullptr || (ld_out > ns_max && B > 1);
  Out prob;
  GPRC_TRY(prob.set_keeping(prob_out, count, gaps, s));
  if (!gaps) {
    GPRC_TRY(launch_gpc_class_prob(s, fs.p, vf.p, prob.dev, count));
  } else {
    for (int64_t b = 0; b < B; ++b)
      GPRC_TRY(launch_gpc_class_prob(s, fs.p + b * ld_out, vf.p + b * ld_out, prob.dev + b * ld_out, ns_each ? ns_each[b] : ns_max));
  }
  return finish_sync(s, prob);
}

int gprc_gpc_batch_get_f_hat(gprc_batch_model* m, double* f_hat_out) {
  const char* who = "gpc_batch_get_f_hat";
  if (!m) return bad(who, "null model");
  GPRC_TRY(ctx_gone(who, *m));
  GPRC_TRY(batch_kind(who, *m, BATCH_GPC));
  if (!f_hat_out) return bad(who, "null output pointer (f_hat_out)");
  GPRC_TRY(use_device(m->ctx));
  hipStream_t s = m->ctx->stream;
  // the kernel left NaN at a flagged model's points and zero behind n_b: rows of 128 to rows of n_max
  GPRC_HIP(hipMemcpy2DAsync(f_hat_out, sizeof(double) * (size_t)m->n_max, m->fhat.p, sizeof(double) * NBI, sizeof(double) * (size_t)m->n_max, (size_t)m->B,
                            hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipStreamSynchronize(s));
  return 0;
}

int gprc_batch_model_dims(const gprc_batch_model* m, int64_t* B_out, int64_t* d_out, int64_t* n_max_out) {
  if (!m) return bad("batch_model_dims", "null model");
  if (B_out) *B_out = m->B;
  if (d_out) *d_out = m->d;
  if (n_max_out) *n_max_out = m->n_max;
  return 0;
}

int gprc_batch_model_free(gprc_batch_model* m) { return free_bound(m, delete_bound<gprc_batch_model>); }

}  // extern "C"
