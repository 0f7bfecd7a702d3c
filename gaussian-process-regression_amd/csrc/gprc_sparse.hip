// gprc_sparse.hip -- sparse GPR with m inducing points Z (Titsias' variational bound in its collapsed form; DESIGN.md section 7,
// "Sparse GPR"), composed from the launchers and the schedules of gprc_sched.hip, with its C entry points (include/gprc_native.h).
//   K_uu = k(Z,Z) + jitter I = L_u L_u^T          V = K(X,Z) L_u^-T   (n x m, row i = v_i^T)
//   B    = I + V^T V / sigma^2 = L_B L_B^T        b = V^T y,   c = L_B^-1 b / sigma^2
//   t    = sum_i ( k(x_i,x_i) - |v_i|^2 )
//   elbo = -n/2 log(2 pi sigma^2) - sum_j log (L_B)_jj - y^T y / (2 sigma^2) + c^T c / 2 - t / (2 sigma^2)
//   predict at x*:  v* = L_u^-1 k(Z,x*),  w* = L_B^-1 v*,  mean = w*^T c,  var = k(x*,x*) - |v*|^2 + |w*|^2
// The fit is ONE pass over the training points in row chunks (chunk_workspace: the predict's sizing, 256-row granularity): cross fill,
// solve_rows with L_u (its per-block sums of squares give |v_i|^2), launch_gram_rows into the packed buffer of B, launch_col_reduce
// with the chunk of y.  The device holds two packed m x m matrices and one chunk, never X.  Whitening with L_u comes first and B is
// I + ...: forming K_uf K_fu and solving with K_uu afterwards would amplify the product's rounding by 1 / lambda_min(K_uu).
// Every result is a function of (n, m) only, bit for bit, whatever the chunking: a row's arithmetic in the fill and the solve depends
// on columns only, the two reductions over rows are chunk-invariant by construction (kernels_gram.hip), and the host sums t and y^T y
// in index order in long double.
#include <algorithm>
#include <cmath>
#include <new>
#include <utility>
#include <vector>

#include "gprc_host.h"
#include "host_sums.h"

namespace gprc {
namespace {

constexpr long double SGPR_PI = 3.141592653589793238462643383279502884L;

struct SgprArgs {
  const double *X, *y, *Z;
  int64_t d, n, m;
  double noise, jitter;
};

int sgpr_check(const char* who, gprc_ctx* ctx, const SgprArgs& a, bool out_ok) {
  if (!ctx || !a.X || !a.y || !a.Z || !out_ok || a.d < 1) { set_error(std::string(who) + ": bad arguments (null pointer or d < 1)"); return GPRC_ERR_ARG; }
  if (a.n < 1 || a.m < 1) { set_error(std::string(who) + ": n >= 1 training points and m >= 1 inducing points"); return GPRC_ERR_ARG; }
  if (!(a.noise > 0.0) || !std::isfinite(a.noise)) { set_error(std::string(who) + ": noise must be finite and > 0"); return GPRC_ERR_ARG; }
  if (!(a.jitter >= 0.0) || !std::isfinite(a.jitter)) { set_error(std::string(who) + ": jitter must be finite and >= 0"); return GPRC_ERR_ARG; }
  return 0;
}

// an empty sparse model of m inducing points with all its buffers
int sgpr_alloc(gprc_ctx* ctx, const KernelSpec& ks, int64_t m, int64_t d, ModelPtr& mo) {
  gprc_model* p = new (std::nothrow) gprc_model();
  if (!p) { set_error("out of host memory"); return GPRC_ERR_NOMEM; }
  mo.reset(p);
  p->ctx = ctx; p->ctx_id = ctx->id; p->type = MODEL_SGPR; p->ks = ks; p->n = m; p->d = d; p->n_pad = pad_up(m, NB);
  const int64_t m_pad = p->n_pad;
  const std::pair<double**, int64_t> parts[] = {{&p->X, d * m}, {&p->packed, gprc_packed_size(m_pad)}, {&p->winv, gprc_winv_size(m_pad)},
                                                {&p->alpha, m_pad}, {&p->work, gprc_trsv_work_size(m_pad)},
                                                {&p->packed_b, gprc_packed_size(m_pad)}, {&p->winv_b, gprc_winv_size(m_pad)}};
  for (const auto& pr : parts) GPRC_TRY(pool_alloc(ctx, sizeof(double) * (size_t)pr.second, (void**)pr.first));
  return 0;
}

// The fit: both factors, c, elbo and t into the model.  *info_out > 0: the leading minor of K_uu or of B that is not positive (the
// error text says which); the model is then not usable.
int sgpr_fit(gprc_model* mo, const SgprArgs& a, int* info_out) {
  gprc_ctx* ctx = mo->ctx;
  hipStream_t s = ctx->stream;
  const int64_t n = a.n, d = a.d, m = a.m, m_pad = mo->n_pad, nblk = m_pad / NBI;
  *info_out = 0;
  GPRC_HIP(hipMemcpyAsync(mo->X, a.Z, sizeof(double) * d * m, hipMemcpyDefault, s));
  DevMem inv;   // explicit inverses of the diagonal blocks of L_B: the vector solve for c
  GPRC_TRY(inv.alloc(gprc_solve_inv_size(m_pad)));

  // K_uu + jitter I = L_u L_u^T (identity in the padding)
  auto fill_uu = [&]() -> int {
    for (int64_t p = 0; p < m_pad / NB; ++p)
      GPRC_TRY(launch_fill(s, mo->ks, mo->X, m, mo->X, m, d, mo->packed + panel_offset(m_pad, p), panel_ld(m_pad, p), p * NB, m_pad - p * NB,
                           p * NB, NB, PAD_IDENTITY, a.jitter));
    return 0;
  };
  GPRC_TRY(fill_uu());
  int info = 0;
  GPRC_TRY(factor_all_or_refill(ctx, mo->packed, m_pad, mo->winv, &info, nullptr, fill_uu));
  if (info != 0) {
    set_error("sgpr: K_uu + jitter I is not positive definite (leading minor of order " + std::to_string(info) + "): duplicate inducing points need a jitter > 0");
    *info_out = info;
    return 0;
  }

  // the pass over the training points: Phi = V^T V into packed_b, b = V^T y into alpha, the per-point k(x_i,x_i) - |v_i|^2 to the host
  std::vector<double> ht((size_t)n), hy((size_t)n);
  GPRC_HIP(hipMemcpyAsync(hy.data(), a.y, sizeof(double) * n, hipMemcpyDefault, s));
  const bool x_on_device = is_device_ptr(a.X);
  auto accumulate = [&]() -> int {
    int64_t rows = 0;
    double *vt = nullptr, *sspart = nullptr, *kxx = nullptr;
    // The Gram kernel reads 128 bytes of each of 256 columns of the chunk per k-tile: with a column pitch of 2^k bytes (the chunk's rows
    // are a multiple of 256, often a power of two) all of them would sit on one memory channel.  Sixteen doubles of pitch (unless
    // GPRC_VT_PAD asks for its own) move consecutive columns by a cache line; the arithmetic does not see the pitch.
    struct PitchPad {
      gprc_ctx* c; int64_t old;
      explicit PitchPad(gprc_ctx* c_) : c(c_), old(c_->vt_pad) { if (old == 0) c->vt_pad = 16; }
      ~PitchPad() { c->vt_pad = old; }
    } pitch(ctx);
    GPRC_TRY(chunk_workspace(ctx, m_pad, pad_up(n, 256), true, &rows, &vt, &sspart, &kxx));   // rows: a multiple of 256
    const int64_t ldv = rows + ctx->vt_pad;
    DevMem xbuf, ybuf, tdev;
    if (!x_on_device) GPRC_TRY(xbuf.alloc(d * rows));   // host data is staged chunk by chunk: the device never holds X
    GPRC_TRY(ybuf.alloc(rows));
    GPRC_TRY(tdev.alloc(rows));
    GPRC_HIP(hipMemsetAsync(mo->packed_b, 0, sizeof(double) * (size_t)gprc_packed_size(m_pad), s));
    GPRC_HIP(hipMemsetAsync(mo->alpha, 0, sizeof(double) * (size_t)m_pad, s));
    for (int64_t s0 = 0; s0 < n; s0 += rows) {
      const int64_t mcur = std::min<int64_t>(rows, n - s0), mp = pad_up(mcur, 256);
      const double* xc = a.X + s0 * d;
      if (!x_on_device) {
        GPRC_HIP(hipMemcpyAsync(xbuf.p, xc, sizeof(double) * d * mcur, hipMemcpyHostToDevice, s));
        xc = xbuf.p;
      }
      GPRC_HIP(hipMemsetAsync(ybuf.p, 0, sizeof(double) * (size_t)mp, s));   // zero in the padding rows
      GPRC_HIP(hipMemcpyAsync(ybuf.p, a.y + s0, sizeof(double) * mcur, hipMemcpyDefault, s));
      GPRC_TRY(launch_fill(s, mo->ks, xc, mcur, mo->X, m, d, vt, ldv, 0, mp, 0, m_pad, PAD_ZERO, 0.0));   // K(X_chunk, Z), zero padded
      GPRC_TRY(solve_rows(ctx, mo->packed, mo->winv, m_pad, vt, ldv, mp, sspart));                        // V = . L_u^-T, |v_i|^2 by block
      GPRC_TRY(launch_colwise(s, mo->ks, xc, xc, d, mcur, kxx));                                          // k(x_i, x_i)
      GPRC_TRY(launch_sum_partials(s, sspart, nblk, mp, mcur, kxx, tdev.p));                              // k(x_i,x_i) - |v_i|^2
      GPRC_HIP(hipMemcpyAsync(ht.data() + s0, tdev.p, sizeof(double) * mcur, hipMemcpyDeviceToHost, s));
      GPRC_TRY(launch_gram_rows(s, vt, ldv, mp, m_pad, mo->packed_b));                                    // Phi += V^T V
      GPRC_TRY(launch_col_reduce(s, vt, ldv, mp, m_pad, ybuf.p, mo->alpha));                              // b += V^T y
    }
    GPRC_TRY(launch_gram_to_b(s, mo->packed_b, m_pad, a.noise));                                          // B = I + Phi / sigma^2
    GPRC_HIP(hipStreamSynchronize(s));   // the staging buffers go out of scope
    return 0;
  };
  GPRC_TRY(accumulate());
  GPRC_TRY(factor_all_or_refill(ctx, mo->packed_b, m_pad, mo->winv_b, &info, inv.p, accumulate));
  if (info != 0) {
    set_error("sgpr: B = I + V^T V / noise is not positive definite (leading minor of order " + std::to_string(info) + ")");
    *info_out = info;
    return 0;
  }
  GPRC_TRY(launch_trsv(s, mo->packed_b, inv.p, m_pad, mo->alpha, 0, mo->work));   // L_B^-1 b
  GPRC_TRY(launch_div_vec(s, mo->alpha, m_pad, a.noise));                         // c
  GPRC_TRY(launch_diag_log_sum(s, mo->packed_b, m_pad, m, ctx->scal_dev));
  std::vector<double> hc((size_t)m);
  double logdet = 0.0;
  GPRC_HIP(hipMemcpyAsync(hc.data(), mo->alpha, sizeof(double) * m, hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipMemcpyAsync(&logdet, ctx->scal_dev, sizeof(double), hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipStreamSynchronize(s));
  long double t = 0.0L, yy = 0.0L, cc = 0.0L;
  for (int64_t i = 0; i < n; ++i) { t += (long double)ht[(size_t)i]; yy += (long double)hy[(size_t)i] * (long double)hy[(size_t)i]; }
  for (int64_t j = 0; j < m; ++j) cc += (long double)hc[(size_t)j] * (long double)hc[(size_t)j];
  const long double s2 = (long double)a.noise;
  mo->trace = (double)t;
  mo->elbo = (double)(-0.5L * (long double)n * std::log(2.0L * SGPR_PI * s2) - (long double)logdet - yy / (2.0L * s2) + 0.5L * cc - t / (2.0L * s2));
  mo->noise = a.noise; mo->jitter = a.jitter; mo->n_train = n;
  return 0;
}

int sgpr_fit_entry(const char* who, gprc_ctx* ctx, int kernel, const double* params, int n_params, const SgprArgs& a, bool out_ok, ModelPtr& mo) {
  GPRC_TRY(sgpr_check(who, ctx, a, out_ok));
  GPRC_TRY(use_device(ctx));
  KernelSpec ks;
  GPRC_TRY(make_spec(kernel, params, n_params, a.d, &ks));
  GPRC_TRY(sgpr_alloc(ctx, ks, a.m, a.d, mo));
  int info = 0;
  GPRC_TRY(sgpr_fit(mo.get(), a, &info));
  return info;
}

// One chunk of test points: K(X*, Z) -> v* (solve with L_u, |v*|^2) -> w* (solve with L_B, |w*|^2) -> mean = w* . c.  part holds
// [nblk x mp sums of squares of v*][mp: k** - |v*|^2][nblk x mp sums of squares of w*]: the variance is ONE in-order sum of the last
// nblk + 1 rows.
int sgpr_predict_chunk(gprc_model* mo, const double* xc, int64_t mcur, double* vt, int64_t ldv, double* part, double* kss, double* red,
                       double* mean_out, double* var_out) {
  gprc_ctx* ctx = mo->ctx;
  hipStream_t s = ctx->stream;
  const int64_t m = mo->n, m_pad = mo->n_pad, d = mo->d, mp = pad_up(mcur, 128), nblk = m_pad / NBI;
  double *ss1 = part, *u = part + nblk * mp, *ss2 = u + mp;
  GPRC_TRY(launch_fill(s, mo->ks, xc, mcur, mo->X, m, d, vt, ldv, 0, mp, 0, m_pad, PAD_ZERO, 0.0));
  GPRC_TRY(solve_rows(ctx, mo->packed, mo->winv, m_pad, vt, ldv, mp, var_out ? ss1 : nullptr));
  GPRC_TRY(solve_rows(ctx, mo->packed_b, mo->winv_b, m_pad, vt, ldv, mp, var_out ? ss2 : nullptr));
  if (mean_out) GPRC_TRY(launch_row_reduce(s, vt, ldv, mp, m_pad, mo->alpha, red, red + mp));
  if (mean_out) GPRC_HIP(hipMemcpyAsync(mean_out, red, sizeof(double) * mcur, hipMemcpyDeviceToDevice, s));
  if (var_out) {
    GPRC_TRY(launch_colwise(s, mo->ks, xc, xc, d, mcur, kss));
    GPRC_TRY(launch_sum_partials(s, ss1, nblk, mp, mp, kss, u));          // (entries past mcur: unused)
    GPRC_TRY(launch_sum_partials(s, u, nblk + 1, mp, mcur, nullptr, var_out));
  }
  return 0;
}

}  // namespace
}  // namespace gprc

using namespace gprc;

extern "C" {

int gprc_sgpr_fit(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n, const double* y,
                  double noise, const double* Z, int64_t m, double jitter, gprc_model** model_out) {
  ModelPtr mo;
  GPRC_TRY(sgpr_fit_entry("sgpr_fit", ctx, kernel, params, n_params, SgprArgs{X, y, Z, d, n, m, noise, jitter}, model_out != nullptr, mo));
  *model_out = mo.release();
  return 0;
}

int gprc_sgpr_elbo(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n, const double* y,
                   double noise, const double* Z, int64_t m, double jitter, double* elbo_out, double* trace_out) {
  ModelPtr mo;
  GPRC_TRY(sgpr_fit_entry("sgpr_elbo", ctx, kernel, params, n_params, SgprArgs{X, y, Z, d, n, m, noise, jitter}, elbo_out != nullptr, mo));
  *elbo_out = mo->elbo;
  if (trace_out) *trace_out = mo->trace;
  GPRC_HIP(hipStreamSynchronize(ctx->stream));   // the model's buffers go back to the pool
  return 0;
}

int gprc_sgpr_get_elbo(gprc_model* model, double* elbo_out, double* trace_out) {
  if (!model || model->type != MODEL_SGPR || !elbo_out) { set_error("sgpr_get_elbo: not a sparse GPR model (or a null output)"); return GPRC_ERR_ARG; }
  *elbo_out = model->elbo;
  if (trace_out) *trace_out = model->trace;
  return 0;
}

int gprc_sgpr_get_c(gprc_model* model, double* c_out) {
  if (!model || model->type != MODEL_SGPR || !c_out) { set_error("sgpr_get_c: not a sparse GPR model (or a null output)"); return GPRC_ERR_ARG; }
  if (!model->ctx || !ctx_alive(model->ctx, model->ctx_id)) { set_error("sgpr_get_c: the model's context has been destroyed"); return GPRC_ERR_ARG; }
  GPRC_TRY(use_device(model->ctx));
  GPRC_HIP(hipMemcpyAsync(c_out, model->alpha, sizeof(double) * model->n, hipMemcpyDefault, model->ctx->stream));
  GPRC_HIP(hipStreamSynchronize(model->ctx->stream));
  return 0;
}

int gprc_sgpr_predict(gprc_model* mo, const double* X_star, int64_t ns, double* mean_out, double* var_out) {
  if (!mo || mo->type != MODEL_SGPR) { set_error("sgpr_predict: not a sparse GPR model"); return GPRC_ERR_ARG; }
  if (ns < 0 || (ns > 0 && !X_star) || (!mean_out && !var_out)) { set_error("sgpr_predict: bad arguments (non-null X_star, at least one output)"); return GPRC_ERR_ARG; }
  if (!mo->ctx || !ctx_alive(mo->ctx, mo->ctx_id)) { set_error("sgpr_predict: the model's context has been destroyed"); return GPRC_ERR_ARG; }
  if (ns == 0) return 0;
  gprc_ctx* ctx = mo->ctx;
  GPRC_TRY(use_device(ctx));
  hipStream_t s = ctx->stream;
  const int64_t m_pad = mo->n_pad;
  In xs;
  Out om, ov;
  GPRC_TRY(xs.set(s, X_star, mo->d * ns));
  if (mean_out) GPRC_TRY(om.set(mean_out, ns));
  if (var_out) GPRC_TRY(ov.set(var_out, ns));
  int64_t rows = 0;
  double *vt = nullptr, *part = nullptr, *kss = nullptr;
  GPRC_TRY(chunk_workspace(ctx, m_pad, ns, true, &rows, &vt, &part, &kss));
  const int64_t ldv = rows + ctx->vt_pad;
  DevMem red;   // the mean of a chunk + the row reduction's partials
  GPRC_TRY(red.alloc(rows * (1 + rowreduce_splits(m_pad))));
  for (int64_t s0 = 0; s0 < ns; s0 += rows) {
    const int64_t mcur = std::min<int64_t>(rows, ns - s0);
    GPRC_TRY(sgpr_predict_chunk(mo, xs.dev + s0 * mo->d, mcur, vt, ldv, part, kss, red.p, mean_out ? om.dev + s0 : nullptr, var_out ? ov.dev + s0 : nullptr));
  }
  if (mean_out) GPRC_TRY(om.finish(s));
  if (var_out) GPRC_TRY(ov.finish(s));
  GPRC_HIP(hipStreamSynchronize(s));
  return 0;
}

}  // extern "C"
