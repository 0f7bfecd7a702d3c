// gprc_model.hip -- everything that holds a gprc_model: the GPR fit, extend and predict, the GPC mode search, the exact gradients,
// multivariate-normal sampling and the symmetric eigensolver, each composed from the launchers and the schedules of gprc_sched.hip,
// with their C entry points (include/gprc_native.h).
#include <algorithm>
#include <array>
#include <cmath>
#include <new>
#include <utility>

#include "gprc_host.h"
#include "host_sums.h"
#include "pair_tile.h"

namespace gprc {

int make_spec(int kernel, const double* params, int n_params, int64_t d, KernelSpec* ks) {
  if (n_params > MAX_PARAMS) { set_error("at most 256 kernel parameters (a per-coordinate sigma of the linear kernel needs d <= 256; a scalar sigma has no limit)"); return GPRC_ERR_ARG; }
  if (n_params < 0 || (n_params > 0 && !params)) { set_error("bad kernel parameter vector"); return GPRC_ERR_ARG; }
  bool ok = false;
  switch (kernel) {
    case GPRC_CONSTANT: ok = n_params == 1; break;
    case GPRC_LINEAR: ok = n_params == 1 || n_params == d; break;
    case GPRC_POLYNOMIAL: case GPRC_GAMMAEXP: case GPRC_RATQUAD: ok = n_params == 2; break;
    case GPRC_SQREXP: ok = n_params == 1; break;
    case GPRC_SQREXP_ARD: case GPRC_MATERN32_ARD: case GPRC_MATERN52_ARD: case GPRC_MATERN32: case GPRC_MATERN52: {
      const std::string name = kernel == GPRC_SQREXP_ARD ? "sqrexp_ard" : kernel == GPRC_MATERN32_ARD ? "matern32_ard" : kernel == GPRC_MATERN52_ARD ? "matern52_ard"
                               : kernel == GPRC_MATERN32 ? "matern32" : "matern52";
      if (kernel == GPRC_MATERN32 || kernel == GPRC_MATERN52) {
        if (n_params != 1) { set_error(name + ": one length scale (n_params == 1)"); return GPRC_ERR_ARG; }
      } else if (n_params != d) { set_error(name + ": one length scale per input dimension (n_params == d <= 256)"); return GPRC_ERR_ARG; }
      for (int i = 0; i < n_params; ++i)
        if (!(params[i] > 0.0) || !std::isfinite(params[i])) { set_error(name + ": every length scale must be finite and > 0"); return GPRC_ERR_ARG; }
      ok = true;
      break;
    }
    default: set_error("unknown kernel id"); return GPRC_ERR_ARG;
  }
  if (!ok) { set_error("wrong number of kernel parameters for this kernel"); return GPRC_ERR_ARG; }
  ks->id = kernel;
  ks->n_params = n_params;
  for (int i = 0; i < MAX_PARAMS; ++i) ks->p[i] = i < n_params ? params[i] : 0.0;
  return 0;
}

// the device buffers of a model and their sizes in doubles; the last two are GPC's
static std::array<std::pair<double**, int64_t>, 8> model_parts(gprc_model* m) {
  const int64_t n_pad = m->n_pad;
  return {{{&m->X, m->d * m->n}, {&m->y, n_pad}, {&m->packed, gprc_packed_size(n_pad)}, {&m->winv, gprc_winv_size(n_pad)},
           {&m->alpha, n_pad}, {&m->work, gprc_trsv_work_size(n_pad)}, {&m->f_hat, n_pad}, {&m->sw, n_pad}}};
}

void free_model(gprc_model* m) {
  if (!m) return;
  if (m->ctx) (void)hipSetDevice(m->ctx->device);
  if (m->borrowed) m->X = m->y = m->packed = m->winv = m->alpha = nullptr;
  for (const auto& pr : model_parts(m))
    if (*pr.first) pool_release(m->ctx, *pr.first, sizeof(double) * (size_t)pr.second);
  if (m->packed_rev) pool_release(m->ctx, m->packed_rev, sizeof(double) * (size_t)gprc_packed_size(m->n_pad));   // the model's own, borrowed or not
  if (m->winv_rev) pool_release(m->ctx, m->winv_rev, sizeof(double) * (size_t)gprc_winv_size(m->n_pad));
  if (m->packed_b) pool_release(m->ctx, m->packed_b, sizeof(double) * (size_t)gprc_packed_size(m->n_pad));         // a sparse model's factor of B
  if (m->winv_b) pool_release(m->ctx, m->winv_b, sizeof(double) * (size_t)gprc_winv_size(m->n_pad));
  if (m->pq) pool_release(m->ctx, m->pq, sizeof(double) * (size_t)(m->n * m->rank));                                  // an iterative model's Q
  if (m->pl) pool_release(m->ctx, m->pl, sizeof(double) * (size_t)(m->n * m->rank));                                  // ... and its L
  delete m;
}

namespace {

// a model of n points bound to ctx, no buffers yet; nullptr (error set): out of host memory
gprc_model* new_model(gprc_ctx* ctx, int type, const KernelSpec& ks, int64_t n, int64_t d) {
  gprc_model* m = new (std::nothrow) gprc_model();
  if (!m) { set_error("out of host memory"); return nullptr; }
  m->ctx = ctx; m->ctx_id = ctx->id; m->type = type; m->ks = ks; m->n = n; m->d = d; m->n_pad = pad_up(n, NB);
  return m;
}

int alloc_model(gprc_ctx* ctx, int type, const KernelSpec& ks, int64_t n, int64_t d, ModelPtr& m) {
  m.reset(new_model(ctx, type, ks, n, d));
  if (!m) return GPRC_ERR_NOMEM;
  const auto parts = model_parts(m.get());
  for (int i = 0; i < (type == MODEL_GPC ? 8 : 6); ++i)
    GPRC_TRY(pool_alloc(ctx, sizeof(double) * (size_t)parts[i].second, (void**)parts[i].first));
  return 0;
}

// How every fit begins: the argument checks (out_ok: the caller's output pointers are there; scalar_bad: the text about noise or
// epsilon when that value is out of range, else null), then an empty model of `type` on the context's device
int begin_model(const char* who, int type, gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d,
                int64_t n, const double* y, bool out_ok, const char* scalar_bad, ModelPtr& m) {
  if (!ctx || !X || !y || !out_ok || d < 1 || n < 1) return bad(who, "bad arguments");
  if (scalar_bad) { set_error(scalar_bad); return GPRC_ERR_ARG; }
  GPRC_TRY(use_device(ctx));
  KernelSpec ks;
  GPRC_TRY(make_spec(kernel, params, n_params, d, &ks));
  return alloc_model(ctx, type, ks, n, d, m);
}

// alpha = (L L^T)^-1 y and logp of a factored model; inv: the explicit inverses of the factor's diagonal blocks.  Synchronises.
int gpr_alpha_logp(gprc_model* m, const double* inv) {
  gprc_ctx* ctx = m->ctx;
  hipStream_t s = ctx->stream;
  GPRC_HIP(hipMemcpyAsync(m->alpha, m->y, sizeof(double) * m->n_pad, hipMemcpyDeviceToDevice, s));
  GPRC_TRY(launch_trsv(s, m->packed, inv, m->n_pad, m->alpha, 0, m->work));
  GPRC_TRY(launch_trsv(s, m->packed, inv, m->n_pad, m->alpha, 1, m->work));
  GPRC_TRY(launch_logp(s, m->packed, m->n_pad, m->n, m->y, m->alpha, ctx->scal_dev));
  GPRC_HIP(hipMemcpyAsync(&m->logp, ctx->scal_dev, sizeof(double), hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipStreamSynchronize(s));
  return 0;
}

// one attempt; model must already hold X and y.  *info_out = LAPACK info.
int gpr_attempt(gprc_model* m, double noise, int* info_out) {
  gprc_ctx* ctx = m->ctx;
  hipStream_t s = ctx->stream;
  const int64_t n = m->n, n_pad = m->n_pad, P = n_pad / NB;
  auto fill = [&]() -> int {
    for (int64_t p = 0; p < P; ++p)
      GPRC_TRY(launch_fill(s, m->ks, m->X, n, m->X, n, m->d, m->packed + panel_offset(n_pad, p), panel_ld(n_pad, p), p * NB,
                           n_pad - p * NB, p * NB, NB, PAD_IDENTITY, noise));
    return 0;
  };
  GPRC_TRY(fill());
  DevMem inv;   // explicit inverses of the diagonal blocks: needed by the two vector solves only
  GPRC_TRY(inv.alloc(gprc_solve_inv_size(n_pad)));
  GPRC_TRY(factor_all_or_refill(ctx, m->packed, n_pad, m->winv, info_out, inv.p, fill));
  if (*info_out != 0) return 0;
  GPRC_TRY(gpr_alpha_logp(m, inv.p));
  m->noise = noise;
  return 0;
}

int gpr_prepare(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n,
                const double* y, double noise, ModelPtr& m, bool out_ok = true) {
  GPRC_TRY(begin_model("fit", MODEL_GPR, ctx, kernel, params, n_params, X, d, n, y, out_ok,
                       noise >= 0.0 ? nullptr : "noise must be >= 0", m));  // R/GPRclass.R:130
  hipStream_t s = ctx->stream;
  hipError_t e = hipMemcpyAsync(m->X, X, sizeof(double) * d * n, hipMemcpyDefault, s);
  if (e == hipSuccess) e = hipMemsetAsync(m->y, 0, sizeof(double) * m->n_pad, s);
  if (e == hipSuccess) e = hipMemcpyAsync(m->y, y, sizeof(double) * n, hipMemcpyDefault, s);
  if (e != hipSuccess) return hip_fail(e, "copy X,y", __FILE__, __LINE__);
  return 0;
}

// prepare + one attempt that must succeed: info > 0 is the error "the leading minor ... is not positive definite"
int gpr_fit_once(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n, const double* y,
                 double noise, ModelPtr& m, bool out_ok = true) {
  GPRC_TRY(gpr_prepare(ctx, kernel, params, n_params, X, d, n, y, noise, m, out_ok));
  int info = 0;
  GPRC_TRY(gpr_attempt(m.get(), noise, &info));
  if (info != 0) { set_error("the leading minor of order " + std::to_string(info) + " is not positive definite"); return info; }
  return 0;
}

// eigen(A, symmetric = TRUE) on the device: cyclic Jacobi (kernels_eig.hip).  A_dev: m x m, lower triangle read.
// On return V_dev (m x m) holds the eigenvectors in Jacobi order, `values` the matching eigenvalues and `perm` the
// column order that makes them decreasing (R's convention).
int sym_eigen_dev(gprc_ctx* ctx, const double* A_dev, int64_t lda, int64_t m, double* V_dev, std::vector<double>& values,
                  std::vector<int>& perm, int* sweeps_out) {
  if (m < 1 || m > 16384) { set_error("eigen: m must be in [1, 16384]"); return GPRC_ERR_ARG; }
  hipStream_t s = ctx->stream;
  DevMem W, cs, od;
  GPRC_TRY(W.alloc(m * m));
  GPRC_TRY(cs.alloc(m + 2));
  GPRC_TRY(od.alloc(2 * m));
  std::vector<double> h(2 * m);
  // The sweeps run on W = 2^-e A with max|W| in [1, 2): the stop rule squares the entries, and the squares of an A below 2^-511 or
  // above 2^511 leave the double range.  A power of two changes no bit of a rotation, so the vectors are those of A and the values
  // are scaled back exactly.
  GPRC_TRY(launch_sym_absmax(s, A_dev, lda, (int)m, od.p));
  GPRC_HIP(hipMemcpyAsync(h.data(), od.p, sizeof(double) * m, hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipStreamSynchronize(s));
  double amax = 0.0;
  for (int64_t j = 0; j < m; ++j) amax = h[j] > amax ? h[j] : amax;
  if (!std::isfinite(amax)) { set_error("eigen: matrix has non-finite entries"); return GPRC_ERR_ARG; }
  const int e = amax > 0.0 ? std::min(std::max(std::ilogb(amax), -1022), 1022) : 0;
  GPRC_TRY(launch_sym_copy(s, A_dev, lda, m, std::ldexp(1.0, -e), W.p, V_dev));
  int sweeps = 0;
  for (;; ++sweeps) {
    GPRC_TRY(launch_jacobi_offnorm(s, W.p, (int)m, od.p, od.p + m));
    GPRC_HIP(hipMemcpyAsync(h.data(), od.p, sizeof(double) * 2 * m, hipMemcpyDeviceToHost, s));
    GPRC_HIP(hipStreamSynchronize(s));
    long double off2 = 0.0L, dg2 = 0.0L;
    for (int64_t j = 0; j < m; ++j) { off2 += h[j]; dg2 += (long double)h[m + j] * h[m + j]; }
    // ||off||_F <= max(1e-15, m eps) ||A||_F: below m*eps the off-diagonal part is rounding noise of the rotations
    // themselves (a rank-deficient covariance keeps ~m^2 such entries alive in its null space) and never shrinks
    const long double rel = std::max(1e-15L, (long double)m * 2.220446049250313e-16L);
    if (off2 <= rel * rel * (off2 + dg2) || sweeps >= 40) break;
    if (m > 1) GPRC_TRY(launch_jacobi_sweep(s, W.p, V_dev, (int)m, cs.p));
  }
  values.resize(m);
  for (int64_t j = 0; j < m; ++j) values[j] = std::ldexp(h[m + j], e);
  perm.resize(m);
  for (int64_t j = 0; j < m; ++j) perm[j] = (int)j;
  std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return values[a] > values[b]; });
  if (sweeps_out) *sweeps_out = sweeps;
  return 0;
}

// t(chol(cov)) or, when that fails, eigen$vectors %*% diag(sqrt(pmax(eigen$values, 0)))  (R/GPRclass.R:362-368).
// L_dev: m x m (ld m).  *method: 1 Cholesky (L lower triangular), 2 eigen.
int mvn_factor_dev(gprc_ctx* ctx, const double* cov_dev, int64_t ld, int64_t m, double tol, double* L_dev, int* method) {
  hipStream_t s = ctx->stream;
  const int64_t n_pad = pad_up(m, NB);
  {
    DevMem packed, winv;
    GPRC_TRY(packed.alloc(gprc_packed_size(n_pad)));
    GPRC_TRY(winv.alloc(gprc_winv_size(n_pad)));
    auto pack = [&]() -> int { return launch_pack_dense(s, cov_dev, ld, m, n_pad, packed.p); };
    GPRC_TRY(pack());
    int info = 0;
    GPRC_TRY(factor_all_or_refill(ctx, packed.p, n_pad, winv.p, &info, nullptr, pack));
    if (info == 0) {
      GPRC_TRY(launch_unpack_L(s, packed.p, n_pad, m, L_dev, m));
      GPRC_HIP(hipStreamSynchronize(s));
      *method = 1;
      return 0;
    }
  }
  DevMem V, scale;
  IntMem permd;
  GPRC_TRY(V.alloc(m * m));
  GPRC_TRY(scale.alloc(m));
  GPRC_HIP(hipMalloc(&permd.p, sizeof(int) * (size_t)m));
  std::vector<double> values;
  std::vector<int> perm;
  GPRC_TRY(sym_eigen_dev(ctx, cov_dev, ld, m, V.p, values, perm, nullptr));
  std::vector<double> sc(m);
  const double lead = std::fabs(values[perm[0]]);
  for (int64_t k = 0; k < m; ++k) {
    const double ev = values[perm[k]];
    if (!(ev > -tol * lead)) {  // stopifnot(all(eigval > -tol * abs(eigval[1])))  :366
      set_error("multivariate_normal: covariance is not positive semi-definite (eigenvalue " + std::to_string(ev) + ")");
      return GPRC_ERR_NOT_PD;
    }
    sc[k] = std::sqrt(ev > 0.0 ? ev : 0.0);
  }
  GPRC_HIP(hipMemcpyAsync(scale.p, sc.data(), sizeof(double) * m, hipMemcpyHostToDevice, s));
  GPRC_HIP(hipMemcpyAsync(permd.p, perm.data(), sizeof(int) * m, hipMemcpyHostToDevice, s));
  GPRC_TRY(launch_gather_scale_cols(s, V.p, (int)m, permd.p, scale.p, L_dev, m));
  GPRC_HIP(hipStreamSynchronize(s));
  *method = 2;
  return 0;
}

// One chunk of the test points, everything fused ("Predict epilogues"; section 7, "Prediction gradients"): THE
// chunk pipeline of gprc_gpr_predict, gprc_gpc_predict_latent and gprc_gpr_predict_grad.
//   fill K*^T chunk   + per-tile partials of K*^T w            (w = alpha; GPC: g, with the stored columns scaled by colscale = sqrt(W))
//   vt := vt L^-T     + per-block sums of squares in the panel solves
//   tail              mean = sum of the fill partials; var = k(x*,x*) - sum of the block sums     (R/GPRclass.R:161,164)
//   gradients         vt := vt J,  vt := vt M^-T = (V L^-1) J  with the reversed factor,  the contraction and its two tails
// The chunk is written once by the fill and read/written only by the solves: the two row-reduction passes over it are gone.
// Null outputs switch their stages off; want_solved: the caller reads vt = V L^-1 afterwards (the full covariance), so the solve runs
// whatever the outputs.  vt / part / kss_c are null when neither the mean nor a solve is wanted.  Mean and variance are the same
// launches with the same arguments for every caller: their bits do not depend on which gradients are asked for.
int predict_chunk(gprc_model* m, const double* xc, int64_t mcur, double* vt, int64_t ldv, double* part, double* kss_c, const double* colscale,
                  bool want_solved, double* mean_out, double* var_out, double* pmean = nullptr, double* pvar = nullptr, double* dmean_out = nullptr,
                  double* dvar_out = nullptr) {
  gprc_ctx* ctx = m->ctx;
  hipStream_t s = ctx->stream;
  const int64_t n = m->n, n_pad = m->n_pad, d = m->d, m_pad = pad_up(mcur, PT_R);
  const bool solve = want_solved || var_out || dvar_out;
  if (mean_out || solve) {
    const int64_t mt = fill_mean_tiles(n_pad);
    double* mpart = part;
    double* sspart = part + mt * m_pad;
    GPRC_TRY(launch_fill_cross_fused(s, m->ks, xc, mcur, m->X, n, d, vt, ldv, m_pad, n_pad, mean_out ? m->alpha : nullptr, mpart, colscale));  // :160-161
    if (solve) GPRC_TRY(solve_rows(ctx, m->packed, m->winv, n_pad, vt, ldv, m_pad, var_out ? sspart : nullptr));                                 // :162
    if (mean_out) GPRC_TRY(launch_sum_partials(s, mpart, mt, m_pad, mcur, nullptr, mean_out));
    if (var_out) {
      GPRC_TRY(launch_colwise(s, m->ks, xc, xc, d, mcur, kss_c));                                                                                // k(X*,X*)  :164
      GPRC_TRY(launch_sum_partials(s, sspart, n_pad / NBI, m_pad, mcur, kss_c, var_out));
    }
  }
  if (dvar_out) {
    GPRC_TRY(launch_reverse_cols(s, vt, ldv, m_pad, n_pad));
    GPRC_TRY(solve_rows(ctx, m->packed_rev, m->winv_rev, n_pad, vt, ldv, m_pad));
  }
  if (pmean || pvar) GPRC_TRY(launch_pred_grad(s, m->ks, xc, mcur, m_pad, m->X, n, n_pad, d, m->alpha, dvar_out ? vt : nullptr, ldv, pmean, pvar));
  if (dmean_out) GPRC_TRY(launch_pred_grad_sum(s, m->ks, pmean, n_pad, d, m_pad, mcur, false, dmean_out));
  if (dvar_out) GPRC_TRY(launch_pred_grad_sum(s, m->ks, pvar, n_pad, d, m_pad, mcur, true, dvar_out));
  return 0;
}

// ---- extend: append observations to a fitted GPR model (DESIGN.md section "Extend") -----------------------------------------
// Refactor from the last panel boundary n0 = floor(n / NB) NB: columns [0, n0) of L stay valid in L' = chol(K' + noise I).  The
// TAIL -- old points [n0, n) and the m new ones, t = n' - n0 rows -- gets
//   L21 = K(X_tail, X[, 1:n0]) L11^-T          solve_rows with the OLD factor, panels [0, p0) only (later columns never feed back)
//   panels [0, p0) of L'                       extend_merge: old rows [p NB, n0) + the tail rows of L21, in the new layout
//   L22 = chol(K22 + noise I - L21 L21^T)      fill + one update pass with panels [0, p0) + factor_all on the SUB-VIEW
// The sub-view: panels p0.. of a packed matrix of n_pad' are a packed matrix of n_pad' - n0 of their own, at packed' +
// panel_offset(n_pad', p0) (offset(n_pad, p0 + k) - offset(n_pad, p0) = offset(n_pad - p0 NB, k)), its winv at winv' + n0 NBI and its
// inv at inv' + p0 NB NB -- so the factor schedules run on it unchanged.  Everything is built in NEW buffers (peak memory: the old
// model plus the new one); the model changes only on success.  *info_out > 0: the global 1-based column of the first non-PD minor.
int gpr_extend(gprc_model* m, const double* X_new, int64_t mnew, const double* y_new, int* info_out) {
  gprc_ctx* ctx = m->ctx;
  hipStream_t s = ctx->stream;
  const int64_t n = m->n, d = m->d, n_pad = m->n_pad;
  const int64_t n1 = n + mnew, n_pad1 = pad_up(n1, NB), P1 = n_pad1 / NB;
  const int64_t n0 = n / NB * NB, p0 = n0 / NB, t = n1 - n0, t_pad = pad_up(t, 128);
  *info_out = 0;
  In xin, yin;
  GPRC_TRY(xin.set(s, X_new, d * mnew));
  GPRC_TRY(yin.set(s, y_new, mnew));
  ModelPtr nm;   // the new buffers; whatever it holds at the end goes back to the pool
  GPRC_TRY(alloc_model(ctx, MODEL_GPR, m->ks, n1, d, nm));
  DevMem inv;
  GPRC_TRY(inv.alloc(gprc_solve_inv_size(n_pad1)));
  GPRC_HIP(hipMemcpyAsync(nm->X, m->X, sizeof(double) * d * n, hipMemcpyDeviceToDevice, s));                  // cbind(X, X_new)
  GPRC_HIP(hipMemcpyAsync(nm->X + d * n, xin.dev, sizeof(double) * d * mnew, hipMemcpyDeviceToDevice, s));
  GPRC_HIP(hipMemsetAsync(nm->y, 0, sizeof(double) * n_pad1, s));                                              // c(y, y_new), zero padded
  GPRC_HIP(hipMemcpyAsync(nm->y, m->y, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
  GPRC_HIP(hipMemcpyAsync(nm->y + n, yin.dev, sizeof(double) * mnew, hipMemcpyDeviceToDevice, s));
  if (p0 > 0) {
    const int64_t ldv = t_pad + ctx->vt_pad;
    double* vt = nullptr;
    GPRC_TRY(ws_get(ctx, 0, ldv * n0, &vt));
    GPRC_TRY(launch_fill(s, m->ks, nm->X + d * n0, t, m->X, n, d, vt, ldv, 0, t_pad, 0, n0, PAD_ZERO, 0.0));   // K(X_tail, X[, 1:n0])
    GPRC_TRY(solve_rows(ctx, m->packed, m->winv, n_pad, vt, ldv, t_pad, nullptr, -1, p0));                      // L21 = . L11^-T
    GPRC_TRY(launch_extend_merge(s, m->packed, n_pad, vt, ldv, t_pad, t, n0, n_pad1, nm->packed));
    GPRC_HIP(hipMemcpyAsync(nm->winv, m->winv, sizeof(double) * n0 * NBI, hipMemcpyDeviceToDevice, s));         // kept diagonal blocks
  }
  auto fill_tail = [&]() -> int {   // K22 + noise I (identity padding), then - L21 L21^T in one pass (K = n0)
    for (int64_t p = p0; p < P1; ++p)
      GPRC_TRY(launch_fill(s, m->ks, nm->X, n1, nm->X, n1, d, nm->packed + panel_offset(n_pad1, p), panel_ld(n_pad1, p), p * NB,
                           n_pad1 - p * NB, p * NB, NB, PAD_IDENTITY, m->noise));
    if (p0 == 1) GPRC_TRY(launch_trailing_update(s, nm->packed, n_pad1, 0, p0, P1, 1));
    else if (p0 > 1) GPRC_TRY(launch_trailing_range(s, nm->packed, n_pad1, 0, p0, p0, P1, 1));
    return 0;
  };
  GPRC_TRY(fill_tail());
  int info = 0;
  GPRC_TRY(factor_all_or_refill(ctx, nm->packed + panel_offset(n_pad1, p0), n_pad1 - n0, nm->winv + n0 * NBI, &info, inv.p + p0 * NB * NB,
                                fill_tail));
  if (info != 0) { *info_out = info + (int)n0; return 0; }
  GPRC_TRY(launch_inv512(s, nm->packed, n_pad1, nm->winv, inv.p, 0, p0));
  GPRC_TRY(gpr_alpha_logp(nm.get(), inv.p));
  // success: the new buffers become the model's, the old ones leave with `nm` (free_model sizes them by the swapped n, n_pad) -- the
  // reversed factor of gprc_gpr_predict_grad among them: the factor has changed, the next gradient call builds it again
  nm->noise = m->noise;   // (context, kernel, type and d are the same in both)
  std::swap(*m, *nm);
  return 0;
}

struct GpcMode {   // the state of gpc_mode_search (below)
  DevMem Kf, vec, red, inv;
  int it = 0;
  double objective = 0.0;
};
// out = v - sw B^-1 sw K v with the factor of B the model holds: the Newton step's a from b (R/GPCclass.R:82-84), the evidence
// gradient's u from s2.  st->vec + n_pad is the scratch; v and out must not be it.
int gpc_apply(gprc_model* m, GpcMode* st, const double* v, double* out) {
  hipStream_t s = m->ctx->stream;
  const int64_t n_pad = m->n_pad;
  double* t = st->vec.p + n_pad;
  GPRC_TRY(launch_row_reduce(s, st->Kf.p, n_pad, n_pad, n_pad, v, t, st->red.p));  // K %*% v
  GPRC_TRY(launch_gpc_scale(s, m->sw, t, t, n_pad));                                // sqrt(W) * .
  GPRC_TRY(launch_trsv(s, m->packed, st->inv.p, n_pad, t, 0, m->work));             // :82
  GPRC_TRY(launch_trsv(s, m->packed, st->inv.p, n_pad, t, 1, m->work));             // :83
  return launch_gpc_a(s, v, m->sw, t, out, n_pad);                                  // :84
}

// The Laplace mode search of GPC$initialize (R/GPCclass.R:73-102), shared by gprc_gpc_fit and gprc_gpc_logq_grad: Newton / IRLS from
// f = 0 until |delta objective| < epsilon, then the final B = L L^T at the mode.  The model receives X, y, f_hat, sw and the factor; the
// state keeps what the evidence gradient goes on with: the dense K, a = K^-1 f_hat (vec + 2 n_pad), the objective at the mode and,
// with final_inv, the explicit diagonal-block inverses of the FINAL factor (the fit does not need them and does not compute them).
// st->it is set whatever the outcome (0: the loop was never reached).
int gpc_mode_search(gprc_model* m, const double* X, const double* y, double epsilon, int max_iter, int flags, bool final_inv, GpcMode* st) {
  gprc_ctx* ctx = m->ctx;
  hipStream_t s = ctx->stream;
  const int64_t n = m->n, d = m->d, n_pad = m->n_pad;
  const KernelSpec& ks = m->ks;
  if (max_iter <= 0) max_iter = 1000;
  DevMem &Kf = st->Kf, &vec = st->vec, &red = st->red, &inv = st->inv;
  GPRC_TRY(Kf.alloc(n_pad * n_pad));
  GPRC_TRY(vec.alloc(4 * n_pad));
  GPRC_TRY(red.alloc(n_pad * rowreduce_splits(n_pad)));
  double *b = vec.p, *a = vec.p + 2 * n_pad, *f = m->f_hat;
  GPRC_HIP(hipMemcpyAsync(m->X, X, sizeof(double) * d * n, hipMemcpyDefault, s));
  GPRC_HIP(hipMemsetAsync(m->y, 0, sizeof(double) * n_pad, s));
  GPRC_HIP(hipMemcpyAsync(m->y, y, sizeof(double) * n, hipMemcpyDefault, s));
  GPRC_HIP(hipMemsetAsync(f, 0, sizeof(double) * n_pad, s));  // f <- rep(0, n)  R/GPCclass.R:74
  GPRC_HIP(hipMemsetAsync(vec.p, 0, sizeof(double) * 4 * n_pad, s));
  for (int64_t c0 = 0; c0 < n_pad; c0 += 32768) {  // K <- covariance_matrix(X, X, k)  :73 (dense, zero padded)
    const int64_t nc = (n_pad - c0 < 32768) ? n_pad - c0 : 32768;
    GPRC_TRY(launch_fill(s, ks, m->X, n, m->X, n, d, Kf.p + c0 * n_pad, n_pad, 0, n_pad, c0, nc, PAD_ZERO, 0.0));
  }
  // explicit inverses of B's diagonal blocks, for the two vector solves of an iteration
  GPRC_TRY(inv.alloc(gprc_solve_inv_size(n_pad)));
  // sw, b from f (:78-81) and B = I + sw K sw = L L^T (:80); inv_or_null: where the factor's explicit inverses go
  auto factor_B = [&](double* inv_or_null, const char* not_pd) -> int {
    GPRC_TRY(launch_gpc_pre(s, f, m->y, n, m->sw, b));
    auto build_B = [&]() -> int { return launch_gpc_build_B(s, Kf.p, n_pad, m->sw, m->packed); };
    GPRC_TRY(build_B());
    int info = 0;
    GPRC_TRY(factor_all_or_refill(ctx, m->packed, n_pad, m->winv, &info, inv_or_null, build_B));
    if (info != 0) { set_error(not_pd); return info; }
    return 0;
  };
  int it = 0;
  double objective = 0.0, last_objective = 0.0, least_objective = 0.0;
  int status = 0;
  for (;;) {
    st->it = ++it;
    GPRC_TRY(factor_B(inv.p, "GPC: I + sqrt(W) K sqrt(W) not positive definite"));
    GPRC_TRY(gpc_apply(m, st, b, a));
    GPRC_TRY(launch_row_reduce(s, Kf.p, n_pad, n_pad, n_pad, a, f, red.p));  // f <- K %*% a  :85
    GPRC_TRY(launch_gpc_objective(s, a, f, m->y, n, ctx->scal_dev));          // :86
    GPRC_HIP(hipMemcpyAsync(&objective, ctx->scal_dev, sizeof(double), hipMemcpyDeviceToHost, s));
    GPRC_HIP(hipStreamSynchronize(s));
    if (it > 1) {
      if (std::fabs(objective - last_objective) < epsilon) break;                          // :88
      else if ((flags & GPRC_GPC_REFERENCE_STOP) && least_objective + 10.0 < objective) { status = GPRC_ERR_DIVERGED; break; }  // :90
    } else {
      least_objective = objective;
    }
    last_objective = objective;
    if (it >= max_iter) { status = GPRC_ERR_MAXITER; break; }
  }
  st->objective = objective;
  if (status != 0) {
    set_error(status == GPRC_ERR_DIVERGED ? "Apparently does not converge." : "GPC: iteration cap reached");
    return status;
  }
  return factor_B(final_inv ? inv.p : nullptr, "GPC: final factorisation failed");   // final L from the converged f (:99-102)
}

// W (n_pad x n_pad, ld n_pad, lower triangle) := -V^T V = -(L L^T)^-1 from the model's factor, with V^T = I L^-T (the identity through
// the predict's solve in its triangular form, as gprc_fit_gradient; row tile r of V^T is zero left of column 128 r, so its products
// start there), n^3 / 3 flops each.  With m == nullptr only the two workspaces are claimed (slots 0 and 3: gprc_gpc_logq_grad before
// its mode search, so that a size that does not fit fails before any work); out of memory: GPRC_ERR_NOMEM with the text nomem() builds.
template <class NoMem>
int neg_inverse_from_factor(gprc_ctx* ctx, int64_t n_pad, const gprc_model* m, NoMem nomem, double** W_out) {
  hipStream_t s = ctx->stream;
  double *vt = nullptr, *W = nullptr;
  int rc = ws_get(ctx, 0, n_pad * n_pad, &vt);
  if (rc == 0) rc = ws_get(ctx, 3, n_pad * n_pad, &W);
  if (rc == GPRC_ERR_NOMEM) set_error(nomem());
  if (rc != 0 || !m) return rc;
  GPRC_TRY(launch_set_identity_rows(s, vt, n_pad, n_pad, n_pad, 0));
  GPRC_TRY(solve_rows(ctx, m->packed, m->winv, n_pad, vt, n_pad, n_pad, nullptr, 0));   // vt = L^-T (upper triangular)
  GPRC_HIP(hipMemsetAsync(W, 0, sizeof(double) * (size_t)(n_pad * n_pad), s));
  GPRC_TRY(launch_gemm_nt(s, W, n_pad, vt, n_pad, vt, n_pad, n_pad, n_pad, n_pad, 1, PK_INV_GEMM));
  *W_out = W;
  return 0;
}

template <class NoMem>   // the claim alone (gprc_gpc_logq_grad, before its mode search)
int claim_inverse_workspaces(gprc_ctx* ctx, int64_t n_pad, NoMem nomem) { double* W; return neg_inverse_from_factor(ctx, n_pad, nullptr, nomem, &W); }

// The tail of both exact gradients.  part: grad_partial_rows() x cols partial sums of the contraction (device); they are summed in row
// order in long double, the first n_params columns get the factors that do not depend on (i, j) (kernels_grad.hip), any further column
// is halved.  extra_dev (may be null): one more device scalar, fetched into *extra_host before the one synchronise.
int grad_from_partials(hipStream_t s, const double* part, int64_t cols, int kernel, const double* params, int n_params, double* grad_out,
                       const double* extra_dev = nullptr, double* extra_host = nullptr) {
  const int64_t rows = grad_partial_rows();
  std::vector<double> hp((size_t)(rows * cols));
  GPRC_HIP(hipMemcpyAsync(hp.data(), part, sizeof(double) * hp.size(), hipMemcpyDeviceToHost, s));
  if (extra_dev) GPRC_HIP(hipMemcpyAsync(extra_host, extra_dev, sizeof(double), hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipStreamSynchronize(s));
  std::vector<long double> acc((size_t)cols, 0.0L);
  for (int64_t g = 0; g < rows; ++g)
    for (int64_t k = 0; k < cols; ++k) acc[(size_t)k] += (long double)hp[(size_t)(g * cols + k)];
  const double p0 = params[0], p1 = n_params > 1 ? params[1] : 0.0;
  switch (kernel) {
    case GPRC_GAMMAEXP:
      grad_out[0] = (double)(0.5L * acc[0] * (long double)p1 / (long double)p0);
      grad_out[1] = (double)(-0.25L * acc[1]);
      break;
    case GPRC_RATQUAD: grad_out[1] = (double)(0.5L * acc[1]);   // and the length scale as sqrexp's:
    case GPRC_SQREXP: grad_out[0] = (double)(0.5L * acc[0] / ((long double)p0 * p0 * p0)); break;
    case GPRC_MATERN32: grad_out[0] = (double)(acc[0] / (2.0L * (long double)p0)); break;
    case GPRC_MATERN52: grad_out[0] = (double)(acc[0] / (6.0L * (long double)p0)); break;
    case GPRC_MATERN32_ARD:
      for (int k = 0; k < n_params; ++k) grad_out[k] = (double)(3.0L * acc[(size_t)k] / (2.0L * (long double)params[k]));
      break;
    case GPRC_MATERN52_ARD:
      for (int k = 0; k < n_params; ++k) grad_out[k] = (double)(5.0L * acc[(size_t)k] / (6.0L * (long double)params[k]));
      break;
    default:
      for (int k = 0; k < n_params; ++k) grad_out[k] = (double)(0.5L * acc[(size_t)k] / (long double)params[k]);
  }
  for (int64_t k = n_params; k < cols; ++k) grad_out[k] = (double)(0.5L * acc[(size_t)k]);
  return 0;
}

// The pointwise predict of ns test points, chunk by chunk (chunk_workspace); colscale as predict_chunk
int predict_pointwise(gprc_model* m, const double* xs, int64_t ns, const double* colscale, double* mean_out, double* var_out) {
  gprc_ctx* ctx = m->ctx;
  int64_t rows = 0;
  double *vt = nullptr, *part = nullptr, *tmp = nullptr;
  GPRC_TRY(chunk_workspace(ctx, m->n_pad, ns, true, &rows, &vt, &part, &tmp));
  const int64_t ldv = rows + ctx->vt_pad;  // one leading dimension for every chunk
  for (int64_t s0 = 0; s0 < ns; s0 += rows) {
    const int64_t mcur = (ns - s0 < rows) ? ns - s0 : rows;
    GPRC_TRY(predict_chunk(m, xs + s0 * m->d, mcur, vt, ldv, part, tmp, colscale, true, mean_out + s0, var_out + s0));
  }
  return 0;
}

// What the two predict entry points do around their work: the model's type and the pointers are checked, ns == 0 returns, X_star and
// the two outputs (ns and cnt2 doubles) are staged on the model's device, work(xs, out1, out2) runs, host outputs are copied back
template <class Work>
int predict_entry(gprc_model* m, int type, const char* not_type, const char* bad_args, const double* X_star, int64_t ns, double* out1,
                  double* out2, int64_t cnt2, Work work) {
  if (!m || m->type != type) { set_error(not_type); return GPRC_ERR_ARG; }
  if (ns < 0 || (ns > 0 && (!X_star || !out1 || !out2))) { set_error(bad_args); return GPRC_ERR_ARG; }
  if (ns == 0) return 0;
  GPRC_TRY(use_device(m->ctx));
  hipStream_t s = m->ctx->stream;
  In xs;
  Out a, b;
  GPRC_TRY(xs.set(s, X_star, m->d * ns));
  GPRC_TRY(a.set(out1, ns));
  GPRC_TRY(b.set(out2, cnt2));
  GPRC_TRY(work(xs.dev, a.dev, b.dev));
  return finish_sync(s, a, b);
}

// diag((L L^T)^-1) of a factored model, kinv_i = sum_k (L^-1)_ki^2 for i < n (kinv: n_pad doubles; entries past n may be written): the
// rows of the identity go through the predict's solve in its triangular form, chunk by chunk (n^3 / 3 over all chunks; GPRC_FITGRAD_DENSE=1:
// the dense n^3 form), the panel solves leave the per-block sums of squares and launch_sum_partials adds them in block order.  No n^2
// buffer beyond the chunk; a row's arithmetic depends on columns only, so the result does not depend on the chunking, bit for bit.
// Shared by gprc_fit_gradient and gprc_gpr_loo.
int inverse_diagonal(gprc_model* m, double* kinv) {
  gprc_ctx* ctx = m->ctx;
  hipStream_t s = ctx->stream;
  const int64_t n = m->n, n_pad = m->n_pad;
  int64_t rows = 0;
  double *vt = nullptr, *red = nullptr, *unused = nullptr;
  GPRC_TRY(chunk_workspace(ctx, n_pad, n, false, &rows, &vt, &red, &unused));
  for (int64_t s0 = 0; s0 < n; s0 += rows) {
    const int64_t mcur = std::min<int64_t>(rows, n - s0), m_pad = pad_up(mcur, 128);
    GPRC_TRY(launch_set_identity_rows(s, vt, m_pad, m_pad, n_pad, s0));
    const bool dense = identity_solve_dense();
    if (!dense) GPRC_HIP(hipMemsetAsync(red, 0, sizeof(double) * (size_t)(m_pad * (n_pad / NBI)), s));
    GPRC_TRY(solve_rows(ctx, m->packed, m->winv, n_pad, vt, m_pad, m_pad, red, dense ? -1 : s0));
    GPRC_TRY(launch_sum_partials(s, red, n_pad / NBI, m_pad, m_pad, nullptr, kinv + s0));  // writes m_pad entries: kinv has n_pad
  }
  return 0;
}

}  // namespace

// The reversed factor of a model (kernels_vec.hip, reverse_factor_kernel), built on the first call that needs it and kept
// (gprc_gpr_predict_grad here, gprc_gpr_paths_create in gprc_paths.hip)
int ensure_reversed_factor(gprc_model* m) {
  if (m->packed_rev && m->winv_rev) return 0;
  gprc_ctx* ctx = m->ctx;
  const size_t pb = sizeof(double) * (size_t)gprc_packed_size(m->n_pad), wb = sizeof(double) * (size_t)gprc_winv_size(m->n_pad);
  void *pr = nullptr, *wr = nullptr;
  int rc = pool_alloc(ctx, pb, &pr);
  if (rc == 0 && (rc = pool_alloc(ctx, wb, &wr)) != 0) pool_release(ctx, pr, pb);
  if (rc != 0) {
    if (rc == GPRC_ERR_NOMEM)
      set_error("predict_grad: the variance's gradient needs a second copy of the factor, " + std::to_string((pb + wb) >> 20) +
                " MiB of device memory, which could not be allocated (the model is unchanged; mean, variance and the mean's gradient need none)");
    return rc;
  }
  rc = launch_reverse_factor(ctx->stream, m->packed, m->winv, m->n_pad, (double*)pr, (double*)wr);
  if (rc != 0) { pool_release(ctx, pr, pb); pool_release(ctx, wr, wb); return rc; }
  m->packed_rev = (double*)pr;
  m->winv_rev = (double*)wr;
  return 0;
}

}  // namespace gprc

using namespace gprc;

extern "C" {

// ---- GPR ----------------------------------------------------------------------------------------
int gprc_gpr_fit(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d,
                 int64_t n, const double* y, double noise, gprc_model** model_out) {
  ModelPtr m;
  GPRC_TRY(gpr_fit_once(ctx, kernel, params, n_params, X, d, n, y, noise, m, model_out != nullptr));
  *model_out = m.release();
  return 0;
}

int gprc_gpr_log_marginal(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d,
                          int64_t n, const double* y, double noise, double* logp_out) {
  if (!logp_out) { set_error("log_marginal: null output"); return GPRC_ERR_ARG; }
  ModelPtr m;
  GPRC_TRY(gpr_fit_once(ctx, kernel, params, n_params, X, d, n, y, noise, m));
  *logp_out = m->logp;
  return 0;
}

// dens_deriv(v) of R/fit.R:126-139, quirks included: K is the NOISE-FREE kernel matrix, alpha = K^-1 y, and
//   grad_i = 0.5 * sum( diag(alpha alpha^T - K^-1) %*% dK/dv_i )  =  0.5 * sum_r (alpha_r^2 - (K^-1)_rr) * rowsum_r(dK/dv_i)
// (a vector-matrix product where a trace is meant; `deriv` binds v positionally in its own argument order).
// The reference inverts K with solve() (LU); here K = L L^T (K must be numerically positive definite, else info > 0,
// which the host treats like solve()'s "computationally singular" error) and diag(K^-1)_r = sum_k (L^-1)_kr^2.
int gprc_fit_gradient(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n,
                      const double* y, double* grad_out) {
  if (!grad_out) { set_error("fit_gradient: null output"); return GPRC_ERR_ARG; }
  if (kernel != GPRC_SQREXP && kernel != GPRC_GAMMAEXP && kernel != GPRC_POLYNOMIAL && kernel != GPRC_RATQUAD) {
    set_error("fit_gradient: defined for sqrexp, gammaexp, polynomial, rationalquadratic (R/fit.R:125)");
    return GPRC_ERR_ARG;
  }
  ModelPtr m;
  GPRC_TRY(gpr_prepare(ctx, kernel, params, n_params, X, d, n, y, 0.0, m));
  int info = 0;
  GPRC_TRY(gpr_attempt(m.get(), 0.0, &info));  // L, alpha = K^-1 y
  if (info != 0) { set_error("fit_gradient: K is not positive definite (leading minor " + std::to_string(info) + ")"); return info; }
  hipStream_t s = ctx->stream;
  const int64_t n_pad = m->n_pad;
  const int n_deriv = n_params;  // 1 (sqrexp) or 2
  DevMem kinv, S;
  GPRC_TRY(kinv.alloc(n_pad));
  GPRC_TRY(S.alloc(2 * n));
  GPRC_TRY(inverse_diagonal(m.get(), kinv.p));
  GPRC_TRY(launch_deriv_rowsum(s, kernel, params[0], n_params > 1 ? params[1] : 0.0, m->X, d, n, S.p));
  std::vector<double> ha(n), hk(n), hs(2 * n);
  GPRC_HIP(hipMemcpyAsync(ha.data(), m->alpha, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipMemcpyAsync(hk.data(), kinv.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipMemcpyAsync(hs.data(), S.p, sizeof(double) * n_deriv * n, hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipStreamSynchronize(s));
  for (int i = 0; i < n_deriv; ++i) {
    long double acc = 0.0L;
    for (int64_t r = 0; r < n; ++r) acc += (long double)(ha[r] * ha[r] - hk[r]) * (long double)hs[(int64_t)i * n + r];
    grad_out[i] = (double)(0.5L * acc);
  }
  return 0;
}

// logp and its exact gradient ("Exact gradient and ARD"):
//   fit                    L, alpha, logp                                     as gprc_gpr_log_marginal          n^3 / 3
//   W = -V^T V = -K_y^-1   neg_inverse_from_factor: V^T = I L^-T, then the lower triangle of the product     2 x n^3 / 3
//   contraction            one pass over W with K, dK / dtheta recomputed from X (kernels_grad.hip); host: sum of the partials
int gprc_gpr_logp_grad(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n,
                       const double* y, double noise, double* logp_out, double* grad_out) {
  if (!logp_out || !grad_out) { set_error("logp_grad: null output"); return GPRC_ERR_ARG; }
  GPRC_TRY(check_grad_kernel("logp_grad", kernel));
  ModelPtr m;
  GPRC_TRY(gpr_fit_once(ctx, kernel, params, n_params, X, d, n, y, noise, m));
  hipStream_t s = ctx->stream;
  const int64_t n_pad = m->n_pad;
  double* W = nullptr;
  const auto nomem = [&] {
    return "logp_grad: L^-1 and (K + noise I)^-1 are held whole, 2 x " + std::to_string(n_pad) + "^2 doubles (" +
           std::to_string((2 * n_pad * n_pad * (int64_t)sizeof(double)) >> 20) + " MiB) of device memory, which could not be allocated";
  };
  GPRC_TRY(neg_inverse_from_factor(ctx, n_pad, m.get(), nomem, &W));
  DevMem part;
  GPRC_TRY(part.alloc(grad_partial_rows() * (n_params + 1)));
  GPRC_TRY(launch_grad_contract(s, m->ks, m->X, d, n, m->alpha, W, n_pad, part.p));
  GPRC_TRY(grad_from_partials(s, part.p, n_params + 1, kernel, params, n_params, grad_out));   // the last column: the noise variance
  *logp_out = m->logp;
  return 0;
}

// Leave-one-out predictions of a fitted model ("Leave-one-out cross-validation"): p = diag(K_y^-1) as
// gprc_fit_gradient computes it (inverse_diagonal: n^3 / 3, no n^2 buffer), then one elementwise pass; the call only reads the model
int gprc_gpr_loo(gprc_model* m, double* mean_out, double* var_out, double* logdens_out, double* loo_out) {
  if (!m || m->type != MODEL_GPR) { set_error("loo: not a GPR model"); return GPRC_ERR_ARG; }
  if (!mean_out && !var_out && !logdens_out && !loo_out) { set_error("loo: all four outputs are null"); return GPRC_ERR_ARG; }
  GPRC_TRY(ctx_gone("loo", *m));
  gprc_ctx* ctx = m->ctx;
  GPRC_TRY(use_device(ctx));
  hipStream_t s = ctx->stream;
  const int64_t n = m->n, n_pad = m->n_pad;
  Out om, ov, ol;
  if (mean_out) GPRC_TRY(om.set(mean_out, n));
  if (var_out) GPRC_TRY(ov.set(var_out, n));
  if (logdens_out) GPRC_TRY(ol.set(logdens_out, n));
  DevMem kinv, ell;
  GPRC_TRY(kinv.alloc(n_pad));
  if (loo_out && !logdens_out) GPRC_TRY(ell.alloc(n));
  double* ell_dev = logdens_out ? ol.dev : ell.p;
  GPRC_TRY(inverse_diagonal(m, kinv.p));
  GPRC_TRY(launch_loo_point(s, m->alpha, m->y, kinv.p, nullptr, 0, n, n_pad, om.dev, ov.dev, ell_dev, nullptr, nullptr, nullptr));
  std::vector<double> hl(loo_out ? (size_t)n : 0);
  if (loo_out) GPRC_HIP(hipMemcpyAsync(hl.data(), ell_dev, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  GPRC_TRY(finish_sync(s, om, ov, ol));
  if (loo_out) *loo_out = sum_in_order(hl.data(), n);
  return 0;
}

// The LOO log score and its exact gradient ("Leave-one-out cross-validation"):
//   fit                    L, alpha                                           as gprc_gpr_log_marginal                    n^3 / 3
//   W = -P = -K_y^-1       neg_inverse_from_factor (lower, slot 3; slot 0 is free afterwards)                          2 x n^3 / 3
//   vectors                p = -diag(W): ell, w = alpha / p, sqrt(c); u = P w by the two vector solves with L
//   Q = P diag(sqrt c)     the full matrix, mirrored through LDS into slot 0 (zero columns in the padding)
//   S = -Q Q^T             W := 0, then the lower triangle of C -= A B^T on the MFMA tile core                            n^3
//   contraction            M = u alpha^T + alpha u^T + S is the Laplace form with a = 0, sw = 1, g = alpha, W = S (0 * 0 + (1 * 1) S_ij is exact)
//   noise                  1/2 sum_i M_ii = sum_i (u_i alpha_i + 1/2 S_ii), summed on the host in index order
int gprc_gpr_loo_grad(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n,
                      const double* y, double noise, double* loo_out, double* grad_out) {
  if (!loo_out || !grad_out) { set_error("loo_grad: null output"); return GPRC_ERR_ARG; }
  GPRC_TRY(check_grad_kernel("loo_grad", kernel));
  ModelPtr m;
  GPRC_TRY(gpr_fit_once(ctx, kernel, params, n_params, X, d, n, y, noise, m));
  hipStream_t s = ctx->stream;
  const int64_t n_pad = m->n_pad;
  double *W = nullptr, *Q = nullptr;
  const auto nomem = [&] {
    return "loo_grad: (K + noise I)^-1 and its column-scaled full copy are held whole, 2 x " + std::to_string(n_pad) + "^2 doubles (" +
           std::to_string((2 * n_pad * n_pad * (int64_t)sizeof(double)) >> 20) + " MiB) of device memory, which could not be allocated";
  };
  GPRC_TRY(neg_inverse_from_factor(ctx, n_pad, m.get(), nomem, &W));
  GPRC_TRY(ws_get(ctx, 0, n_pad * n_pad, &Q));   // L^-T has been consumed
  DevMem vec, inv, part;
  GPRC_TRY(vec.alloc(5 * n_pad));
  GPRC_TRY(inv.alloc(gprc_solve_inv_size(n_pad)));
  GPRC_TRY(part.alloc(grad_partial_rows() * n_params));
  double *u = vec.p, *sc = vec.p + n_pad, *one = vec.p + 2 * n_pad, *zero = vec.p + 3 * n_pad, *terms = vec.p + 4 * n_pad;
  GPRC_HIP(hipMemsetAsync(zero, 0, sizeof(double) * (size_t)(2 * n_pad), s));   // and the terms' tail
  GPRC_TRY(launch_loo_point(s, m->alpha, m->y, nullptr, W, n_pad, n, n_pad, nullptr, nullptr, terms, u, sc, one));   // terms: ell for now
  std::vector<double> he((size_t)n), ht((size_t)n);
  GPRC_HIP(hipMemcpyAsync(he.data(), terms, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  GPRC_TRY(launch_inv512(s, m->packed, n_pad, m->winv, inv.p, 0, n_pad / NB));
  GPRC_TRY(launch_trsv(s, m->packed, inv.p, n_pad, u, 0, m->work));   // u = L^-T L^-1 w
  GPRC_TRY(launch_trsv(s, m->packed, inv.p, n_pad, u, 1, m->work));
  GPRC_TRY(launch_loo_q(s, W, sc, n_pad, Q));
  GPRC_HIP(hipMemsetAsync(W, 0, sizeof(double) * (size_t)(n_pad * n_pad), s));
  GPRC_TRY(launch_gemm_nt(s, W, n_pad, Q, n_pad, Q, n_pad, n_pad, n_pad, n_pad, 1, PK_COV_SYRK));   // S = -Q Q^T (lower)
  GPRC_TRY(launch_loo_noise_terms(s, u, m->alpha, W, n_pad, n, terms));
  GPRC_HIP(hipMemcpyAsync(ht.data(), terms, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  GPRC_TRY(launch_gpc_grad_contract(s, m->ks, m->X, d, n, zero, one, u, m->alpha, W, n_pad, part.p));
  GPRC_TRY(grad_from_partials(s, part.p, n_params, kernel, params, n_params, grad_out));   // synchronises: he and ht have arrived
  grad_out[n_params] = sum_in_order(ht.data(), n);
  *loo_out = sum_in_order(he.data(), n);
  return 0;
}

int gprc_gpr_fit_retry(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d,
                       int64_t n, const double* y, double noise, gprc_model** model_out, double* noise_used,
                       int* attempts) {
  ModelPtr m;
  GPRC_TRY(gpr_prepare(ctx, kernel, params, n_params, X, d, n, y, noise, m, model_out != nullptr));
  double new_noise = noise;
  for (int i = 1; i <= 10; ++i) {  // R/GPRclass.R:141-148
    int info = 0;
    GPRC_TRY(gpr_attempt(m.get(), new_noise, &info));
    if (info == 0) {
      if (noise_used) *noise_used = new_noise;
      if (attempts) *attempts = i;
      *model_out = m.release();
      return 0;
    }
    new_noise = 0.01 * i + noise;
  }
  if (attempts) *attempts = 10;
  set_error("Inputs lead to non positive definite covariance matrix. Try using a larger noise or a smaller lengthscale.");
  return GPRC_ERR_NOT_PD;
}

int gprc_gpr_predict(gprc_model* m, const double* X_star, int64_t ns, int pointwise, double* mean_out, double* var_out) {
  return predict_entry(m, MODEL_GPR, "predict: not a GPR model", "predict: bad arguments", X_star, ns, mean_out, var_out, pointwise ? ns : ns * ns,
                       [&](const double* xs, double* mean, double* var) -> int {
    if (pointwise) return predict_pointwise(m, xs, ns, nullptr, mean, var);
    // the full covariance needs all of v at once: no chunking to fall back on
    gprc_ctx* ctx = m->ctx;
    hipStream_t s = ctx->stream;
    const int64_t n_pad = m->n_pad, d = m->d, m_pad = pad_up(ns, PT_R), ldv = m_pad + ctx->vt_pad;
    double *vt = nullptr, *part = nullptr, *kss = nullptr, *cov = nullptr;
    GPRC_TRY(ws_get(ctx, 0, ldv * n_pad, &vt));
    GPRC_TRY(ws_get(ctx, 1, m_pad * predict_partials(n_pad), &part));
    GPRC_TRY(ws_get(ctx, 2, m_pad, &kss));
    GPRC_TRY(ws_get(ctx, 3, m_pad * m_pad, &cov));
    GPRC_TRY(predict_chunk(m, xs, ns, vt, ldv, part, kss, nullptr, true, mean, nullptr));
    GPRC_TRY(launch_fill(s, m->ks, xs, ns, xs, ns, d, cov, m_pad, 0, m_pad, 0, m_pad, PAD_ZERO, 0.0));  // :167
    GPRC_TRY(launch_gemm_nt(s, cov, m_pad, vt, ldv, vt, ldv, m_pad, m_pad, n_pad, 0, PK_COV_SYRK));      // - t(v) %*% v
    GPRC_HIP(hipMemcpy2DAsync(var, sizeof(double) * ns, cov, sizeof(double) * m_pad, sizeof(double) * ns, ns, hipMemcpyDeviceToDevice, s));
    GPRC_HIP(hipStreamSynchronize(s));  // cov goes out of scope
    return 0;
  });
}

// mean, variance and their gradients with respect to the test points ("Prediction gradients"), chunk by chunk
int gprc_gpr_predict_grad(gprc_model* m, const double* X_star, int64_t ns, double* mean_out, double* var_out, double* dmean_out, double* dvar_out) {
  if (!m || m->type != MODEL_GPR) { set_error("predict_grad: not a GPR model"); return GPRC_ERR_ARG; }
  if (m->borrowed) {
    set_error("predict_grad: the model borrows its buffers (gprc_gpr_model_from_device / gprc_mgpu_model_rank) and cannot own a reversed factor");
    return GPRC_ERR_ARG;
  }
  if (ns < 1 || !X_star) { set_error("predict_grad: bad arguments (n_star >= 1, non-null X_star)"); return GPRC_ERR_ARG; }
  if (!mean_out && !var_out && !dmean_out && !dvar_out) { set_error("predict_grad: all four outputs are null"); return GPRC_ERR_ARG; }
  GPRC_TRY(check_grad_kernel("predict_grad", m->ks.id));
  GPRC_TRY(ctx_gone("predict_grad", *m));
  gprc_ctx* ctx = m->ctx;
  GPRC_TRY(use_device(ctx));
  hipStream_t s = ctx->stream;
  const int64_t d = m->d, n_pad = m->n_pad;
  In xs;
  Out om, ov, odm, odv;
  GPRC_TRY(xs.set(s, X_star, d * ns));
  if (mean_out) GPRC_TRY(om.set(mean_out, ns));
  if (var_out) GPRC_TRY(ov.set(var_out, ns));
  if (dmean_out) GPRC_TRY(odm.set(dmean_out, d * ns));
  if (dvar_out) GPRC_TRY(odv.set(dvar_out, d * ns));
  if (dvar_out) GPRC_TRY(ensure_reversed_factor(m));
  int64_t rows = std::min<int64_t>(pad_up(ns, PT_R), 32768);   // the mean's gradient alone: no chunk of K* exists, only the partials
  double *vt = nullptr, *part = nullptr, *tmp = nullptr;
  if (mean_out || var_out || dvar_out) GPRC_TRY(chunk_workspace(ctx, n_pad, ns, true, &rows, &vt, &part, &tmp));
  const int64_t ldv = rows + ctx->vt_pad;
  const int64_t pcount = pred_grad_stripes(n_pad) * d * rows;
  DevMem pmean, pvar;
  if (dmean_out) GPRC_TRY(pmean.alloc(pcount));
  if (dvar_out) GPRC_TRY(pvar.alloc(pcount));
  for (int64_t s0 = 0; s0 < ns; s0 += rows) {
    const int64_t mcur = std::min<int64_t>(rows, ns - s0);
    GPRC_TRY(predict_chunk(m, xs.dev + s0 * d, mcur, vt, ldv, part, tmp, nullptr, false, mean_out ? om.dev + s0 : nullptr,
                           var_out ? ov.dev + s0 : nullptr, pmean.p, pvar.p, dmean_out ? odm.dev + s0 * d : nullptr, dvar_out ? odv.dev + s0 * d : nullptr));
  }
  return finish_sync(s, om, ov, odm, odv);
}

int gprc_gpr_extend(gprc_model* m, const double* X_new, int64_t mnew, const double* y_new) {
  if (!m) { set_error("extend: null model"); return GPRC_ERR_ARG; }
  if (m->type != MODEL_GPR) { set_error("extend: not a GPR model (a GPC fit must iterate again: refit)"); return GPRC_ERR_ARG; }
  if (m->borrowed) {
    set_error("extend: the model borrows its buffers (gprc_gpr_model_from_device / gprc_mgpu_model_rank); refit on the concatenated data");
    return GPRC_ERR_ARG;
  }
  if (mnew < 1 || !X_new || !y_new) { set_error("extend: bad arguments (m >= 1 observations, non-null X_new and y_new)"); return GPRC_ERR_ARG; }
  GPRC_TRY(ctx_gone("extend", *m));
  GPRC_TRY(use_device(m->ctx));
  int info = 0;
  GPRC_TRY(gpr_extend(m, X_new, mnew, y_new, &info));
  if (info != 0) {
    set_error("extend: the leading minor of order " + std::to_string(info) + " is not positive definite (model unchanged)");
    return info;
  }
  return 0;
}

int gprc_model_dims(const gprc_model* m, int64_t* n_out, int64_t* d_out) {
  if (!m) { set_error("null model"); return GPRC_ERR_ARG; }
  if (n_out) *n_out = m->n;
  if (d_out) *d_out = m->d;
  return 0;
}

int gprc_model_get_L(gprc_model* m, double* L_out, int64_t ld_out) {
  if (!m || !L_out || ld_out < m->n) { set_error("get_L: bad arguments"); return GPRC_ERR_ARG; }
  if (m->type == MODEL_SGPR) { set_error("get_L: a sparse model holds two factors of inducing-point size, not the factor of K + noise I"); return GPRC_ERR_ARG; }
  if (m->type == MODEL_IGPR) { set_error("get_L: an iterative model holds no factor"); return GPRC_ERR_ARG; }
  GPRC_TRY(use_device(m->ctx));
  hipStream_t s = m->ctx->stream;
  const int64_t n = m->n;
  Out o;   // host output: only the n x n block of the caller's array is written
  GPRC_TRY(o.set(L_out, ld_out, n, n));
  GPRC_TRY(launch_unpack_L(s, m->packed, m->n_pad, n, o.dev, o.ld));
  return finish_sync(s, o);
}

// the getters of a model of `type`: a vector field (n doubles, device to wherever dst points) or a scalar field
static int get_vector(gprc_model* m, int type, const char* not_type, double* gprc_model::*field, double* dst) {
  if (!m || m->type != type) { set_error(not_type); return GPRC_ERR_ARG; }
  if (!dst || !(m->*field)) { set_error("bad arguments"); return GPRC_ERR_ARG; }
  GPRC_TRY(use_device(m->ctx));
  GPRC_HIP(hipMemcpyAsync(dst, m->*field, sizeof(double) * m->n, hipMemcpyDefault, m->ctx->stream));
  GPRC_HIP(hipStreamSynchronize(m->ctx->stream));
  return 0;
}
static int get_scalar(const gprc_model* m, int type, const char* not_type, double gprc_model::*field, double* out) {
  if (!m || m->type != type || !out) { set_error(not_type); return GPRC_ERR_ARG; }
  *out = m->*field;
  return 0;
}
int gprc_gpr_get_alpha(gprc_model* m, double* alpha_out) { return get_vector(m, MODEL_GPR, "not a GPR model", &gprc_model::alpha, alpha_out); }
int gprc_gpr_get_logp(gprc_model* m, double* logp_out) { return get_scalar(m, MODEL_GPR, "not a GPR model", &gprc_model::logp, logp_out); }
int gprc_gpr_get_noise(gprc_model* m, double* noise_out) { return get_scalar(m, MODEL_GPR, "not a GPR model", &gprc_model::noise, noise_out); }
int gprc_model_free(gprc_model* m) { return free_bound(m, free_model); }   // ctx == nullptr: the buffers go straight back to the driver

// ---- GPC ----------------------------------------------------------------------------------------
int gprc_gpc_fit(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d,
                 int64_t n, const double* y, double epsilon, int max_iter, int flags, gprc_model** model_out,
                 int* iters_out) {
  ModelPtr m;
  GPRC_TRY(begin_model("fit", MODEL_GPC, ctx, kernel, params, n_params, X, d, n, y, model_out != nullptr,
                       epsilon > 0.0 ? nullptr : "epsilon must be > 0", m));  // R/GPCclass.R:68
  hipStream_t s = ctx->stream;
  GpcMode st;
  const int rc = gpc_mode_search(m.get(), X, y, epsilon, max_iter, flags, false, &st);
  if (iters_out && st.it > 0) *iters_out = st.it;   // stored before a failure is reported
  GPRC_TRY(rc);
  // logq = objective - sum(diag(L)) (:103, sic)
  double dsum = 0.0;
  GPRC_TRY(launch_diag_sum(s, m->packed, m->n_pad, n, ctx->scal_dev));
  GPRC_HIP(hipMemcpyAsync(&dsum, ctx->scal_dev, sizeof(double), hipMemcpyDeviceToHost, s));
  GPRC_TRY(launch_gpc_grad(s, m->f_hat, m->y, n, m->alpha, m->sw));  // g = (y+1)/2 - P, sw = sqrt(P(1-P)) for predict
  GPRC_HIP(hipStreamSynchronize(s));
  m->logq = st.objective - dsum;
  *model_out = m.release();
  return 0;
}

// log q(y | X, theta) of the Laplace approximation and its exact gradient ("GPC evidence gradient"):
//   mode search            the loop of gprc_gpc_fit (flags 0); K stays; final B = L L^T at the mode with the solve inverses
//   W = -V^T V = -B^-1     neg_inverse_from_factor: V^T = I L^-T, then the lower triangle of the product (PK_INV_GEMM)     2 x n^3 / 3
//   vectors                s2 from diag(W); u = s2 - sw B^-1 sw (K s2): one K-matvec, two vector solves
//   contraction            one pass over W, M = a a^T + sw sw^T o W + u g^T + g u^T, K and dK / dtheta recomputed from X (kernels_grad.hip)
int gprc_gpc_logq_grad(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n,
                       const double* y, double epsilon, int max_iter, double* logq_out, double* grad_out, int* iters_out) {
  if (!logq_out || !grad_out) { set_error("logq_grad: null output"); return GPRC_ERR_ARG; }
  GPRC_TRY(check_grad_kernel("logq_grad", kernel));
  const int64_t n_pad = pad_up(n, NB);
  const auto nomem = [&] {
    return "logq_grad: K, the factor, L^-1 and B^-1 are held whole, about 3.5 x " + std::to_string(n_pad) + "^2 doubles (" +
           std::to_string((7 * n_pad * n_pad * (int64_t)sizeof(double) / 2) >> 20) + " MiB) of device memory, which could not be allocated";
  };
  const auto or_nomem = [&](int rc) { if (rc == GPRC_ERR_NOMEM) set_error(nomem()); return rc; };
  ModelPtr m;
  GPRC_TRY(or_nomem(begin_model("logq_grad", MODEL_GPC, ctx, kernel, params, n_params, X, d, n, y, true,
                                epsilon > 0.0 ? nullptr : "epsilon must be > 0", m)));
  hipStream_t s = ctx->stream;
  GPRC_TRY(claim_inverse_workspaces(ctx, n_pad, nomem));   // before the mode search: a size that does not fit fails before any work
  GpcMode st;
  const int rc = gpc_mode_search(m.get(), X, y, epsilon, max_iter, 0, true, &st);
  if (iters_out && st.it > 0) *iters_out = st.it;
  GPRC_TRY(or_nomem(rc));
  double* a = st.vec.p + 2 * n_pad;                  // K^-1 f_hat (the loop's a)
  double *s2 = st.vec.p, *u = st.vec.p + 3 * n_pad;  // b of the loop is free now
  double* g = m->alpha;
  GPRC_TRY(launch_diag_log_sum(s, m->packed, n_pad, n, ctx->scal_dev + 1));
  GPRC_TRY(launch_gpc_grad(s, m->f_hat, m->y, n, g, m->sw));                 // g = (y+1)/2 - P; sw as the final factorisation used it
  double* W = nullptr;
  GPRC_TRY(neg_inverse_from_factor(ctx, n_pad, m.get(), nomem, &W));
  GPRC_TRY(launch_gpc_s2(s, m->f_hat, W, n_pad, n, s2));
  GPRC_TRY(gpc_apply(m.get(), &st, s2, u));                                  // u = s2 - sw B^-1 sw K s2
  DevMem part;
  GPRC_TRY(part.alloc(grad_partial_rows() * n_params));
  GPRC_TRY(launch_gpc_grad_contract(s, m->ks, m->X, d, n, a, m->sw, u, g, W, n_pad, part.p));
  double lsum = 0.0;
  GPRC_TRY(grad_from_partials(s, part.p, n_params, kernel, params, n_params, grad_out, ctx->scal_dev + 1, &lsum));
  *logq_out = st.objective - lsum;
  return 0;
}

int gprc_gpc_predict_latent(gprc_model* m, const double* X_star, int64_t ns, double* fs_bar_out, double* Vfs_out) {
  // R/GPCclass.R:112-115: m->alpha holds g = (y+1)/2 - P, the stored columns are sqrt(W) * K_star
  return predict_entry(m, MODEL_GPC, "predict_latent: not a GPC model", "predict_latent: bad arguments", X_star, ns, fs_bar_out, Vfs_out, ns,
                       [&](const double* xs, double* fs, double* vf) { return predict_pointwise(m, xs, ns, m->sw, fs, vf); });
}

int gprc_gpc_predict_class(gprc_model* m, const double* X_star, int64_t ns, double* prob_out) {
  if (!m || m->type != MODEL_GPC) { set_error("predict_class: not a GPC model"); return GPRC_ERR_ARG; }
  if (ns < 0 || (ns > 0 && (!X_star || !prob_out))) { set_error("predict_class: bad arguments"); return GPRC_ERR_ARG; }
  if (ns == 0) return 0;
  DevMem lat;
  GPRC_TRY(use_device(m->ctx));
  GPRC_TRY(lat.alloc(2 * ns));
  GPRC_TRY(gprc_gpc_predict_latent(m, X_star, ns, lat.p, lat.p + ns));   // device outputs: used in place
  return gprc_class_probability(m->ctx, lat.p, lat.p + ns, ns, prob_out);
}

int gprc_gpc_get_f_hat(gprc_model* m, double* f_hat_out) { return get_vector(m, MODEL_GPC, "not a GPC model", &gprc_model::f_hat, f_hat_out); }
int gprc_gpc_get_logq(gprc_model* m, double* logq_out) { return get_scalar(m, MODEL_GPC, "not a GPC model", &gprc_model::logq, logq_out); }

// ---- sampling -----------------------------------------------------------------------------
int gprc_sym_eigen(gprc_ctx* ctx, const double* A, int64_t lda, int64_t m, double* values_out, double* vectors_out, int* sweeps_out) {
  GPRC_TRY(use_device_unless(ctx, !A || !values_out || m < 1 || lda < m, "sym_eigen: bad arguments"));
  hipStream_t s = ctx->stream;
  In a;
  Out vals, vecs;
  GPRC_TRY(a.set(s, A, lda * m));
  GPRC_TRY(vals.set(values_out, m));
  if (vectors_out) GPRC_TRY(vecs.set(vectors_out, m * m));
  DevMem V;
  IntMem permd;
  GPRC_TRY(V.alloc(m * m));
  std::vector<double> values;
  std::vector<int> perm;
  GPRC_TRY(sym_eigen_dev(ctx, a.dev, lda, m, V.p, values, perm, sweeps_out));
  std::vector<double> sorted(m);
  for (int64_t k = 0; k < m; ++k) sorted[k] = values[perm[k]];
  GPRC_HIP(hipMemcpyAsync(vals.dev, sorted.data(), sizeof(double) * m, hipMemcpyHostToDevice, s));
  if (vectors_out) {
    GPRC_HIP(hipMalloc(&permd.p, sizeof(int) * (size_t)m));
    GPRC_HIP(hipMemcpyAsync(permd.p, perm.data(), sizeof(int) * m, hipMemcpyHostToDevice, s));
    GPRC_TRY(launch_gather_scale_cols(s, V.p, (int)m, permd.p, nullptr, vecs.dev, m));
    GPRC_TRY(vecs.finish(s));
  }
  return finish_sync(s, vals);
}

int gprc_mvn_factor(gprc_ctx* ctx, const double* cov, int64_t ld, int64_t m, double tol, double* L_out, int* method_out) {
  GPRC_TRY(use_device_unless(ctx, !cov || !L_out || m < 1 || ld < m, "mvn_factor: bad arguments"));
  hipStream_t s = ctx->stream;
  In c;
  Out L;
  GPRC_TRY(c.set(s, cov, ld * m));
  GPRC_TRY(L.set(L_out, m * m));
  int method = 0;
  GPRC_TRY(mvn_factor_dev(ctx, c.dev, ld, m, tol, L.dev, &method));
  GPRC_TRY(finish_sync(s, L));
  if (method_out) *method_out = method;
  return 0;
}

int gprc_mvn_sample(gprc_ctx* ctx, const double* cov, int64_t ld, int64_t m, const double* mean, double tol, const double* Z,
                    int64_t n_draws, double* out, int* method_out) {
  GPRC_TRY(use_device_unless(ctx, !cov || !mean || !Z || !out || m < 1 || ld < m || n_draws < 1, "mvn_sample: bad arguments"));
  hipStream_t s = ctx->stream;
  In c, mu, z;
  Out o;
  GPRC_TRY(c.set(s, cov, ld * m));
  GPRC_TRY(mu.set(s, mean, m));
  GPRC_TRY(z.set(s, Z, m * n_draws));
  GPRC_TRY(o.set(out, m * n_draws));
  DevMem L;
  GPRC_TRY(L.alloc(m * m));
  int method = 0;
  GPRC_TRY(mvn_factor_dev(ctx, c.dev, ld, m, tol, L.p, &method));
  GPRC_TRY(launch_affine_lz(s, L.p, m, m, mu.dev, z.dev, m, n_draws, o.dev, m, method == 1));  // drop(mean) + L %*% Z  :369
  GPRC_TRY(finish_sync(s, o));
  if (method_out) *method_out = method;
  return 0;
}

int gprc_gpr_model_from_device(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X,
                               int64_t d, int64_t n, const double* y, double* packed, double* winv, double* alpha,
                               double noise, double logp, gprc_model** model_out) {
  GPRC_TRY(use_device_unless(ctx, !X || !y || !packed || !winv || !alpha || !model_out || d < 1 || n < 1, "model_from_device: bad arguments"));
  KernelSpec ks;
  GPRC_TRY(make_spec(kernel, params, n_params, d, &ks));
  gprc_model* m = new_model(ctx, MODEL_GPR, ks, n, d);
  if (!m) return GPRC_ERR_NOMEM;
  m->borrowed = true;
  m->X = const_cast<double*>(X); m->y = const_cast<double*>(y); m->packed = packed; m->winv = winv; m->alpha = alpha;
  m->noise = noise; m->logp = logp;
  *model_out = m;
  return 0;
}

}  // extern "C"
