// gprc_local.hip -- the local GPR ("Local GPR"): the host side of gprc_dev_knn and gprc_lgpr_*.  A test point is
// conditioned on its m <= 128 nearest training points only: the exact neighbour search of kernels_knn.hip, the gather into the strided
// slabs of the batched small models, then gprc_gpr_batch_fit and gprc_gpr_batch_predict (gprc_batch.hip) on device pointers -- one
// model per test point, one test point per model.  Nothing here factorises; the training set lives on the device once, in the object.
// A model, and so a test point, does not look at any other: its bits do not depend on n*, on the chunk it falls into or on its place.
// The Vecchia likelihood ("Vecchia likelihood"): gprc_dev_knn_before, and on the same object gprc_lgpr_vecchia_prepare
// (the conditioning sets, searched once and kept as n x m_cond indices), gprc_lgpr_vecchia_logp_grad (launches of kernels_vecchia.hip over
// chunks of GPRC_VECCHIA_CHUNK points, the groups' rows added in order in long double, 1/2 and cross_grad_finish once) and
// gprc_lgpr_vecchia_neighbours.
// The local classifier ("Batched and local GPC"): gprc_lgpc_* on the same object with a kind tag -- the same search
// and gather, then gprc_gpc_batch_fit, the latent prediction and the class probability, one Laplace classifier per test point.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "gprc_host.h"
#include "pair_tile.h"

using namespace gprc;

constexpr int64_t LGPR_CHUNK = 2048;   // test points per batched fit: 2048 x 128 KiB = 256 MiB of L^-1 at a time

enum LocalKind { LOCAL_GPR = 0, LOCAL_GPC = 1 };
struct gprc_local_model : Bound {
  int kind = LOCAL_GPR;
  double epsilon = 0.0;   // LOCAL_GPC: the mode search's stop threshold and its cap
  int max_iter = 0;
  int kernel = 0;
  std::vector<double> params;
  double noise = 0.0;
  int64_t n = 0, d = 0, m = 0;
  DevMem X;       // d x n
  DevMem y;       // n
  DevMem scale;   // d doubles, 1 / l_c: the search metric of an ARD kernel (not allocated otherwise: Euclidean)
  DevMem nbr;     // gprc_lgpr_vecchia_prepare: n rows of m_cond 32-bit indices, the conditioning sets, frozen until the next prepare
  int64_t m_cond = -1;   // -1: no prepare yet; 0: n = 1, nothing to keep
};

namespace {

// the queries of a search: the ns points at Xs, or (Xs null) the window [first, first + ns) of X itself, candidates below each
struct KnnQueries {
  const double* Xs;
  int64_t first, ns;
};

// the search on device pointers, asynchronous: the split, its workspace (released to the pool when this returns: the stream orders its reuse)
int knn_run(gprc_ctx* ctx, const double* X, int64_t d, int64_t n, const KnnQueries& q, const double* scale, int64_t m, int* idx, double* dist, int64_t ld) {
  int cus = 0;
  GPRC_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  int parts = 1;
  int64_t part_len = 0;
  knn_split(q.Xs ? n : q.first + q.ns, q.ns, cus, &parts, &part_len);
  DevMem work;
  if (parts > 1) GPRC_TRY(work.alloc((int64_t)knn_workspace_doubles(q.ns, (int)m, parts)));
  if (q.Xs) return launch_knn(ctx->stream, X, d, n, q.Xs, q.ns, scale, (int)m, idx, dist, ld, parts, part_len, work.p);
  return launch_knn_before(ctx->stream, X, d, q.first, q.ns, scale, (int)m, idx, dist, ld, parts, part_len, work.p);
}

int check_scale(const char* who, const double* scale, int64_t d) {
  for (int64_t c = 0; c < d; ++c)
    if (!(scale[c] > 0.0) || !std::isfinite(scale[c])) return bad(who, "scale[" + std::to_string(c) + "] must be finite and > 0");
  return 0;
}

// The checks of a call with work to do that the two gprc_dev_knn* entry points share.  (The 2^31 limit and ld_out < m are theirs too, but
// each stands between checks that differ -- of m, of the window -- and two can fire at once: they stay where they are.)
int knn_checks(const char* who, const int* idx_out, const double* scale, int64_t d) {
  if (!idx_out) return bad(who, "null output pointer (idx_out)");
  if (scale && is_device_ptr(scale)) return bad(who, "scale must be host memory");
  return scale ? check_scale(who, scale, d) : 0;
}

// idx / dist (rows of m, pitch ld_out, both host or both device; dist may be null) of the queries, which are on the device; synchronises
int knn_to_caller(const char* who, gprc_ctx* ctx, const double* Xdev, int64_t d, int64_t n, const KnnQueries& q, const double* scale_dev, int64_t m,
                  int* idx_out, double* dist_out, int64_t ld_out) {
  IntOut idx;
  GPRC_TRY(idx.set(idx_out, ld_out, q.ns, m));
  Out dist;
  if (dist_out) {
    if (is_device_ptr(dist_out) != (idx.host == nullptr)) return bad(who, "idx_out and dist_out must both be host or both be device memory");
    if (idx.host) GPRC_TRY(dist.set(dist_out, ld_out, m, q.ns));   // compact rows of m, copied back with the caller's pitch
    else dist.dev = dist_out;
  }
  GPRC_TRY(knn_run(ctx, Xdev, d, n, q, scale_dev, m, idx.dev, dist.dev, idx.ld));
  return finish_sync(ctx->stream, idx, dist);
}

int alive(const char* who, const gprc_local_model* m) {
  if (!m) return bad(who, "null model");
  return ctx_gone(who, *m);
}

// parameters and noise into the object; an ARD kernel's metric 1 / l_c to the device
int store_params(const char* who, gprc_local_model* m, const double* params, int n_params, double noise) {
  if (!params) return bad(who, "null input pointer (params)");
  if (!(noise >= 0.0) || !std::isfinite(noise)) return bad(who, "noise must be finite and >= 0");
  KernelSpec ks;
  GPRC_TRY(make_spec(m->kernel, params, n_params, m->d, &ks));
  if (is_ard(m->kernel)) {
    std::vector<double> sc((size_t)m->d);
    for (int64_t c = 0; c < m->d; ++c) sc[(size_t)c] = 1.0 / params[c];
    GPRC_TRY(check_scale(who, sc.data(), m->d));
    if (!m->scale.p) GPRC_TRY(m->scale.alloc(m->d));
    GPRC_HIP(hipMemcpyAsync(m->scale.p, sc.data(), sizeof(double) * sc.size(), hipMemcpyHostToDevice, m->ctx->stream));
    GPRC_HIP(hipStreamSynchronize(m->ctx->stream));   // sc leaves scope
  }
  m->params.assign(params, params + n_params);
  m->noise = noise;
  return 0;
}

// a regression call on a classifier, or the other way round
int local_kind(const char* who, const gprc_local_model* m, int kind) {
  if (m->kind == kind) return 0;
  return bad(who, kind == LOCAL_GPC ? "the model is a local regression (gprc_lgpr_create): use the gprc_lgpr_* calls"
                                    : "the model is a local classifier (gprc_lgpc_create): use the gprc_lgpc_* calls");
}

// what gprc_lgpr_create and gprc_lgpc_create share: the checks, the object with the training set on the device
int local_create(const char* who, int kind, gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n,
                 const double* y, double noise, int64_t m, double epsilon, int max_iter, gprc_local_model** model_out) {
  if (model_out) *model_out = nullptr;
  if (!ctx) return bad(who, "null context");
  GPRC_TRY(check_grad_kernel(who, kernel));
  if (!model_out) return bad(who, "null output pointer (model_out)");
  if (!X || !y) return bad(who, "null input pointer (X, y)");
  if (d < 1 || n < 1) return bad(who, "d < 1 or n < 1");
  if (n >= (int64_t(1) << 31)) return bad(who, "n >= 2^31: the neighbour indices are 32-bit");
  if (m < 1) return bad(who, "m < 1");
  if (kind == LOCAL_GPC) {
    if (!(epsilon > 0.0)) return bad(who, "epsilon must be > 0");
    if (max_iter > GPRC_BATCH_GPC_MAX_ITER) return bad(who, "max_iter > 1000");
  }
  GPRC_TRY(use_device(ctx));
  hipStream_t s = ctx->stream;
  std::unique_ptr<gprc_local_model, BoundDelete> mod(new gprc_local_model);
  mod->ctx = ctx;
  mod->ctx_id = ctx->id;
  mod->kind = kind;
  mod->epsilon = epsilon;
  mod->max_iter = max_iter;
  mod->kernel = kernel;
  mod->n = n;
  mod->d = d;
  mod->m = std::min<int64_t>(std::min<int64_t>(m, n), GPRC_BATCH_MAX_N);
  GPRC_TRY(store_params(who, mod.get(), params, n_params, noise));
  GPRC_TRY(mod->X.copy_from(s, X, d * n));
  GPRC_TRY(mod->y.copy_from(s, y, n));
  GPRC_HIP(hipStreamSynchronize(s));
  *model_out = mod.release();
  return 0;
}

}  // namespace

extern "C" {

int gprc_dev_knn(gprc_ctx* ctx, const double* X, int64_t d, int64_t n, const double* X_star, int64_t n_star, const double* scale, int64_t m, int* idx_out,
                 double* dist_out, int64_t ld_out) {
  const char* who = "dev_knn";
  if (!ctx) return bad(who, "null context");
  if (d < 1 || n < 1 || n_star < 0) return bad(who, "d < 1, n < 1 or n_star < 0");
  if (n >= (int64_t(1) << 31)) return bad(who, "n >= 2^31: the neighbour indices are 32-bit");
  if (m < 1 || m > n || m > GPRC_BATCH_MAX_N) return bad(who, "m = " + std::to_string(m) + " is outside 1 .. min(n, 128)");
  if (ld_out < m) return bad(who, "ld_out < m");
  if (n_star == 0) return 0;
  if (!X || !X_star) return bad(who, "null input pointer (X, X_star)");
  GPRC_TRY(knn_checks(who, idx_out, scale, d));
  GPRC_TRY(use_device(ctx));
  hipStream_t s = ctx->stream;
  In xin, sc, xs;
  GPRC_TRY(xin.set(s, X, d * n));
  if (scale) GPRC_TRY(sc.set(s, scale, d));
  GPRC_TRY(xs.set(s, X_star, d * n_star));
  return knn_to_caller(who, ctx, xin.dev, d, n, {xs.dev, 0, n_star}, sc.dev, m, idx_out, dist_out, ld_out);
}

int gprc_lgpr_create(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n, const double* y, double noise,
                     int64_t m, gprc_local_model** model_out) {
  return local_create("lgpr_create", LOCAL_GPR, ctx, kernel, params, n_params, X, d, n, y, noise, m, 0.0, 0, model_out);
}

int gprc_lgpr_set_params(gprc_local_model* m, const double* params, int n_params, double noise) {
  const char* who = "lgpr_set_params";
  GPRC_TRY(alive(who, m));
  GPRC_TRY(local_kind(who, m, LOCAL_GPR));
  GPRC_TRY(use_device(m->ctx));
  return store_params(who, m, params, n_params, noise);
}

int gprc_lgpr_neighbours(gprc_local_model* m, const double* X_star, int64_t n_star, int* idx_out, double* dist_out, int64_t ld_out) {
  const char* who = "lgpr_neighbours";
  GPRC_TRY(alive(who, m));
  if (n_star < 0) return bad(who, "n_star < 0");
  if (ld_out < m->m) return bad(who, "ld_out < m");
  if (n_star == 0) return 0;
  if (!X_star) return bad(who, "null input pointer (X_star)");
  if (!idx_out) return bad(who, "null output pointer (idx_out)");
  GPRC_TRY(use_device(m->ctx));
  In xs;
  GPRC_TRY(xs.set(m->ctx->stream, X_star, m->d * n_star));
  return knn_to_caller(who, m->ctx, m->X.p, m->d, m->n, {xs.dev, 0, n_star}, m->scale.p, m->m, idx_out, dist_out, ld_out);
}

int gprc_lgpr_predict(gprc_local_model* m, const double* X_star, int64_t n_star, double* mean_out, double* var_out, int* info_out) {
  const char* who = "lgpr_predict";
  GPRC_TRY(alive(who, m));
  GPRC_TRY(local_kind(who, m, LOCAL_GPR));
  if (n_star < 0) return bad(who, "n_star < 0");
  if (n_star == 0) return 0;
  if (!X_star) return bad(who, "null input pointer (X_star)");
  if (!mean_out) return bad(who, "null output pointer (mean_out)");
  if (info_out && is_device_ptr(info_out)) return bad(who, "info_out must be host memory");
  gprc_ctx* ctx = m->ctx;
  GPRC_TRY(use_device(ctx));
  hipStream_t s = ctx->stream;
  const int64_t d = m->d, k = m->m;
  const int n_params = (int)m->params.size();
  In xs;
  GPRC_TRY(xs.set(s, X_star, d * n_star));
  Out mean, var;
  GPRC_TRY(mean.set(mean_out, n_star));
  if (var_out) GPRC_TRY(var.set(var_out, n_star));
  const int64_t chunk = std::min<int64_t>(n_star, LGPR_CHUNK);
  // what every chunk's models share, once: the parameter rows and the noises of the batched fit, its host outputs
  std::vector<double> thetas((size_t)(chunk * n_params)), noises((size_t)chunk, m->noise), logp((size_t)chunk);
  for (int64_t b = 0; b < chunk; ++b) std::copy(m->params.begin(), m->params.end(), thetas.begin() + b * n_params);
  std::vector<int> info((size_t)chunk);
  DevMem idx, Xg, yg;
  GPRC_TRY(idx.alloc((chunk * k + 1) / 2));
  GPRC_TRY(Xg.alloc(chunk * d * k));
  GPRC_TRY(yg.alloc(chunk * k));
  int* idx_dev = reinterpret_cast<int*>(idx.p);
  for (int64_t j0 = 0; j0 < n_star; j0 += chunk) {
    const int64_t B = std::min<int64_t>(chunk, n_star - j0);
    const double* xs_c = xs.dev + j0 * d;
    GPRC_TRY(knn_run(ctx, m->X.p, d, m->n, {xs_c, 0, B}, m->scale.p, k, idx_dev, nullptr, k));
    GPRC_TRY(launch_knn_gather(s, idx_dev, k, m->X.p, m->y.p, d, B, k, Xg.p, yg.p));
    gprc_batch_model* fitted = nullptr;
    GPRC_TRY(gprc_gpr_batch_fit(ctx, m->kernel, B, thetas.data(), n_params, n_params, noises.data(), Xg.p, d, k, d * k, yg.p, k, nullptr, &fitted,
                                logp.data(), info.data()));
    // one test point per model, straight into the outputs; a flagged model's point is NaN
    const int rc = gprc_gpr_batch_predict(fitted, xs_c, 1, d, nullptr, mean.dev + j0, var_out ? var.dev + j0 : nullptr, 1);
    gprc_batch_model_free(fitted);
    GPRC_TRY(rc);
    if (info_out) std::copy(info.begin(), info.begin() + B, info_out + j0);
  }
  return finish_sync(s, mean, var);
}

int gprc_dev_knn_before(gprc_ctx* ctx, const double* X, int64_t d, int64_t n, int64_t first, int64_t count, const double* scale, int64_t m, int* idx_out,
                        double* dist_out, int64_t ld_out) {
  const char* who = "dev_knn_before";
  if (!ctx) return bad(who, "null context");
  if (d < 1 || n < 1) return bad(who, "d < 1 or n < 1");
  if (n >= (int64_t(1) << 31)) return bad(who, "n >= 2^31: the neighbour indices are 32-bit");
  if (m < 1 || m > GPRC_BATCH_MAX_N) return bad(who, "m = " + std::to_string(m) + " is outside 1 .. 128");
  if (first < 0 || count < 0 || first > n || count > n - first) return bad(who, "the window [first, first + count) is outside 0 .. n");
  if (ld_out < m) return bad(who, "ld_out < m");
  if (count == 0) return 0;
  if (!X) return bad(who, "null input pointer (X)");
  GPRC_TRY(knn_checks(who, idx_out, scale, d));
  GPRC_TRY(use_device(ctx));
  hipStream_t s = ctx->stream;
  In xin, sc;
  GPRC_TRY(xin.set(s, X, d * (first + count)));   // no column from first + count on is a candidate or a query
  if (scale) GPRC_TRY(sc.set(s, scale, d));
  return knn_to_caller(who, ctx, xin.dev, d, first + count, {nullptr, first, count}, sc.dev, m, idx_out, dist_out, ld_out);
}

int gprc_lgpr_vecchia_prepare(gprc_local_model* m, int64_t m_cond) {
  const char* who = "lgpr_vecchia_prepare";
  GPRC_TRY(alive(who, m));
  GPRC_TRY(local_kind(who, m, LOCAL_GPR));
  if (m_cond < 1 || m_cond > GPRC_BATCH_MAX_N - 1) return bad(who, "m_cond = " + std::to_string(m_cond) + " is outside 1 .. 127");
  gprc_ctx* ctx = m->ctx;
  GPRC_TRY(use_device(ctx));
  const int64_t mc = std::min<int64_t>(m_cond, m->n - 1);
  GPRC_HIP(hipStreamSynchronize(ctx->stream));
  m->nbr.reset();   // a second prepare replaces the first
  m->m_cond = -1;
  if (mc > 0) {
    GPRC_TRY(m->nbr.alloc((m->n * mc + 1) / 2));
    GPRC_TRY(knn_run(ctx, m->X.p, m->d, m->n, {nullptr, 0, m->n}, m->scale.p, mc, reinterpret_cast<int*>(m->nbr.p), nullptr, mc));
    GPRC_HIP(hipStreamSynchronize(ctx->stream));
  }
  m->m_cond = mc;
  return 0;
}

int gprc_lgpr_vecchia_neighbours(gprc_local_model* m, int* idx_out, int64_t ld_out) {
  const char* who = "lgpr_vecchia_neighbours";
  GPRC_TRY(alive(who, m));
  GPRC_TRY(local_kind(who, m, LOCAL_GPR));
  if (m->m_cond < 0) return bad(who, "no gprc_lgpr_vecchia_prepare yet");
  if (ld_out < m->m_cond) return bad(who, "ld_out < m_cond");
  if (m->m_cond == 0) return 0;
  if (!idx_out) return bad(who, "null output pointer (idx_out)");
  GPRC_TRY(use_device(m->ctx));
  GPRC_HIP(hipMemcpy2DAsync(idx_out, sizeof(int) * (size_t)ld_out, m->nbr.p, sizeof(int) * (size_t)m->m_cond, sizeof(int) * (size_t)m->m_cond, (size_t)m->n,
                            is_device_ptr(idx_out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, m->ctx->stream));
  GPRC_HIP(hipStreamSynchronize(m->ctx->stream));
  return 0;
}

int gprc_lgpr_vecchia_logp_grad(gprc_local_model* m, const double* params, int n_params, double noise, double* logp_out, double* grad_out, double* cond_out,
                                int64_t* flagged_out) {
  const char* who = "lgpr_vecchia_logp_grad";
  GPRC_TRY(alive(who, m));
  GPRC_TRY(local_kind(who, m, LOCAL_GPR));
  if (!params) return bad(who, "null input pointer (params)");
  if (!logp_out) return bad(who, "null output pointer (logp_out)");
  if (!(noise >= 0.0) || !std::isfinite(noise)) return bad(who, "noise must be finite and >= 0");
  if (m->m_cond < 0) return bad(who, "no gprc_lgpr_vecchia_prepare yet");
  if (grad_out && is_device_ptr(grad_out)) return bad(who, "grad_out must be host memory");
  KernelSpec ks;
  GPRC_TRY(make_spec(m->kernel, params, n_params, m->d, &ks));
  if (is_ard(m->kernel))
    for (int k = 0; k < n_params; ++k)
      if (!(1.0 / params[k] > 0.0) || !std::isfinite(1.0 / params[k])) return bad(who, "length scale " + std::to_string(k) + " must be finite and > 0");
  gprc_ctx* ctx = m->ctx;
  GPRC_TRY(use_device(ctx));
  hipStream_t s = ctx->stream;
  const int64_t n = m->n;
  const bool want_grad = grad_out != nullptr;
  const int stride = n_params + 2, grp_stride = stride + 1;
  const int64_t chunk = std::min<int64_t>(n, GPRC_VECCHIA_CHUNK), groups = (n + 255) / 256;
  static_assert(GPRC_VECCHIA_CHUNK % 256 == 0, "launches start at multiples of 256: the groups are those of the global index");
  const KernelSpec dspec = make_deriv_spec(ks);
  DevMem spec_dev, out, info, grp;
  GPRC_TRY(spec_dev.alloc((int64_t)((sizeof(KernelSpec) + 7) / 8)));
  GPRC_TRY(out.alloc(chunk * stride));
  GPRC_TRY(info.alloc((chunk + 1) / 2));
  GPRC_TRY(grp.alloc(groups * grp_stride));
  Out cond;
  if (cond_out) GPRC_TRY(cond.set(cond_out, n));
  GPRC_HIP(hipMemcpyAsync(spec_dev.p, &dspec, sizeof(KernelSpec), hipMemcpyHostToDevice, s));
  VecchiaArgs a{m->X.p, m->y.p, reinterpret_cast<const int*>(m->nbr.p), reinterpret_cast<const KernelSpec*>(spec_dev.p), out.p, reinterpret_cast<int*>(info.p),
                m->d, 0, noise, (int)m->m_cond, n_params, stride, want_grad ? 1 : 0};
  for (int64_t i0 = 0; i0 < n; i0 += chunk) {
    const int64_t count = std::min<int64_t>(chunk, n - i0);
    a.i0 = i0;
    GPRC_TRY(launch_vecchia(s, m->kernel, a, count));
    VecchiaReduceArgs r{out.p, reinterpret_cast<const int*>(info.p), grp.p + (i0 / 256) * grp_stride, cond_out ? cond.dev + i0 : nullptr, count, stride,
                        want_grad ? 1 : 0};
    GPRC_TRY(launch_vecchia_reduce(s, r));
  }
  std::vector<double> hgrp((size_t)(groups * grp_stride));
  GPRC_HIP(hipMemcpyAsync(hgrp.data(), grp.p, sizeof(double) * hgrp.size(), hipMemcpyDeviceToHost, s));   // waits for dspec's upload too
  GPRC_TRY(finish_sync(s, cond));
  // the groups' rows in order, in long double; 1/2 and the factors of cross_grad_finish once, after the sum over points
  long double value = 0.0L, flagged = 0.0L, dnoise = 0.0L;
  std::vector<long double> acc((size_t)n_params, 0.0L);
  for (int64_t g = 0; g < groups; ++g) {
    const double* row = hgrp.data() + g * grp_stride;
    value += (long double)row[0];
    flagged += (long double)row[stride];
    if (want_grad) {
      for (int k = 0; k < n_params; ++k) acc[(size_t)k] += (long double)row[1 + k];
      dnoise += (long double)row[1 + n_params];
    }
  }
  const bool any = flagged > 0.0L;
  *logp_out = any ? std::numeric_limits<double>::quiet_NaN() : (double)value;
  if (flagged_out) *flagged_out = (int64_t)flagged;
  if (want_grad) half_theta_grad(ks, acc.data(), dnoise, !any, n_params, grad_out);
  return 0;
}

int gprc_lgpc_create(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n, const double* y, int64_t m,
                     double epsilon, int max_iter, gprc_local_model** model_out) {
  return local_create("lgpc_create", LOCAL_GPC, ctx, kernel, params, n_params, X, d, n, y, 0.0, m, epsilon, max_iter, model_out);
}

int gprc_lgpc_set_params(gprc_local_model* m, const double* params, int n_params) {
  const char* who = "lgpc_set_params";
  GPRC_TRY(alive(who, m));
  GPRC_TRY(local_kind(who, m, LOCAL_GPC));
  GPRC_TRY(use_device(m->ctx));
  return store_params(who, m, params, n_params, 0.0);
}

int gprc_lgpc_predict(gprc_local_model* m, const double* X_star, int64_t n_star, double* fs_bar_out, double* Vfs_out, double* prob_out, int* iters_out,
                      int* info_out) {
  const char* who = "lgpc_predict";
  GPRC_TRY(alive(who, m));
  GPRC_TRY(local_kind(who, m, LOCAL_GPC));
  if (n_star < 0) return bad(who, "n_star < 0");
  if (n_star == 0) return 0;
  if (!X_star) return bad(who, "null input pointer (X_star)");
  if (!fs_bar_out && !Vfs_out && !prob_out) return bad(who, "null output pointers (fs_bar_out, Vfs_out, prob_out: not all three may be NULL)");
  if ((iters_out && is_device_ptr(iters_out)) || (info_out && is_device_ptr(info_out))) return bad(who, "iters_out and info_out must be host memory");
  gprc_ctx* ctx = m->ctx;
  GPRC_TRY(use_device(ctx));
  hipStream_t s = ctx->stream;
  const int64_t d = m->d, k = m->m;
  const int n_params = (int)m->params.size();
  In xs;
  GPRC_TRY(xs.set(s, X_star, d * n_star));
  Out fs, vf, prob;
  GPRC_TRY(fs.set_keeping(fs_bar_out, n_star, false, s));
  GPRC_TRY(vf.set_keeping(Vfs_out, n_star, false, s));
  GPRC_TRY(prob.set_keeping(prob_out, n_star, false, s));
  const int64_t chunk = std::min<int64_t>(n_star, LGPR_CHUNK);
  std::vector<double> thetas((size_t)(chunk * n_params)), logq((size_t)chunk);
  for (int64_t b = 0; b < chunk; ++b) std::copy(m->params.begin(), m->params.end(), thetas.begin() + b * n_params);
  std::vector<int> iters((size_t)chunk), info((size_t)chunk);
  DevMem idx, Xg, yg, fs_tmp, vf_tmp;   // the class probability needs both latent values, asked for or not
  GPRC_TRY(idx.alloc((chunk * k + 1) / 2));
  GPRC_TRY(Xg.alloc(chunk * d * k));
  GPRC_TRY(yg.alloc(chunk * k));
  if (prob_out && !fs_bar_out) GPRC_TRY(fs_tmp.alloc(chunk));
  if (prob_out && !Vfs_out) GPRC_TRY(vf_tmp.alloc(chunk));
  int* idx_dev = reinterpret_cast<int*>(idx.p);
  for (int64_t j0 = 0; j0 < n_star; j0 += chunk) {
    const int64_t B = std::min<int64_t>(chunk, n_star - j0);
    const double* xs_c = xs.dev + j0 * d;
    GPRC_TRY(knn_run(ctx, m->X.p, d, m->n, {xs_c, 0, B}, m->scale.p, k, idx_dev, nullptr, k));
    GPRC_TRY(launch_knn_gather(s, idx_dev, k, m->X.p, m->y.p, d, B, k, Xg.p, yg.p));
    gprc_batch_model* fitted = nullptr;
    GPRC_TRY(gprc_gpc_batch_fit(ctx, m->kernel, B, thetas.data(), n_params, n_params, Xg.p, d, k, d * k, yg.p, k, nullptr, m->epsilon, m->max_iter, &fitted,
                                logq.data(), iters.data(), info.data()));
    // one test point per model, straight into the outputs; a flagged model's point is NaN, and so is its probability
    double* fsp = fs_bar_out ? fs.dev + j0 : fs_tmp.p;
    double* vfp = Vfs_out ? vf.dev + j0 : vf_tmp.p;
    int rc = gprc_gpc_batch_predict_latent(fitted, xs_c, 1, d, nullptr, fsp, vfp, 1);
    if (rc == 0 && prob_out) rc = launch_gpc_class_prob(s, fsp, vfp, prob.dev + j0, B);
    gprc_batch_model_free(fitted);
    GPRC_TRY(rc);
    if (iters_out) std::copy(iters.begin(), iters.begin() + B, iters_out + j0);
    if (info_out) std::copy(info.begin(), info.begin() + B, info_out + j0);
  }
  return finish_sync(s, fs, vf, prob);
}

int gprc_lgpr_dims(const gprc_local_model* m, int64_t* n_out, int64_t* d_out, int64_t* m_out) {
  if (!m) return bad("lgpr_dims", "null model");
  if (n_out) *n_out = m->n;
  if (d_out) *d_out = m->d;
  if (m_out) *m_out = m->m;
  return 0;
}

int gprc_lgpr_free(gprc_local_model* m) { return free_bound(m, delete_bound<gprc_local_model>); }

}  // extern "C"
