// gprc_iter.hip -- iterative exact GPR ("Iterative GPR"): K_y^-1 B by preconditioned conjugate gradients on the
// matrix-free product K(X, X) P (gen_gemm, gprc_paths.hip), in O(n S) memory -- no n x n factor.  Kernels with k(x, x) = 1 (those of
// with_gradient_kernel).  K_y = K + noise I, noise = sigma^2 > 0.
//   preconditioner   L (n x r) = the partial pivoted Cholesky of K (kernels_cg.hip);  P = L L^T + noise I;
//                    B = I + L^T L / noise = C C^T on the sparse GPR's path (launch_gram_rows, the factor, solve_rows): Q = L C^-T / sigma and
//                    P^-1 V = (V - Q (Q^T V)) / noise, formed once per model; the loop holds two tall-skinny products and no small solve
//   loop             right-hand sides in blocks of CG_SB = 64 columns (the product's sample block).  Per iteration: AP = K P; then on the
//                    device, per column, alpha, x, r and |r|^2 (cg_step), z = P^-1 r, beta and p (cg_direction).  The host reads the block's
//                    |r|^2 and nothing else.  A column stops at |r|^2 <= tol^2 |b|^2 -- the doubles the device compares, so host and device
//                    agree on which columns run -- and is frozen: no kernel writes its x, r or p again.
//   after the loop   one more product: the TRUE residual |b - K_y x| / |b| per column; the recurrence drifts from it.
//   evidence         gprc_igpr_logp_grad ("Iterative GPR evidence"): probes z = L g1 + sigma g2 ~ N(0, P), w = P^-1 z, u = K_y^-1 z
//                    by the loop above, which then also stores every column's alpha_j and beta_j; per probe the Lanczos tridiagonal of
//                    P^-1/2 K_y P^-1/2 from those coefficients and its Gauss quadrature of log on the host (host_quadrature.h); the
//                    gradient's n x n weight 1/2 alpha alpha^T - 1/(2T) sum u w^T as two n x (T + 1) factors, contracted with dK / dtheta
//                    by kernels_igrad.hip without being formed.  The model keeps L beside Q and log det P for it.
// Invariance: a column's bits are the same alone or in any batch, on every call, from host and from device pointers -- each (s, i)
// accumulator of the product is its own chain, every vector step has one workgroup and one set of scalars per column.
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "gprc_host.h"
#include "host_quadrature.h"
#include "pair_tile.h"

namespace gprc {
namespace {

constexpr int64_t IGPR_MAX_RANK = 1024;

int igpr_usable(const char* who, const gprc_model* m) {
  if (!m || m->type != MODEL_IGPR) return bad(who, "not an iterative GPR model");
  return ctx_gone(who, *m);
}

// L (rows x r, pitch ldl, DEVICE), piv (r, DEVICE) and the rank; synchronises
int pivoted_cholesky(gprc_ctx* ctx, const KernelSpec& ks, const double* X, int64_t d, int64_t n, int64_t r, double* L, int64_t ldl, int64_t* piv,
                     int64_t* rank_out) {
  hipStream_t s = ctx->stream;
  DevMem pval, dg, st_word;
  GPRC_TRY(pval.alloc(r));
  GPRC_TRY(dg.alloc(n));
  GPRC_TRY(st_word.alloc(1));
  int* state = reinterpret_cast<int*>(st_word.p);
  GPRC_TRY(launch_pivoted_cholesky(s, ks, X, d, n, r, L, ldl, piv, pval.p, dg.p, state));
  int st = 0;
  GPRC_HIP(hipMemcpyAsync(&st, state, sizeof(int), hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipStreamSynchronize(s));
  *rank_out = st < 0 ? r : st;
  return 0;
}

// Q of the model from r steps of the pivoted Cholesky (header of this file); the model's rank is what the sweep reached
int build_preconditioner(gprc_model* m, int64_t r) {
  gprc_ctx* ctx = m->ctx;
  hipStream_t s = ctx->stream;
  const int64_t n = m->n, rows = pad_up(n, 256), r_pad = pad_up(r, NB), ld = rows + 16;   // the pitch off powers of two, as the sparse fit's
  DevMem vt, piv, packed, winv;
  GPRC_TRY(vt.alloc(ld * r_pad));
  GPRC_TRY(piv.alloc(r));
  GPRC_TRY(packed.alloc(gprc_packed_size(r_pad)));
  GPRC_TRY(winv.alloc(gprc_winv_size(r_pad)));
  GPRC_HIP(hipMemsetAsync(vt.p, 0, vt.bytes, s));   // zero in the padding rows and columns
  int64_t rank = 0;
  GPRC_TRY(pivoted_cholesky(ctx, m->ks, m->X, m->d, n, r, vt.p, ld, reinterpret_cast<int64_t*>(piv.p), &rank));
  m->rank = rank;
  GPRC_TRY(pool_alloc(ctx, sizeof(double) * (size_t)(n * rank), (void**)&m->pl));   // L itself: the probes z = L g1 + sigma g2 of the evidence
  GPRC_TRY(launch_copy_scaled(s, vt.p, ld, m->pl, n, n, rank, 1.0));
  auto form_b = [&]() -> int {   // B = I + L^T L / noise, packed
    GPRC_HIP(hipMemsetAsync(packed.p, 0, packed.bytes, s));
    GPRC_TRY(launch_gram_rows(s, vt.p, ld, rows, r_pad, packed.p));
    return launch_gram_to_b(s, packed.p, r_pad, m->noise);
  };
  GPRC_TRY(form_b());
  int info = 0;
  GPRC_TRY(factor_all_or_refill(ctx, packed.p, r_pad, winv.p, &info, nullptr, form_b));
  if (info != 0) { set_error("igpr_fit: the preconditioner's I + L^T L / noise is not positive definite (leading minor of order " + std::to_string(info) + ")"); return GPRC_ERR_NOT_PD; }
  // log det P = n log noise + log det B = n log noise + 2 sum log diag(C); the columns from the rank on are zero, their diagonal is 1
  double half_logdet_b = 0.0;
  GPRC_TRY(launch_diag_log_sum(s, packed.p, r_pad, r, ctx->scal_dev));
  GPRC_HIP(hipMemcpyAsync(&half_logdet_b, ctx->scal_dev, sizeof(double), hipMemcpyDeviceToHost, s));
  GPRC_TRY(solve_rows(ctx, packed.p, winv.p, r_pad, vt.p, ld, rows));   // L C^-T
  GPRC_TRY(pool_alloc(ctx, sizeof(double) * (size_t)(n * rank), (void**)&m->pq));
  GPRC_TRY(launch_copy_scaled(s, vt.p, ld, m->pq, n, n, rank, std::sqrt(m->noise)));
  GPRC_HIP(hipStreamSynchronize(s));   // the workspaces go out of scope
  m->logdet_p = (double)n * std::log(m->noise) + 2.0 * half_logdet_b;
  return 0;
}

// one block of S <= CG_SB right-hand sides; the five n x S buffers and the scalars are the caller's
// hist: null, or cg_max_iter x CG_SB x 2 doubles for the coefficients (launch_cg_step)
struct CgWork { double *x, *r, *z, *p, *ap, *t, *sc, *res, *hist; };

int cg_block(gprc_model* m, const CgWork& w, const double* B, int64_t ldb, int64_t S, double* X, int64_t ldx, int* iters, double* relres,
             double* relres_true, bool* maxiter_hit, std::vector<double>* hist_out) {
  gprc_ctx* ctx = m->ctx;
  hipStream_t s = ctx->stream;
  const int64_t n = m->n;
  const double* z = m->pq ? w.z : w.r;   // no preconditioner: z = r
  auto product = [&](const double* V, double* out) { return gen_gemm(ctx, &m->ks, m->X, nullptr, n, m->X, n, m->d, V, n, S, 1.0, false, out, n); };
  auto precondition = [&]() -> int { return m->pq ? launch_apply_precond(s, m->pq, m->rank, w.r, n, S, m->noise, w.t, w.z) : 0; };
  double bb[CG_SB], thr2[CG_SB], rr[CG_SB];
  bool active[CG_SB];
  int it_of[CG_SB];
  GPRC_TRY(launch_cg_init(s, B, ldb, n, S, m->cg_tol, w.r, w.x, w.sc));
  GPRC_TRY(precondition());
  GPRC_TRY(launch_cg_direction(s, w.r, z, w.p, n, S, true, w.sc));
  GPRC_HIP(hipMemcpyAsync(bb, w.sc + CG_BB * CG_SB, sizeof(double) * S, hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipMemcpyAsync(thr2, w.sc + CG_THR2 * CG_SB, sizeof(double) * S, hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipStreamSynchronize(s));
  int running = 0;
  for (int64_t c = 0; c < S; ++c) { rr[c] = bb[c]; it_of[c] = 0; active[c] = !(bb[c] <= thr2[c]); running += active[c]; }
  int it = 0;
  int64_t bad = -1;
  while (running > 0 && it < m->cg_max_iter) {
    GPRC_TRY(product(w.p, w.ap));
    GPRC_TRY(launch_cg_step(s, w.p, w.ap, w.x, w.r, n, S, m->noise, w.sc, w.hist, it));
    GPRC_TRY(precondition());
    GPRC_TRY(launch_cg_direction(s, w.r, z, w.p, n, S, false, w.sc, w.hist, it));
    GPRC_HIP(hipMemcpyAsync(rr, w.sc + CG_RR * CG_SB, sizeof(double) * S, hipMemcpyDeviceToHost, s));
    GPRC_HIP(hipStreamSynchronize(s));
    ++it;
    for (int64_t c = 0; c < S; ++c) {
      if (!active[c]) continue;
      it_of[c] = it;
      if (!(rr[c] >= 0.0) || !std::isfinite(rr[c])) { bad = c; active[c] = false; --running; }
      else if (rr[c] <= thr2[c]) { active[c] = false; --running; }
    }
    if (bad >= 0) break;
  }
  if (bad >= 0) {
    set_error("igpr: p^T (K + noise I) p was not finite or not positive in iteration " + std::to_string(it) + " (column " + std::to_string(bad) +
              " of its block): the matrix is not positive definite in floating point, or the right-hand side is not finite");
    return GPRC_ERR_NOT_PD;
  }
  if (running > 0) *maxiter_hit = true;
  if (w.hist && hist_out && it > 0) {   // a column's own steps: those it ran before it froze
    std::vector<double> h((size_t)it * CG_SB * 2);
    GPRC_HIP(hipMemcpyAsync(h.data(), w.hist, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s));
    GPRC_HIP(hipStreamSynchronize(s));
    for (int64_t c = 0; c < S; ++c) {
      hist_out[c].resize((size_t)it_of[c] * 2);
      for (int j = 0; j < it_of[c]; ++j) {
        hist_out[c][2 * j] = h[((size_t)j * CG_SB + c) * 2];
        hist_out[c][2 * j + 1] = j + 1 < it_of[c] ? h[((size_t)j * CG_SB + c) * 2 + 1] : 0.0;
      }
    }
  }
  GPRC_TRY(product(w.x, w.ap));
  GPRC_TRY(launch_cg_residual(s, B, ldb, w.ap, w.x, n, S, m->noise, w.sc, w.res));
  GPRC_HIP(hipMemcpy2DAsync(X, sizeof(double) * ldx, w.x, sizeof(double) * n, sizeof(double) * n, (size_t)S, hipMemcpyDeviceToDevice, s));
  if (relres_true) {
    GPRC_HIP(hipMemcpyAsync(relres_true, w.res, sizeof(double) * S, hipMemcpyDeviceToHost, s));
    GPRC_HIP(hipStreamSynchronize(s));
  }
  for (int64_t c = 0; c < S; ++c) {
    if (iters) iters[c] = it_of[c];
    if (relres) relres[c] = bb[c] > 0.0 ? std::sqrt(rr[c] / bb[c]) : 0.0;
  }
  return 0;
}

// acc[k] += sum_ij (A B^T)_ij (integrand of theta_k), DEVICE pointers, any R: blocks of IG_RMAX columns, one launch each, the partials of
// a launch added in workgroup order and the blocks in order, in long double; synchronises
int lowrank_grad_dev(gprc_ctx* ctx, const KernelSpec& ks, const double* X, int64_t d, int64_t n, const double* A, int64_t lda, const double* B,
                     int64_t ldb, int64_t R, long double* acc) {
  hipStream_t s = ctx->stream;
  const int64_t wgs = lowrank_grad_wgs(n);
  DevMem part;
  GPRC_TRY(part.alloc(wgs * ks.n_params));
  std::vector<double> hp((size_t)(wgs * ks.n_params));
  for (int64_t r0 = 0; r0 < R; r0 += IG_RMAX) {
    GPRC_TRY(launch_lowrank_grad(s, ks, X, d, n, A + r0 * lda, lda, B + r0 * ldb, ldb, std::min<int64_t>(IG_RMAX, R - r0), part.p));
    GPRC_HIP(hipMemcpyAsync(hp.data(), part.p, sizeof(double) * hp.size(), hipMemcpyDeviceToHost, s));
    GPRC_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < ks.n_params; ++k) {
      long double sum = 0.0L;
      for (int64_t g = 0; g < wgs; ++g) sum += (long double)hp[(size_t)(g * ks.n_params + k)];
      acc[k] += sum;
    }
  }
  return 0;
}

// Z (n x T, pitch ldz, DEVICE) from DEVICE G1 and G2
int igpr_probes_dev(gprc_model* m, const double* G1, int64_t ldg1, const double* G2, int64_t ldg2, int64_t T, double* Z, int64_t ldz) {
  return launch_igpr_probes(m->ctx->stream, m->pl, m->rank, G1, ldg1, G2, ldg2, std::sqrt(m->noise), m->n, T, Z, ldz);
}

int check_probe_args(const char* who, const gprc_model* m, const double* G1, int64_t ldg1, const double* G2, int64_t ldg2, int64_t T) {
  if (T < 1 || T > 65535) return bad(who, "the number of probes T must be between 1 and 65535");
  if (!G2 || ldg2 < m->n) return bad(who, "G2 must be non-null with ldg2 >= n");
  if (m->rank > 0 && (!G1 || ldg1 < m->rank)) return bad(who, "G1 must be non-null with ldg1 >= the preconditioner's rank");
  return 0;
}

}  // namespace

int igpr_solve_dev(gprc_model* m, const double* B, int64_t ldb, int64_t S, double* X, int64_t ldx, int* iters, double* relres, double* relres_true,
                   std::vector<double>* hist) {
  const int64_t n = m->n, sb = std::min<int64_t>(S, CG_SB);
  DevMem vec, small, hbuf;
  if (hist) GPRC_TRY(hbuf.alloc((int64_t)m->cg_max_iter * CG_SB * 2));
  GPRC_TRY(vec.alloc((m->pq ? 5 : 4) * n * sb));
  GPRC_TRY(small.alloc(std::max<int64_t>(m->rank, 1) * sb + (CG_ROWS + 1) * CG_SB));
  CgWork w{};
  w.x = vec.p; w.r = w.x + n * sb; w.p = w.r + n * sb; w.ap = w.p + n * sb; w.z = m->pq ? w.ap + n * sb : nullptr;
  w.t = small.p; w.sc = w.t + std::max<int64_t>(m->rank, 1) * sb; w.res = w.sc + CG_ROWS * CG_SB; w.hist = hbuf.p;
  bool maxiter_hit = false;
  for (int64_t s0 = 0; s0 < S; s0 += CG_SB) {
    const int64_t scur = std::min<int64_t>(CG_SB, S - s0);
    GPRC_TRY(cg_block(m, w, B + s0 * ldb, ldb, scur, X + s0 * ldx, ldx, iters ? iters + s0 : nullptr, relres ? relres + s0 : nullptr,
                      relres_true ? relres_true + s0 : nullptr, &maxiter_hit, hist ? hist + s0 : nullptr));
  }
  if (maxiter_hit) {
    GPRC_HIP(hipStreamSynchronize(m->ctx->stream));   // the outputs of the last iterate are complete when the caller sees the status
    set_error("igpr: the conjugate-gradient loop reached max_iter = " + std::to_string(m->cg_max_iter) +
              " before every column met tol; the outputs hold the last iterate (raise max_iter or the preconditioner's rank)");
    return GPRC_ERR_MAXITER;
  }
  return 0;
}

}  // namespace gprc

using namespace gprc;

extern "C" {

int gprc_igpr_fit(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n, const double* y, double noise,
                  double tol, int max_iter, int64_t precond_rank, gprc_model** model_out) {
  if (!ctx || !X || !y || !model_out || d < 1 || n < 1) { set_error("igpr_fit: bad arguments (null pointer, d < 1 or n < 1)"); return GPRC_ERR_ARG; }
  if (!(noise > 0.0) || !std::isfinite(noise)) { set_error("igpr_fit: noise must be finite and > 0"); return GPRC_ERR_ARG; }
  if (!(tol > 0.0) || !std::isfinite(tol)) { set_error("igpr_fit: tol must be finite and > 0"); return GPRC_ERR_ARG; }
  if (precond_rank < 0 || precond_rank > IGPR_MAX_RANK) { set_error("igpr_fit: precond_rank must be between 0 (no preconditioner) and 1024"); return GPRC_ERR_ARG; }
  GPRC_TRY(check_grad_kernel("igpr_fit", kernel));
  GPRC_TRY(use_device(ctx));
  KernelSpec ks;
  GPRC_TRY(make_spec(kernel, params, n_params, d, &ks));
  ModelPtr m(new (std::nothrow) gprc_model());
  if (!m) { set_error("out of host memory"); return GPRC_ERR_NOMEM; }
  m->ctx = ctx; m->ctx_id = ctx->id; m->type = MODEL_IGPR; m->ks = ks; m->n = n; m->d = d; m->n_pad = pad_up(n, NB);
  m->noise = noise; m->cg_tol = tol; m->cg_max_iter = max_iter <= 0 ? 1000 : max_iter;
  hipStream_t s = ctx->stream;
  GPRC_TRY(pool_alloc(ctx, sizeof(double) * (size_t)(d * n), (void**)&m->X));
  GPRC_TRY(pool_alloc(ctx, sizeof(double) * (size_t)m->n_pad, (void**)&m->y));
  GPRC_TRY(pool_alloc(ctx, sizeof(double) * (size_t)m->n_pad, (void**)&m->alpha));
  GPRC_HIP(hipMemcpyAsync(m->X, X, sizeof(double) * d * n, hipMemcpyDefault, s));
  GPRC_HIP(hipMemsetAsync(m->y, 0, sizeof(double) * m->n_pad, s));
  GPRC_HIP(hipMemcpyAsync(m->y, y, sizeof(double) * n, hipMemcpyDefault, s));
  GPRC_HIP(hipMemsetAsync(m->alpha, 0, sizeof(double) * m->n_pad, s));
  if (precond_rank > 0) GPRC_TRY(build_preconditioner(m.get(), std::min(precond_rank, n)));
  GPRC_TRY(igpr_solve_dev(m.get(), m->y, n, 1, m->alpha, n, &m->cg_iters, &m->cg_relres, &m->cg_relres_true));   // MAXITER: no model
  GPRC_HIP(hipStreamSynchronize(s));
  *model_out = m.release();
  return 0;
}

int gprc_igpr_solve(gprc_model* m, const double* B, int64_t ldb, int64_t S, double* Xout, int64_t ldx, int* iters_out, double* relres_true_out) {
  GPRC_TRY(igpr_usable("igpr_solve", m));
  if (!B || !Xout || S < 1) { set_error("igpr_solve: bad arguments (non-null B and Xout, S >= 1)"); return GPRC_ERR_ARG; }
  if (ldb < m->n || ldx < m->n) { set_error("igpr_solve: ldb < n or ldx < n"); return GPRC_ERR_ARG; }
  gprc_ctx* ctx = m->ctx;
  GPRC_TRY(use_device(ctx));
  hipStream_t s = ctx->stream;
  In b;
  Out o;
  GPRC_TRY(b.set(s, B, ldb * (S - 1) + m->n));
  GPRC_TRY(o.set(Xout, ldx, m->n, S));
  const int rc = igpr_solve_dev(m, b.dev, ldb, S, o.dev, o.ld, iters_out, nullptr, relres_true_out);
  if (rc != 0 && rc != GPRC_ERR_MAXITER) return rc;
  GPRC_TRY(finish_sync(s, o));
  return rc;
}

int gprc_igpr_predict(gprc_model* m, const double* X_star, int64_t ns, double* mean_out, double* var_out) {
  GPRC_TRY(igpr_usable("igpr_predict", m));
  if (ns < 1 || !X_star || !mean_out) { set_error("igpr_predict: bad arguments (n_star >= 1, non-null X_star and mean)"); return GPRC_ERR_ARG; }
  gprc_ctx* ctx = m->ctx;
  GPRC_TRY(use_device(ctx));
  hipStream_t s = ctx->stream;
  const int64_t n = m->n, d = m->d;
  In xs;
  Out om, ov;
  GPRC_TRY(xs.set(s, X_star, d * ns));
  GPRC_TRY(om.set(mean_out, ns));
  if (var_out) GPRC_TRY(ov.set(var_out, ns));
  GPRC_TRY(gen_gemm(ctx, &m->ks, m->X, nullptr, n, xs.dev, ns, d, m->alpha, n, 1, 1.0, false, om.dev, ns));
  int rc = 0;
  if (var_out) {   // var_i = 1 - k*_i^T K_y^-1 k*_i: a full solve per block of test points
    const int64_t sb = std::min<int64_t>(ns, CG_SB);
    DevMem ks_blk, w;
    GPRC_TRY(ks_blk.alloc(n * sb));
    GPRC_TRY(w.alloc(n * sb));
    for (int64_t s0 = 0; s0 < ns; s0 += CG_SB) {
      const int64_t scur = std::min<int64_t>(CG_SB, ns - s0);
      GPRC_TRY(launch_fill(s, m->ks, m->X, n, xs.dev + s0 * d, scur, d, ks_blk.p, n, 0, n, 0, scur, PAD_NONE, 0.0));   // K(X, X*_block)
      const int rb = igpr_solve_dev(m, ks_blk.p, n, scur, w.p, n, nullptr, nullptr, nullptr);
      if (rb != 0 && rb != GPRC_ERR_MAXITER) return rb;
      if (rb != 0) rc = rb;
      GPRC_TRY(launch_cg_var(s, ks_blk.p, w.p, n, scur, ov.dev + s0));
    }
  }
  GPRC_TRY(finish_sync(s, om, ov));
  return rc;
}

int gprc_igpr_get_alpha(gprc_model* m, double* alpha_out) {
  GPRC_TRY(igpr_usable("igpr_get_alpha", m));
  if (!alpha_out) { set_error("igpr_get_alpha: null output"); return GPRC_ERR_ARG; }
  GPRC_TRY(use_device(m->ctx));
  GPRC_HIP(hipMemcpyAsync(alpha_out, m->alpha, sizeof(double) * m->n, hipMemcpyDefault, m->ctx->stream));
  GPRC_HIP(hipStreamSynchronize(m->ctx->stream));
  return 0;
}

int gprc_igpr_stats(gprc_model* m, int* iterations_out, double* relres_recurrence_out, double* relres_true_out, int64_t* rank_out) {
  if (!m || m->type != MODEL_IGPR) { set_error("igpr_stats: not an iterative GPR model"); return GPRC_ERR_ARG; }
  if (iterations_out) *iterations_out = m->cg_iters;
  if (relres_recurrence_out) *relres_recurrence_out = m->cg_relres;
  if (relres_true_out) *relres_true_out = m->cg_relres_true;
  if (rank_out) *rank_out = m->rank;
  return 0;
}

int gprc_igpr_probes(gprc_model* m, const double* G1, int64_t ldg1, const double* G2, int64_t ldg2, int64_t T, double* Z_out, int64_t ldz) {
  GPRC_TRY(igpr_usable("igpr_probes", m));
  GPRC_TRY(check_probe_args("igpr_probes", m, G1, ldg1, G2, ldg2, T));
  if (!Z_out || ldz < m->n) { set_error("igpr_probes: Z_out must be non-null with ldz >= n"); return GPRC_ERR_ARG; }
  gprc_ctx* ctx = m->ctx;
  GPRC_TRY(use_device(ctx));
  hipStream_t s = ctx->stream;
  In g1, g2;
  Out o;
  if (m->rank > 0) GPRC_TRY(g1.set(s, G1, ldg1 * (T - 1) + m->rank));
  GPRC_TRY(g2.set(s, G2, ldg2 * (T - 1) + m->n));
  GPRC_TRY(o.set(Z_out, ldz, m->n, T));
  GPRC_TRY(igpr_probes_dev(m, g1.dev, ldg1, g2.dev, ldg2, T, o.dev, o.ld));
  return finish_sync(s, o);
}

int gprc_igpr_logp_grad(gprc_model* m, const double* G1, int64_t ldg1, const double* G2, int64_t ldg2, int64_t T, double* logp_out, double* se_out,
                        double* grad_out, double* terms_out) {
  GPRC_TRY(igpr_usable("igpr_logp_grad", m));
  GPRC_TRY(check_probe_args("igpr_logp_grad", m, G1, ldg1, G2, ldg2, T));
  if (!logp_out || !grad_out) { set_error("igpr_logp_grad: null logp_out or grad_out"); return GPRC_ERR_ARG; }
  if (se_out && T < 2) { set_error("igpr_logp_grad: the standard error needs T >= 2 probes"); return GPRC_ERR_ARG; }
  gprc_ctx* ctx = m->ctx;
  GPRC_TRY(use_device(ctx));
  hipStream_t s = ctx->stream;
  const int64_t n = m->n, R = T + 1;
  const int np = m->ks.n_params;
  In g1, g2;
  if (m->rank > 0) GPRC_TRY(g1.set(s, G1, ldg1 * (T - 1) + m->rank));
  GPRC_TRY(g2.set(s, G2, ldg2 * (T - 1) + n));
  // A = [alpha, u_1 .. u_T], B = [alpha / 2, -w_1 / (2 T) .. -w_T / (2 T)]: G = A B^T (never formed); z and w = P^-1 z beside them
  DevMem za, zb, zz, zw, tq, dots;
  GPRC_TRY(za.alloc(n * R));
  GPRC_TRY(zb.alloc(n * R));
  GPRC_TRY(zz.alloc(n * T));
  if (m->pq) GPRC_TRY(zw.alloc(n * T));
  GPRC_TRY(tq.alloc(std::max<int64_t>(m->rank, 1) * CG_SB));
  GPRC_TRY(dots.alloc(2 * T + 2));
  double *U = za.p + n, *Z = zz.p, *W = m->pq ? zw.p : zz.p;   // rank 0: P = I, w = z
  GPRC_TRY(igpr_probes_dev(m, g1.dev, ldg1, g2.dev, ldg2, T, Z, n));
  if (m->pq)
    for (int64_t s0 = 0; s0 < T; s0 += CG_SB)   // the blocks of the loop: w is what the loop's first preconditioned residual is
      GPRC_TRY(launch_apply_precond(s, m->pq, m->rank, Z + s0 * n, n, std::min<int64_t>(CG_SB, T - s0), m->noise, tq.p, W + s0 * n));
  std::vector<int> iters((size_t)T);
  std::vector<std::vector<double>> hist((size_t)T);
  const int rc = igpr_solve_dev(m, Z, n, T, U, n, iters.data(), nullptr, nullptr, hist.data());
  if (rc != 0 && rc != GPRC_ERR_MAXITER) return rc;
  const std::string maxiter_msg = rc != 0 ? gprc_last_error() : "";
  GPRC_HIP(hipMemcpyAsync(za.p, m->alpha, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
  GPRC_TRY(launch_copy_scaled(s, m->alpha, n, zb.p, n, n, 1, 2.0));
  GPRC_TRY(launch_copy_scaled(s, W, n, zb.p + n, n, n, T, -2.0 * (double)T));
  GPRC_TRY(launch_col_dots(s, Z, n, W, n, n, T, dots.p));             // z^T P^-1 z
  GPRC_TRY(launch_col_dots(s, U, n, W, n, n, T, dots.p + T));         // u^T w
  GPRC_TRY(launch_col_dots(s, m->y, n, m->alpha, n, n, 1, dots.p + 2 * T));
  GPRC_TRY(launch_col_dots(s, m->alpha, n, m->alpha, n, n, 1, dots.p + 2 * T + 1));
  std::vector<double> hd((size_t)(2 * T + 2));
  GPRC_HIP(hipMemcpyAsync(hd.data(), dots.p, sizeof(double) * hd.size(), hipMemcpyDeviceToHost, s));
  std::vector<long double> acc((size_t)np, 0.0L);
  GPRC_TRY(lowrank_grad_dev(ctx, m->ks, m->X, m->d, n, za.p, n, zb.p, n, R, acc.data()));   // synchronises
  cross_grad_finish(m->ks, acc.data(), grad_out);
  // the quadrature: q_s = (z^T P^-1 z) e_1^T log(T_s) e_1 from the column's own coefficients
  std::vector<double> q((size_t)T), al, be, dg, of;
  long double qsum = 0.0L, uw = 0.0L;
  for (int64_t c = 0; c < T; ++c) {
    const int mm = iters[(size_t)c];
    double quad = 0.0;
    if (mm > 0) {
      al.resize((size_t)mm); be.resize((size_t)mm); dg.resize((size_t)mm); of.resize((size_t)mm);
      for (int j = 0; j < mm; ++j) { al[j] = hist[(size_t)c][2 * j]; be[j] = hist[(size_t)c][2 * j + 1]; }
      cg_tridiagonal(mm, al.data(), be.data(), dg.data(), of.data());
      const int qrc = tridiag_log_quadrature(mm, dg.data(), of.data(), &quad);
      if (qrc != QUAD_OK) {
        set_error("igpr_logp_grad: the Lanczos tridiagonal of probe " + std::to_string(c) + (qrc == QUAD_NOT_POSITIVE ? " has a non-positive eigenvalue" : " did not yield its eigenvalues") +
                  ": the preconditioned matrix is not positive definite in floating point");
        return GPRC_ERR_NOT_PD;
      }
    }
    q[(size_t)c] = hd[(size_t)c] * quad;
    qsum += (long double)q[(size_t)c];
    uw += (long double)hd[(size_t)(T + c)];
  }
  const long double mean_q = qsum / (long double)T;
  const double two_pi = 6.283185307179586476925286766559;
  *logp_out = (double)(-0.5L * (long double)hd[(size_t)(2 * T)] - 0.5L * ((long double)m->logdet_p + mean_q) - 0.5L * (long double)n * (long double)std::log(two_pi));
  grad_out[np] = (double)(0.5L * (long double)hd[(size_t)(2 * T + 1)] - uw / (2.0L * (long double)T));
  if (se_out) {
    long double ss = 0.0L;
    for (int64_t c = 0; c < T; ++c) { const long double dq = (long double)q[(size_t)c] - mean_q; ss += dq * dq; }
    *se_out = (double)(0.5L * std::sqrt(ss / (long double)(T - 1)) / std::sqrt((long double)T));
  }
  if (terms_out) for (int64_t c = 0; c < T; ++c) terms_out[c] = q[(size_t)c];
  if (rc != 0) set_error(maxiter_msg);
  return rc;
}

int gprc_dev_lowrank_grad(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n, const double* A,
                          int64_t lda, const double* B, int64_t ldb, int64_t R, double* grad_out) {
  GPRC_TRY(use_device_unless(ctx, !X || !A || !B || !grad_out || d < 1 || n < 1 || R < 1 || lda < n || ldb < n,
                             "dev_lowrank_grad: bad arguments (non-null pointers, d, n, R >= 1, lda >= n, ldb >= n)"));
  GPRC_TRY(check_grad_kernel("dev_lowrank_grad", kernel));
  KernelSpec ks;
  GPRC_TRY(make_spec(kernel, params, n_params, d, &ks));
  hipStream_t s = ctx->stream;
  In x, a, b;
  GPRC_TRY(x.set(s, X, d * n));
  GPRC_TRY(a.set(s, A, lda * (R - 1) + n));
  GPRC_TRY(b.set(s, B, ldb * (R - 1) + n));
  std::vector<long double> acc((size_t)ks.n_params, 0.0L);
  GPRC_TRY(lowrank_grad_dev(ctx, ks, x.dev, d, n, a.dev, lda, b.dev, ldb, R, acc.data()));
  cross_grad_finish(ks, acc.data(), grad_out);
  return 0;
}

int gprc_dev_pivoted_cholesky(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n, int64_t r, double* L,
                              int64_t ldl, int64_t* piv_out, int64_t* rank_out) {
  GPRC_TRY(use_device_unless(ctx, !X || !L || !piv_out || !rank_out || d < 1 || n < 1 || r < 1 || r > n || r > IGPR_MAX_RANK || ldl < n,
                             "dev_pivoted_cholesky: bad arguments (1 <= r <= min(n, 1024), ldl >= n, non-null pointers)"));
  GPRC_TRY(check_grad_kernel("dev_pivoted_cholesky", kernel));
  KernelSpec ks;
  GPRC_TRY(make_spec(kernel, params, n_params, d, &ks));
  hipStream_t s = ctx->stream;
  In x;
  Out o;
  DevMem piv;
  GPRC_TRY(x.set(s, X, d * n));
  GPRC_TRY(o.set(L, ldl, n, r));
  GPRC_TRY(piv.alloc(r));
  GPRC_HIP(hipMemsetAsync(piv.p, 0xff, piv.bytes, s));   // -1 from the rank on
  GPRC_TRY(pivoted_cholesky(ctx, ks, x.dev, d, n, r, o.dev, o.ld, reinterpret_cast<int64_t*>(piv.p), rank_out));
  GPRC_HIP(hipMemcpyAsync(piv_out, piv.p, sizeof(int64_t) * r, hipMemcpyDefault, s));
  return finish_sync(s, o);
}

}  // extern "C"
