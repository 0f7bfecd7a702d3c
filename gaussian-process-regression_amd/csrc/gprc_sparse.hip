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
// The gradient of the bound (sgpr_grad, gprc_sgpr_elbo_grad) reuses that pass as it is and adds a second one: see sgpr_grad.
#include <algorithm>
#include <cmath>
#include <new>
#include <utility>
#include <vector>

#include "gprc_host.h"
#include "host_sums.h"
#include "pair_tile.h"

namespace gprc {
namespace {

constexpr long double SGPR_PI = 3.141592653589793238462643383279502884L;

struct SgprArgs {
  const double *X, *y, *Z;
  int64_t d, n, m;
  double noise, jitter;
};

int sgpr_check(const char* who, gprc_ctx* ctx, const SgprArgs& a, bool out_ok) {
  if (!ctx || !a.X || !a.y || !a.Z || !out_ok || a.d < 1) return bad(who, "bad arguments (null pointer or d < 1)");
  if (a.n < 1 || a.m < 1) return bad(who, "n >= 1 training points and m >= 1 inducing points");
  if (!(a.noise > 0.0) || !std::isfinite(a.noise)) return bad(who, "noise must be finite and > 0");
  if (!(a.jitter >= 0.0) || !std::isfinite(a.jitter)) return bad(who, "jitter must be finite and >= 0");
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

// what the bound's gradient wants of the fit beyond the model: B before it is factored (packed) and the three host sums of the bound
struct SgprKeep {
  DevMem b;
  long double yy = 0.0L, cc = 0.0L, t = 0.0L;
};

// The fit: both factors, c, elbo and t into the model.  *info_out > 0: the leading minor of K_uu or of B that is not positive (the
// error text says which); the model is then not usable.  keep: see SgprKeep (the fit itself is the same launches and the same bits).
int sgpr_fit(gprc_model* mo, const SgprArgs& a, int* info_out, SgprKeep* keep = nullptr) {
  gprc_ctx* ctx = mo->ctx;
  hipStream_t s = ctx->stream;
  const int64_t n = a.n, d = a.d, m = a.m, m_pad = mo->n_pad, nblk = m_pad / NBI;
  *info_out = 0;
  GPRC_HIP(hipMemcpyAsync(mo->X, a.Z, sizeof(double) * d * m, hipMemcpyDefault, s));
  DevMem inv;   // explicit inverses of the diagonal blocks of L_B: the vector solve for c
  GPRC_TRY(inv.alloc(gprc_solve_inv_size(m_pad)));
  if (keep) GPRC_TRY(keep->b.alloc(gprc_packed_size(m_pad)));

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
    if (keep) GPRC_HIP(hipMemcpyAsync(keep->b.p, mo->packed_b, keep->b.bytes, hipMemcpyDeviceToDevice, s));
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
  if (keep) { keep->yy = yy; keep->cc = cc; keep->t = t; }
  return 0;
}

int sgpr_fit_entry(const char* who, gprc_ctx* ctx, int kernel, const double* params, int n_params, const SgprArgs& a, bool out_ok, ModelPtr& mo,
                   SgprKeep* keep = nullptr) {
  GPRC_TRY(sgpr_check(who, ctx, a, out_ok));
  GPRC_TRY(use_device(ctx));
  KernelSpec ks;
  GPRC_TRY(make_spec(kernel, params, n_params, a.d, &ks));
  GPRC_TRY(sgpr_alloc(ctx, ks, a.m, a.d, mo));
  int info = 0;
  GPRC_TRY(sgpr_fit(mo.get(), a, &info, keep));
  return info;
}

// One launch of the contraction (kernels_sgrad.hip) and what follows it: the theta partials go to the host and into acc (times f_theta,
// workgroup order, long double); with dz the column sums are added to it (times f_z, stripe order).  part, pz: the launch's buffers.
int cross_grad_step(hipStream_t s, const KernelSpec& ks, const double* G, int64_t ld, const double* A, int64_t rows, int64_t rows_pad, const double* Z,
                    int64_t cols, int64_t cols_pad, int64_t d, double* part, double* pz, long double f_theta, double f_z, long double* acc, double* dz) {
  GPRC_TRY(launch_cross_grad(s, ks, G, ld, A, rows, rows_pad, Z, cols, cols_pad, d, part, dz ? pz : nullptr));
  std::vector<double> hp((size_t)(cross_grad_wgs(rows_pad, cols_pad) * ks.n_params));
  GPRC_HIP(hipMemcpyAsync(hp.data(), part, sizeof(double) * hp.size(), hipMemcpyDeviceToHost, s));
  if (dz) GPRC_TRY(launch_cross_grad_sum(s, ks, pz, rows_pad, cols_pad, cols, d, f_z, dz));
  GPRC_HIP(hipStreamSynchronize(s));
  cross_grad_add_partials(hp.data(), rows_pad, cols_pad, ks.n_params, f_theta, acc);
  return 0;
}

// The gradient of the bound after sgpr_fit ("Sparse GPR gradient"); notation of the head of this file, and
//   q = L_B^-T c,  mu = L_u^-T q,  r = y - V q
//   G_fu = [ V (I - B^-1) L_u^-1 + r mu^T ] / sigma^2                     n x m, chunk by chunk
//   G_uu = 1/2 L_u^-T (2 I - B^-1 - B) L_u^-1 - 1/2 mu mu^T              m x m
//   d elbo / d theta = sum G_fu dK_fu + sum G_uu dK_uu,   d elbo / d Z likewise (K_uu: both arguments move, twice the column sums)
// The m^3 part, whitened throughout (no K_uu^-1, no Sigma^-1 is formed): E_u = L_u^-T and E_B = L_B^-T as the identity through the
// predict's solve in its triangular form; W = -E_B E_B^T = -B^-1 as logp_grad forms K_y^-1 (lower triangle); then, with four m_pad^2
// buffers, T' = -E_u (I + W) (= -[(I - B^-1) L_u^-1]^T), P = -E_u (2 I + W - B), G_uu' = -mu mu^T - P E_u^T: three launch_gemm_nt.  The
// second pass over the training points is chunked as the fit's (half its rows: V and G' share the chunk workspace): fill, row solve with
// L_u, r by the row reduction, G' = r mu^T - V T'^T in one launch_gemm_nt, the contraction.  The factors 1/2 and 1 / sigma^2 go on the sums, not on the matrices.
// Order of summation: within a launch as kernels_sgrad.hip says; theta: K_uu's launch, then the chunks in order, each launch's
// workgroups in order, in long double on the host; dZ: the same order on the device, one fused multiply-add per launch and entry.
// grad_out: n_params + 1 (host), d elbo / d sigma^2 last, assembled in long double; dz: d x m on the device, or nullptr.
int sgpr_grad(gprc_model* mo, const SgprArgs& a, const SgprKeep& keep, double* grad_out, double* dz) {
  gprc_ctx* ctx = mo->ctx;
  hipStream_t s = ctx->stream;
  const int64_t n = a.n, d = a.d, m = a.m, m_pad = mo->n_pad, sq = m_pad * m_pad;
  const int np = mo->ks.n_params;
  const long double s2 = (long double)a.noise;
  DevMem eu, b1, b2, b3, q, mu, red;
  for (DevMem* p : {&eu, &b1, &b2, &b3}) GPRC_TRY(p->alloc(sq));
  GPRC_TRY(q.alloc(m_pad));
  GPRC_TRY(mu.alloc(m_pad));
  GPRC_TRY(red.alloc(m_pad * rowreduce_splits(m_pad)));
  // E_u, E_B, q, mu
  GPRC_TRY(launch_set_identity_rows(s, eu.p, m_pad, m_pad, m_pad, 0));
  GPRC_TRY(solve_rows(ctx, mo->packed, mo->winv, m_pad, eu.p, m_pad, m_pad, nullptr, 0));
  GPRC_TRY(launch_set_identity_rows(s, b1.p, m_pad, m_pad, m_pad, 0));
  GPRC_TRY(solve_rows(ctx, mo->packed_b, mo->winv_b, m_pad, b1.p, m_pad, m_pad, nullptr, 0));
  GPRC_TRY(launch_row_reduce(s, b1.p, m_pad, m_pad, m_pad, mo->alpha, q.p, red.p));
  GPRC_TRY(launch_row_reduce(s, eu.p, m_pad, m_pad, m_pad, q.p, mu.p, red.p));
  // W = -B^-1 (lower) into b2, B (lower) into b3; tr B^-1 and q to the host
  GPRC_HIP(hipMemsetAsync(b2.p, 0, sizeof(double) * (size_t)sq, s));
  GPRC_TRY(launch_gemm_nt(s, b2.p, m_pad, b1.p, m_pad, b1.p, m_pad, m_pad, m_pad, m_pad, 1, PK_INV_GEMM));
  GPRC_TRY(launch_unpack_L(s, keep.b.p, m_pad, m_pad, b3.p, m_pad));
  std::vector<double> hdiag((size_t)m), hq((size_t)m);
  GPRC_HIP(hipMemcpy2DAsync(hdiag.data(), sizeof(double), b2.p, sizeof(double) * (size_t)(m_pad + 1), sizeof(double), (size_t)m, hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipMemcpyAsync(hq.data(), q.p, sizeof(double) * m, hipMemcpyDeviceToHost, s));
  GPRC_TRY(launch_sgrad_mid(s, b2.p, b3.p, m_pad));                                                     // b2 = I + W, b3 = 2 I + W - B, symmetric
  GPRC_HIP(hipMemsetAsync(b1.p, 0, sizeof(double) * (size_t)sq, s));
  GPRC_TRY(launch_gemm_nt(s, b1.p, m_pad, eu.p, m_pad, b2.p, m_pad, m_pad, m_pad, m_pad, 0, PK_COV_SYRK));   // b1 = T' = -E_u (I + W)
  GPRC_HIP(hipMemsetAsync(b2.p, 0, sizeof(double) * (size_t)sq, s));
  GPRC_TRY(launch_gemm_nt(s, b2.p, m_pad, eu.p, m_pad, b3.p, m_pad, m_pad, m_pad, m_pad, 0, PK_COV_SYRK));   // b2 = P = -E_u (2 I + W - B)
  GPRC_TRY(launch_rank_one(s, b3.p, m_pad, m_pad, m_pad, mu.p, mu.p, -1.0));
  GPRC_TRY(launch_gemm_nt(s, b3.p, m_pad, b2.p, m_pad, eu.p, m_pad, m_pad, m_pad, m_pad, 0, PK_COV_SYRK));   // b3 = 2 G_uu
  if (dz) GPRC_HIP(hipMemsetAsync(dz, 0, sizeof(double) * (size_t)(d * m), s));

  std::vector<long double> acc((size_t)np, 0.0L);
  {  // K_uu's part: G = 2 G_uu as a full square, A = Z; 1/2 on theta, 2 x 1/2 on dZ
    DevMem part, pz;
    GPRC_TRY(part.alloc(cross_grad_partials(m_pad, np)));
    if (dz) GPRC_TRY(pz.alloc(cross_grad_zpartials(m_pad, d)));
    GPRC_TRY(cross_grad_step(s, mo->ks, b3.p, m_pad, mo->X, m, m_pad, mo->X, m, m_pad, d, part.p, pz.p, 0.5L, 1.0, acc.data(), dz));
  }
  {  // K_fu's part: the fit's pass again
    const bool x_on_device = is_device_ptr(a.X);
    int64_t rows = 0;
    double *vt = nullptr, *sspart = nullptr, *kxx = nullptr;
    struct PitchPad {   // as in sgpr_fit
      gprc_ctx* c; int64_t old;
      explicit PitchPad(gprc_ctx* c_) : c(c_), old(c_->vt_pad) { if (old == 0) c->vt_pad = 16; }
      ~PitchPad() { c->vt_pad = old; }
    } pitch(ctx);
    // the chunk is sized for 2 m_pad columns: V in the first half, G' in the second (so the budget and the retry on a full device
    // cover both; the chunks have half the rows of the fit's)
    GPRC_TRY(chunk_workspace(ctx, 2 * m_pad, pad_up(n, 256), true, &rows, &vt, &sspart, &kxx));
    const int64_t ldv = rows + ctx->vt_pad;
    double* gbuf = vt + ldv * m_pad;
    DevMem xbuf, ybuf, rbuf, rred, part, pz;
    if (!x_on_device) GPRC_TRY(xbuf.alloc(d * rows));
    GPRC_TRY(ybuf.alloc(rows));
    GPRC_TRY(rbuf.alloc(rows));
    GPRC_TRY(rred.alloc(rows * (1 + rowreduce_splits(m_pad))));
    GPRC_TRY(part.alloc(cross_grad_partials(m_pad, np)));
    if (dz) GPRC_TRY(pz.alloc(cross_grad_zpartials(m_pad, d)));
    for (int64_t s0 = 0; s0 < n; s0 += rows) {
      const int64_t mcur = std::min<int64_t>(rows, n - s0), mp = pad_up(mcur, 256);
      const double* xc = a.X + s0 * d;
      if (!x_on_device) {
        GPRC_HIP(hipMemcpyAsync(xbuf.p, xc, sizeof(double) * d * mcur, hipMemcpyHostToDevice, s));
        xc = xbuf.p;
      }
      GPRC_HIP(hipMemsetAsync(ybuf.p, 0, sizeof(double) * (size_t)mp, s));
      GPRC_HIP(hipMemcpyAsync(ybuf.p, a.y + s0, sizeof(double) * mcur, hipMemcpyDefault, s));
      GPRC_TRY(launch_fill(s, mo->ks, xc, mcur, mo->X, m, d, vt, ldv, 0, mp, 0, m_pad, PAD_ZERO, 0.0));
      GPRC_TRY(solve_rows(ctx, mo->packed, mo->winv, m_pad, vt, ldv, mp, nullptr));                          // V
      GPRC_TRY(launch_row_reduce(s, vt, ldv, mp, m_pad, q.p, rred.p, rred.p + mp));                          // V q
      GPRC_TRY(launch_sum_partials(s, rred.p, 1, mp, mp, ybuf.p, rbuf.p));                                   // r = y - V q (zero in the padding)
      GPRC_TRY(launch_rank_one(s, gbuf, ldv, mp, m_pad, rbuf.p, mu.p, 1.0));
      GPRC_TRY(launch_gemm_nt(s, gbuf, ldv, vt, ldv, b1.p, m_pad, mp, m_pad, m_pad, 0, PK_COV_SYRK));     // G' = r mu^T + V T
      GPRC_TRY(cross_grad_step(s, mo->ks, gbuf, ldv, xc, mcur, mp, mo->X, m, m_pad, d, part.p, pz.p, 1.0L / s2, 1.0 / a.noise, acc.data(), dz));
    }
  }
  cross_grad_finish(mo->ks, acc.data(), grad_out);
  // d elbo / d sigma^2
  long double trinv = 0.0L, qq = 0.0L;
  for (int64_t j = 0; j < m; ++j) { trinv -= (long double)hdiag[(size_t)j]; qq += (long double)hq[(size_t)j] * (long double)hq[(size_t)j]; }
  grad_out[np] = (double)(-(long double)n / (2.0L * s2) + ((long double)m - trinv) / (2.0L * s2) + keep.yy / (2.0L * s2 * s2) - keep.cc / (2.0L * s2) -
                          qq / (2.0L * s2) + keep.t / (2.0L * s2 * s2));
  return 0;
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

int gprc_sgpr_elbo_grad(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n, const double* y,
                        double noise, const double* Z, int64_t m, double jitter, double* elbo_out, double* grad_out, double* dZ_out) {
  if (!grad_out) { set_error("sgpr_elbo_grad: null output"); return GPRC_ERR_ARG; }
  GPRC_TRY(check_grad_kernel("sgpr_elbo_grad", kernel));
  ModelPtr mo;
  SgprKeep keep;
  const SgprArgs a{X, y, Z, d, n, m, noise, jitter};
  GPRC_TRY(sgpr_fit_entry("sgpr_elbo_grad", ctx, kernel, params, n_params, a, elbo_out != nullptr, mo, &keep));
  hipStream_t s = ctx->stream;
  Out oz;
  if (dZ_out) GPRC_TRY(oz.set(dZ_out, d * m));
  GPRC_TRY(sgpr_grad(mo.get(), a, keep, grad_out, dZ_out ? oz.dev : nullptr));
  *elbo_out = mo->elbo;
  return finish_sync(s, oz);   // (also: the model's buffers go back to the pool)
}

int gprc_dev_cross_grad(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* G, int64_t ld, const double* A, int64_t rows,
                        const double* Z, int64_t cols, int64_t d, double f, double* grad_out, double* dZ) {
  GPRC_TRY(use_device_unless(ctx, !G || !A || !Z || !grad_out || rows < 1 || cols < 1 || d < 1, "dev_cross_grad: bad arguments"));
  GPRC_TRY(check_grad_kernel("dev_cross_grad", kernel));
  KernelSpec ks;
  GPRC_TRY(make_spec(kernel, params, n_params, d, &ks));
  const int64_t rows_pad = pad_up(rows, PT_R), cols_pad = pad_up(cols, PT_C);
  DevMem part, pz;
  GPRC_TRY(part.alloc(cross_grad_partials(cols_pad, n_params)));
  if (dZ) GPRC_TRY(pz.alloc(cross_grad_zpartials(cols_pad, d)));
  std::vector<long double> acc((size_t)n_params, 0.0L);
  GPRC_TRY(cross_grad_step(ctx->stream, ks, G, ld, A, rows, rows_pad, Z, cols, cols_pad, d, part.p, pz.p, (long double)f, f, acc.data(), dZ));
  cross_grad_finish(ks, acc.data(), grad_out);
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
  GPRC_TRY(ctx_gone("sgpr_get_c", *model));
  GPRC_TRY(use_device(model->ctx));
  GPRC_HIP(hipMemcpyAsync(c_out, model->alpha, sizeof(double) * model->n, hipMemcpyDefault, model->ctx->stream));
  GPRC_HIP(hipStreamSynchronize(model->ctx->stream));
  return 0;
}

int gprc_sgpr_predict(gprc_model* mo, const double* X_star, int64_t ns, double* mean_out, double* var_out) {
  if (!mo || mo->type != MODEL_SGPR) { set_error("sgpr_predict: not a sparse GPR model"); return GPRC_ERR_ARG; }
  if (ns < 0 || (ns > 0 && !X_star) || (!mean_out && !var_out)) { set_error("sgpr_predict: bad arguments (non-null X_star, at least one output)"); return GPRC_ERR_ARG; }
  GPRC_TRY(ctx_gone("sgpr_predict", *mo));
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
  return finish_sync(s, om, ov);
}

}  // extern "C"
