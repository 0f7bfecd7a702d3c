// gprc_paths.hip -- posterior sample paths by pathwise conditioning (Matheron's rule; DESIGN.md section 7, "Posterior sample paths"):
// the gprc_paths object and its entry points, and the two generated-operand products alone (gprc_dev_feature_gemm,
// gprc_dev_kernel_gemm).  Composed from kernels_paths.hip's launchers and the row solve of gprc_sched.hip.
//
//   f_s(x) = sqrt(2 / D) phi(x)^T w_s + sum_j k(x, x_j) U[j, s],      phi_k(x) = cospi(2 (nu_k . x + u_k))
//   U[:, s] = K_y^-1 (y - sqrt(2 / D) Phi(X) w_s - sqrt(noise) e_s),   K_y = K + noise I: the model's factor and its stored noise
//
// create: the prior term at the training points goes into U's own buffer (n x S); S rows at a time (the chunk workspace's rows, S padded to
// 128) the residual is laid out as the rows of a solve chunk, R L^-T by solve_rows, then columns reversed and solve_rows with the reversed
// factor as predict_chunk's variance gradient does: (R L^-T L^-1) J, which paths_weights_kernel reads back into U.  An iterative model
// (MODEL_IGPR, gprc_iter.hip) has no factor: the residual stays n x S and U is its conjugate-gradient solve.
// eval: two products into the caller's array, the prior term first, the update added to it; rows in chunks sized by the context's
// chunk budget.  Memory: rows x S x (1 + stripes) doubles per chunk; no n* x n and no n* x n* buffer.
// eval_grad: the same two products differentiated with respect to the test point (gen_gemm_grad; the values, when asked for, by eval's
// own two launches); rows x S x d x stripes doubles per chunk.  gprc_dev_feature_gemm_grad / gprc_dev_kernel_gemm_grad: each alone.
#include <algorithm>
#include <cmath>
#include <memory>
#include <new>

#include "gprc_host.h"
#include "pair_tile.h"

using namespace gprc;

struct gprc_paths : Bound {
  KernelSpec ks{};
  int64_t n = 0, d = 0, D = 0, S = 0;
  DevMem X;       // d x n: the training points at creation
  DevMem Nu;      // d x D, cycles
  DevMem phase;   // D, turns
  DevMem W;       // D x S
  DevMem U;       // n x S
};

namespace gprc {

// One generated-operand product over all rows, in chunks: a chunk's partials are rows x S x stripes doubles, sized by the context's chunk
// budget (at most 1 GiB).  Results do not depend on the chunking, bit for bit (kernels_paths.hip).
int gen_gemm(gprc_ctx* ctx, const KernelSpec* ks, const double* Bp, const double* phase, int64_t cols, const double* A, int64_t rows, int64_t d,
             const double* B, int64_t ldb, int64_t S, double scale, bool accumulate, double* out, int64_t ld) {
  const int64_t stripes = gen_gemm_stripes(cols);
  const int64_t budget = (int64_t)std::min<size_t>(ctx->chunk_bytes, (size_t)1 << 30);
  int64_t chunk = budget / ((int64_t)sizeof(double) * S * (stripes + 1)) / PT_R * PT_R;
  chunk = std::min(std::max<int64_t>(chunk, PT_R), pad_up(rows, PT_R));
  DevMem part;
  GPRC_TRY(part.alloc(stripes * S * chunk));
  for (int64_t r0 = 0; r0 < rows; r0 += chunk) {
    const int64_t mcur = std::min(chunk, rows - r0);
    GPRC_TRY(launch_gen_gemm(ctx->stream, ks, Bp, phase, cols, A + r0 * d, mcur, pad_up(mcur, PT_R), d, B, ldb, S, scale, accumulate, part.p, out + r0, ld));
  }
  return 0;
}

namespace {

// Its gradient with respect to the rows' points: dout is rows x (S d), pitch ld.  A chunk's partials are rows x S x d x stripes doubles
// inside the same budget, a chunk is never below one row tile, and the bits do not depend on the chunking either.
int gen_gemm_grad(gprc_ctx* ctx, const KernelSpec* ks, const double* Bp, const double* phase, int64_t cols, const double* A, int64_t rows, int64_t d,
                  const double* B, int64_t ldb, int64_t S, double scale, bool accumulate, double* dout, int64_t ld) {
  const int64_t stripes = gen_gemm_stripes(cols);
  const int64_t budget = (int64_t)std::min<size_t>(ctx->chunk_bytes, (size_t)1 << 30);
  int64_t chunk = budget / ((int64_t)sizeof(double) * S * d * stripes) / PT_R * PT_R;
  chunk = std::min(std::max<int64_t>(chunk, PT_R), pad_up(rows, PT_R));
  DevMem part;
  GPRC_TRY(part.alloc(stripes * S * d * chunk));
  for (int64_t r0 = 0; r0 < rows; r0 += chunk) {
    const int64_t mcur = std::min(chunk, rows - r0);
    GPRC_TRY(launch_gen_gemm_grad(ctx->stream, ks, Bp, phase, cols, A + r0 * d, mcur, pad_up(mcur, PT_R), d, B, ldb, S, scale, accumulate, part.p,
                                  dout + r0, ld));
  }
  return 0;
}

int paths_usable(const char* who, const gprc_paths* p) {
  if (!p) return bad(who, "null paths object");
  return ctx_gone(who, *p, "the context of the paths has been destroyed");
}

}  // namespace

}  // namespace gprc

extern "C" {

int gprc_gpr_paths_create(gprc_model* m, const double* Nu, const double* phase, int64_t D, const double* W, const double* E, int64_t S,
                          gprc_paths** paths_out) {
  if (!m || (m->type != MODEL_GPR && m->type != MODEL_IGPR)) {
    set_error("paths_create: not a GPR model (paths of a GPC or a sparse model are not defined here)");
    return GPRC_ERR_ARG;
  }
  const bool iterative = m->type == MODEL_IGPR;   // U by conjugate gradients: no factor, no reversed factor
  if (m->borrowed) {
    set_error("paths_create: the model borrows its buffers (gprc_gpr_model_from_device / gprc_mgpu_model_rank) and cannot own a reversed factor");
    return GPRC_ERR_ARG;
  }
  if (D < 1 || S < 1) { set_error("paths_create: bad arguments (D >= 1 features, S >= 1 paths)"); return GPRC_ERR_ARG; }
  if (!Nu || !phase || !W || !E || !paths_out) { set_error("paths_create: null pointer (Nu, phase, W, E and paths_out are all needed)"); return GPRC_ERR_ARG; }
  if (!has_exact_gradient(m->ks.id)) {
    set_error("paths_create: defined for sqrexp, gammaexp, rationalquadratic and sqrexp_ard, matern32, matern52, matern32_ard and matern52_ard");
    return GPRC_ERR_ARG;
  }
  GPRC_TRY(ctx_gone("paths_create", *m));
  gprc_ctx* ctx = m->ctx;
  GPRC_TRY(use_device(ctx));
  hipStream_t s = ctx->stream;
  const int64_t n = m->n, d = m->d, n_pad = m->n_pad;
  In nu, ph, w, e;
  GPRC_TRY(nu.set(s, Nu, d * D));
  GPRC_TRY(ph.set(s, phase, D));
  GPRC_TRY(w.set(s, W, D * S));
  GPRC_TRY(e.set(s, E, n * S));
  std::unique_ptr<gprc_paths, BoundDelete> p(new (std::nothrow) gprc_paths());
  if (!p) { set_error("out of host memory"); return GPRC_ERR_NOMEM; }
  p->ctx = ctx; p->ctx_id = ctx->id; p->ks = m->ks; p->n = n; p->d = d; p->D = D; p->S = S;
  GPRC_TRY(p->X.copy_from(s, m->X, d * n));
  GPRC_TRY(p->Nu.copy_from(s, nu.dev, d * D));
  GPRC_TRY(p->phase.copy_from(s, ph.dev, D));
  GPRC_TRY(p->W.copy_from(s, w.dev, D * S));
  GPRC_TRY(p->U.alloc(n * S));
  if (!iterative) GPRC_TRY(ensure_reversed_factor(m));
  // the prior term at the training points, sqrt(2 / D) Phi(X) W, into U's buffer
  GPRC_TRY(gen_gemm(ctx, nullptr, p->Nu.p, p->phase.p, D, p->X.p, n, d, p->W.p, D, S, std::sqrt(2.0 / (double)D), false, p->U.p, n));
  if (iterative) {   // U = K_y^-1 (y - prior - sqrt(noise) E) in blocks of right-hand sides (gprc_iter.hip)
    DevMem rhs;
    GPRC_TRY(rhs.alloc(n * S));
    GPRC_HIP(hipMemcpyAsync(rhs.p, p->U.p, sizeof(double) * n * S, hipMemcpyDeviceToDevice, s));
    GPRC_TRY(launch_paths_rhs(s, m->y, rhs.p, n, e.dev, n, std::sqrt(m->noise), n, S));
    GPRC_TRY(igpr_solve_dev(m, rhs.p, n, S, p->U.p, n, nullptr, nullptr, nullptr));
    GPRC_HIP(hipStreamSynchronize(s));
    *paths_out = p.release();
    return 0;
  }
  int64_t rows = 0;
  double *vt = nullptr, *part = nullptr, *unused = nullptr;
  GPRC_TRY(chunk_workspace(ctx, n_pad, S, false, &rows, &vt, &part, &unused));
  const int64_t ldv = rows + ctx->vt_pad;
  const double sqn = std::sqrt(m->noise);
  for (int64_t s0 = 0; s0 < S; s0 += rows) {
    const int64_t scur = std::min(rows, S - s0), m_pad = pad_up(scur, NBI);
    GPRC_TRY(launch_paths_residual(s, m->y, p->U.p, n, e.dev, n, sqn, s0, scur, n, m_pad, n_pad, vt, ldv));
    GPRC_TRY(solve_rows(ctx, m->packed, m->winv, n_pad, vt, ldv, m_pad));            // R L^-T
    GPRC_TRY(launch_reverse_cols(s, vt, ldv, m_pad, n_pad));
    GPRC_TRY(solve_rows(ctx, m->packed_rev, m->winv_rev, n_pad, vt, ldv, m_pad));    // (R L^-T L^-1) J
    GPRC_TRY(launch_paths_weights(s, vt, ldv, n_pad, s0, scur, n, p->U.p, n));
  }
  GPRC_HIP(hipStreamSynchronize(s));   // the staged inputs go out of scope
  *paths_out = p.release();
  return 0;
}

int gprc_gpr_paths_eval(gprc_paths* p, const double* X_star, int64_t ns, double* out, int64_t ld_out) {
  GPRC_TRY(paths_usable("paths_eval", p));
  if (ns < 1 || !X_star || !out) { set_error("paths_eval: bad arguments (n_star >= 1, non-null X_star and out)"); return GPRC_ERR_ARG; }
  if (ld_out < ns) { set_error("paths_eval: ld_out < n_star"); return GPRC_ERR_ARG; }
  gprc_ctx* ctx = p->ctx;
  GPRC_TRY(use_device(ctx));
  hipStream_t s = ctx->stream;
  In xs;
  Out o;
  GPRC_TRY(xs.set(s, X_star, p->d * ns));
  GPRC_TRY(o.set(out, ld_out, ns, p->S));
  GPRC_TRY(gen_gemm(ctx, nullptr, p->Nu.p, p->phase.p, p->D, xs.dev, ns, p->d, p->W.p, p->D, p->S, std::sqrt(2.0 / (double)p->D), false, o.dev, o.ld));
  GPRC_TRY(gen_gemm(ctx, &p->ks, p->X.p, nullptr, p->n, xs.dev, ns, p->d, p->U.p, p->n, p->S, 1.0, true, o.dev, o.ld));
  return finish_sync(s, o);
}

int gprc_gpr_paths_eval_grad(gprc_paths* p, const double* X_star, int64_t ns, double* out, int64_t ld_out, double* dout, int64_t ld_dout) {
  GPRC_TRY(paths_usable("paths_eval_grad", p));
  if (ns < 1 || !X_star) { set_error("paths_eval_grad: bad arguments (n_star >= 1, non-null X_star)"); return GPRC_ERR_ARG; }
  if (!dout) { set_error("paths_eval_grad: null dout (the values alone are gprc_gpr_paths_eval's)"); return GPRC_ERR_ARG; }
  if (ld_dout < ns) { set_error("paths_eval_grad: ld_dout < n_star"); return GPRC_ERR_ARG; }
  if (out && ld_out < ns) { set_error("paths_eval_grad: ld_out < n_star"); return GPRC_ERR_ARG; }
  gprc_ctx* ctx = p->ctx;
  GPRC_TRY(use_device(ctx));
  hipStream_t s = ctx->stream;
  const double scale = std::sqrt(2.0 / (double)p->D);
  In xs;
  Out o, g;
  GPRC_TRY(xs.set(s, X_star, p->d * ns));
  GPRC_TRY(g.set(dout, ld_dout, ns, p->S * p->d));
  if (out) {   // the launches of gprc_gpr_paths_eval with its arguments: its bits
    GPRC_TRY(o.set(out, ld_out, ns, p->S));
    GPRC_TRY(gen_gemm(ctx, nullptr, p->Nu.p, p->phase.p, p->D, xs.dev, ns, p->d, p->W.p, p->D, p->S, scale, false, o.dev, o.ld));
    GPRC_TRY(gen_gemm(ctx, &p->ks, p->X.p, nullptr, p->n, xs.dev, ns, p->d, p->U.p, p->n, p->S, 1.0, true, o.dev, o.ld));
  }
  GPRC_TRY(gen_gemm_grad(ctx, nullptr, p->Nu.p, p->phase.p, p->D, xs.dev, ns, p->d, p->W.p, p->D, p->S, scale, false, g.dev, g.ld));
  GPRC_TRY(gen_gemm_grad(ctx, &p->ks, p->X.p, nullptr, p->n, xs.dev, ns, p->d, p->U.p, p->n, p->S, 1.0, true, g.dev, g.ld));
  return finish_sync(s, g, o);
}

int gprc_gpr_paths_get_weights(gprc_paths* p, double* U_out) {
  GPRC_TRY(paths_usable("paths_get_weights", p));
  if (!U_out) { set_error("paths_get_weights: null output"); return GPRC_ERR_ARG; }
  GPRC_TRY(use_device(p->ctx));
  GPRC_HIP(hipMemcpyAsync(U_out, p->U.p, sizeof(double) * p->n * p->S, hipMemcpyDefault, p->ctx->stream));
  GPRC_HIP(hipStreamSynchronize(p->ctx->stream));
  return 0;
}

int gprc_gpr_paths_dims(const gprc_paths* p, int64_t* n_out, int64_t* d_out, int64_t* D_out, int64_t* S_out) {
  if (!p) { set_error("paths_dims: null paths object"); return GPRC_ERR_ARG; }
  if (n_out) *n_out = p->n;
  if (d_out) *d_out = p->d;
  if (D_out) *D_out = p->D;
  if (S_out) *S_out = p->S;
  return 0;
}

int gprc_gpr_paths_free(gprc_paths* p) { return free_bound(p, delete_bound<gprc_paths>); }

int gprc_dev_feature_gemm(gprc_ctx* ctx, const double* Nu, const double* phase, int64_t D, const double* A, int64_t rows, int64_t d, const double* W,
                          int64_t ldw, int64_t S, double scale, double* out, int64_t ld) {
  GPRC_TRY(use_device_unless(ctx, !Nu || !phase || !A || !W || !out || D < 1 || rows < 1 || d < 1 || S < 1 || ldw < D || ld < rows,
                             "dev_feature_gemm: bad arguments"));
  GPRC_TRY(gen_gemm(ctx, nullptr, Nu, phase, D, A, rows, d, W, ldw, S, scale, false, out, ld));
  GPRC_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int gprc_dev_kernel_gemm(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* A, int64_t rows, const double* Bpts, int64_t cols,
                         int64_t d, const double* U, int64_t ldu, int64_t S, double* out, int64_t ld) {
  GPRC_TRY(use_device_unless(ctx, !A || !Bpts || !U || !out || rows < 1 || cols < 1 || d < 1 || S < 1 || ldu < cols || ld < rows,
                             "dev_kernel_gemm: bad arguments"));
  GPRC_TRY(check_grad_kernel("dev_kernel_gemm", kernel));
  KernelSpec ks;
  GPRC_TRY(make_spec(kernel, params, n_params, d, &ks));
  GPRC_TRY(gen_gemm(ctx, &ks, Bpts, nullptr, cols, A, rows, d, U, ldu, S, 1.0, false, out, ld));
  GPRC_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int gprc_dev_feature_gemm_grad(gprc_ctx* ctx, const double* Nu, const double* phase, int64_t D, const double* A, int64_t rows, int64_t d, const double* W,
                               int64_t ldw, int64_t S, double scale, double* dout, int64_t ld) {
  GPRC_TRY(use_device_unless(ctx, !Nu || !phase || !A || !W || !dout || D < 1 || rows < 1 || d < 1 || S < 1 || ldw < D || ld < rows,
                             "dev_feature_gemm_grad: bad arguments"));
  GPRC_TRY(gen_gemm_grad(ctx, nullptr, Nu, phase, D, A, rows, d, W, ldw, S, scale, false, dout, ld));
  GPRC_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int gprc_dev_kernel_gemm_grad(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* A, int64_t rows, const double* Bpts,
                              int64_t cols, int64_t d, const double* U, int64_t ldu, int64_t S, double* dout, int64_t ld) {
  GPRC_TRY(use_device_unless(ctx, !A || !Bpts || !U || !dout || rows < 1 || cols < 1 || d < 1 || S < 1 || ldu < cols || ld < rows,
                             "dev_kernel_gemm_grad: bad arguments"));
  GPRC_TRY(check_grad_kernel("dev_kernel_gemm_grad", kernel));
  KernelSpec ks;
  GPRC_TRY(make_spec(kernel, params, n_params, d, &ks));
  GPRC_TRY(gen_gemm_grad(ctx, &ks, Bpts, nullptr, cols, A, rows, d, U, ldu, S, 1.0, false, dout, ld));
  GPRC_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

}  // extern "C"
