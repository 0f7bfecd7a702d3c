// gprc_host.h -- what the units of the host layer (see gprc_internal.h for the list) share: the context, the base of every handle that
// lives on one (Bound: the liveness check ctx_gone, the one free free_bound) and the model, scoped device memory that knows whether its
// owner is alive (DevMem), argument staging (In, Out, IntOut, finish_sync), bad(who, msg), the gradient tail, the schedules.
#pragma once
#include <atomic>
#include <cstdio>
#include <limits>
#include <memory>
#include <vector>

#include "gprc_internal.h"

constexpr int SVC_TRACE_PANELS = 48;

struct gprc_ctx {
  uint64_t id = 0;             // unique per context ever created: a model remembers (pointer, id), so a LATER context at the same address is not mistaken for its own
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int* info_dev = nullptr;     // LAPACK info written by the diagonal-block kernel
  void* sync_dev = nullptr;    // 64 bytes of flags for the fused panel kernel (zeroed before every launch, stream-ordered)
                               // + another 64 for launches on the look-ahead stream
  // the factor service's persistent launch runs on a high-priority side stream beside the caller's kernels (factor_group_service)
  hipStream_t side_stream = nullptr;
  hipStream_t side_stream2 = nullptr;  // the shared service's second launch (the 4-wave roles) runs beside the first
  void* svc_trace = nullptr;          // GPRC_SERVICE_TRACE: 16 stamps x SVC_TRACE_PANELS of the last factor-service sweep (measurement)
  hipEvent_t ev_pool[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  unsigned ev_next = 0;
  double* scal_dev = nullptr;  // 8 doubles of scalar results
  size_t chunk_bytes = (size_t)40 << 30;  // budget for one K_star^T chunk (n* = n = 65536 in one piece: fewer, fuller launches)
  // grow-only workspace slots (predict chunks): a multi-GiB hipMalloc/hipFree per call costs 100s of ms
  double* ws[4] = {nullptr, nullptr, nullptr, nullptr};
  int64_t ws_cap[4] = {0, 0, 0, 0};
  int64_t vt_pad = 0;                     // extra doubles in the chunk's leading dimension (keeps it off powers of two)
  // Free-list of device blocks released by calls on this context (exact-size reuse).  fit() evaluates the same n
  // dozens to hundreds of times; without it every dens(v) pays seven hipMalloc/hipFree pairs (each hipFree is a
  // device-wide sync).  Reuse is safe without events: everything on a context runs on its one stream, in order.
  struct Block { void* p; size_t bytes; };
  std::vector<Block> pool;
  size_t pool_bytes = 0;
  size_t pool_cap = (size_t)16 << 30;     // GPRC_POOL_BYTES; blocks larger than the cap are never kept
};

enum ModelType { MODEL_GPR = 1, MODEL_GPC = 2, MODEL_SGPR = 3, MODEL_IGPR = 4 };

// what a handle that lives on a context starts with: gprc_model, gprc_paths, gprc_batch_model, gprc_local_model
struct Bound {
  gprc_ctx* ctx = nullptr;
  uint64_t ctx_id = 0;
};

struct gprc_model : Bound {
  int type = 0;
  gprc::KernelSpec ks{};
  int64_t n = 0, d = 0, n_pad = 0;
  double* X = nullptr;       // d x n
  double* y = nullptr;       // n_pad (zero padded)
  double* packed = nullptr;  // factor, packed block columns
  double* winv = nullptr;    // inverses of the 128x128 diagonal blocks
  double* alpha = nullptr;   // n_pad (GPR) ; g = (y+1)/2 - P (GPC)
  double* f_hat = nullptr;   // GPC
  double* sw = nullptr;      // GPC sqrt(W)
  double* work = nullptr;    // trsv partials
  double* packed_rev = nullptr;  // J L^T J in the packed layout and its diagonal-block inverses: built by the first gprc_gpr_predict_grad that
  double* winv_rev = nullptr;    // wants the variance's gradient, owned by the model (never borrowed), gone after gprc_gpr_extend
  double logp = 0.0, noise = 0.0, logq = 0.0;
  bool borrowed = false;     // X, y, packed, winv, alpha belong to the caller
  // MODEL_SGPR (gprc_sparse.hip): n = m inducing points, X = Z (d x m), packed / winv = L_u, alpha = c, y = nullptr (the training set is
  // not kept); the factor of B, the bound, its trace term, the jitter of K_uu and the number of training points:
  double* packed_b = nullptr;
  double* winv_b = nullptr;
  double elbo = 0.0, trace = 0.0, jitter = 0.0;
  int64_t n_train = 0;
  // MODEL_IGPR (gprc_iter.hip): X, y, alpha = K_y^-1 y by conjugate gradients and noise as a GPR model's; no factor (packed, winv and work
  // stay null).  pq = Q (n x rank, pitch n) of the preconditioner (I - Q Q^T) / noise, null at rank 0; pl = L (the same shape) of
  // P = L L^T + noise I, for the probes of gprc_igpr_logp_grad, and logdet_p = log det P (0 at rank 0, where P = I there); the solver's
  // settings and what the fit's own solve reported:
  double* pq = nullptr;
  double* pl = nullptr;
  double logdet_p = 0.0;
  int64_t rank = 0;
  double cg_tol = 0.0, cg_relres = 0.0, cg_relres_true = 0.0;
  int cg_max_iter = 0, cg_iters = 0;
};

namespace gprc {

// ---- gprc_ctx.hip ------------------------------------------------------------------------------------
int use_device(const gprc_ctx* ctx);   // hipSetDevice + whose pool the scoped temporaries below use (per host thread)
int use_device_unless(const gprc_ctx* ctx, bool bad, const char* msg);   // ... then GPRC_ERR_ARG with msg if `bad`: an entry point's argument check
bool ctx_alive(const gprc_ctx* c, uint64_t id);
int pool_alloc(gprc_ctx* ctx, size_t bytes, void** out);
void pool_release(gprc_ctx* ctx, void* p, size_t bytes);
void pool_trim(gprc_ctx* ctx);
bool is_device_ptr(const void* p);
// workspace slot `slot` of the context, at least `count` doubles (contents undefined)
int ws_get(gprc_ctx* ctx, int slot, int64_t count, double** out);

inline int bad(const char* who, const std::string& msg) { set_error(std::string(who) + ": " + msg); return GPRC_ERR_ARG; }

// 0, or GPRC_ERR_ARG with "<who>: <what>" when the handle's context has been destroyed (the handle may only be freed then)
inline int ctx_gone(const char* who, const Bound& h, const char* what = "the model's context has been destroyed") {
  return h.ctx && ctx_alive(h.ctx, h.ctx_id) ? 0 : bad(who, what);
}
// the *_free entry points: if the context went first its stream is gone (and was synchronised) and its pool too, so f(h) sees ctx == nullptr
template <class H, class Free>
int free_bound(H* h, Free f) {
  if (!h) return 0;
  if (h->ctx && !ctx_alive(h->ctx, h->ctx_id)) {
    h->ctx = nullptr;
    (void)hipDeviceSynchronize();
  }
  if (h->ctx && h->ctx->stream) (void)hipStreamSynchronize(h->ctx->stream);
  f(h);
  return 0;
}
// ... of a handle whose buffers are DevMem members (they know where to go): f is delete_bound<H>, which is also its unique_ptr's deleter
template <class H>
void delete_bound(H* h) {
  if (!h) return;
  if (h->ctx) (void)hipSetDevice(h->ctx->device);
  delete h;
}
struct BoundDelete {
  template <class H>
  void operator()(H* h) const { delete_bound(h); }
};

// Scoped device allocation from the current context's pool.  It remembers its owner as a handle remembers its context, (pointer, id): a
// block released after its owner has gone goes straight back to the driver, so a handle's members need no telling when the context dies first.
struct DevMem {
  double* p = nullptr;
  Bound owner;
  size_t bytes = 0;
  ~DevMem() { reset(); }
  void reset() {   // releases now; the object is empty again
    if (p) pool_release(ctx_alive(owner.ctx, owner.ctx_id) ? owner.ctx : nullptr, p, bytes);
    p = nullptr;
    bytes = 0;
  }
  int alloc(int64_t count);
  int copy_from(hipStream_t s, const double* src, int64_t count);   // alloc + an asynchronous copy of a host or device array
};
struct IntMem {  // scoped int buffer, straight from the driver (not pooled)
  int* p = nullptr;
  ~IntMem() { if (p) (void)hipFree(p); }
};
// Input staging: device pointers pass through, host arrays are copied to a temporary.
struct In {
  const double* dev = nullptr;
  DevMem tmp;
  int set(hipStream_t s, const double* p, int64_t count) {
    if (count <= 0) { dev = nullptr; return 0; }
    if (!p) { set_error("null input pointer"); return GPRC_ERR_ARG; }
    if (is_device_ptr(p)) { dev = p; return 0; }
    GPRC_TRY(tmp.alloc(count));
    GPRC_HIP(hipMemcpyAsync(tmp.p, p, tmp.bytes, hipMemcpyHostToDevice, s));
    dev = tmp.p;
    return 0;
  }
};
// Output staging: device pointers are written in place; host arrays get a temporary + D2H at finish().  The matrix form (rows x
// cols): a device pointer keeps the caller's leading dimension, a host array gets a compact temporary (ld = rows) that finish() copies
// back with the caller's pitch, so rows beyond `rows` of the caller's array are never touched.
struct Out {
  double* dev = nullptr;
  DevMem tmp;
  double* host = nullptr;
  int64_t ld = 0, ld_host = 0, cols = 0;   // matrix form only
  int set(double* p, int64_t cnt) {
    if (cnt <= 0) return 0;
    if (!p) { set_error("null output pointer"); return GPRC_ERR_ARG; }
    if (is_device_ptr(p)) { dev = p; return 0; }
    host = p;
    GPRC_TRY(tmp.alloc(cnt));
    dev = tmp.p;
    return 0;
  }
  int set(double* p, int64_t ld_out, int64_t rows, int64_t ncols) {   // rows, ncols >= 1: callers return early for an empty matrix
    dev = p; ld = ld_out;
    if (is_device_ptr(p)) return 0;
    host = p; ld_host = ld_out; cols = ncols;
    GPRC_TRY(tmp.alloc(rows * ncols));
    dev = tmp.p; ld = rows;
    return 0;
  }
  // an optional vector (null p: nothing is set) that the launch may not write whole: with `keep` a host temporary starts as the caller's
  // array, so what the launch leaves alone comes back as it was
  int set_keeping(double* p, int64_t cnt, bool keep, hipStream_t s) {
    if (!p) return 0;
    GPRC_TRY(set(p, cnt));
    if (host && keep) GPRC_HIP(hipMemcpyAsync(dev, p, sizeof(double) * (size_t)cnt, hipMemcpyHostToDevice, s));
    return 0;
  }
  int finish(hipStream_t s) {   // nothing to do for an Out that was never set, or set to device memory
    if (cols) GPRC_HIP(hipMemcpy2DAsync(host, sizeof(double) * ld_host, tmp.p, sizeof(double) * ld, sizeof(double) * ld, cols, hipMemcpyDeviceToHost, s));
    else if (host) GPRC_HIP(hipMemcpyAsync(host, tmp.p, tmp.bytes, hipMemcpyDeviceToHost, s));
    return 0;
  }
};
// an int array on the device for a host or device destination of `rows` rows of m with pitch ld
struct IntOut {
  int* dev = nullptr;
  int* host = nullptr;
  DevMem tmp;
  int64_t ld = 0, ld_host = 0, m = 0, rows = 0;
  int set(int* p, int64_t ld_out, int64_t rows_, int64_t m_) {
    dev = p; ld = ld_out; m = m_; rows = rows_;
    if (is_device_ptr(p)) return 0;
    host = p; ld_host = ld_out;
    GPRC_TRY(tmp.alloc((rows * m + 1) / 2));
    dev = reinterpret_cast<int*>(tmp.p); ld = m;
    return 0;
  }
  int finish(hipStream_t s) {
    if (host) GPRC_HIP(hipMemcpy2DAsync(host, sizeof(int) * ld_host, dev, sizeof(int) * ld, sizeof(int) * m, rows, hipMemcpyDeviceToHost, s));
    return 0;
  }
};

// the end of an entry point: host outputs (Out, IntOut; unset ones are skipped) are copied back in order, then the stream is waited for
template <class... Outs>
int finish_sync(hipStream_t s, Outs&... outs) {
  int rc = 0;
  ((rc = rc ? rc : outs.finish(s)), ...);
  GPRC_TRY(rc);
  GPRC_HIP(hipStreamSynchronize(s));
  return 0;
}

// The tail of an exact gradient whose device sums lack 1/2 and the factors that do not depend on (i, j): sums (n_params) and dnoise in,
// grad_out (n_params + 1, d / dnoise last) out; all NaN when the model was flagged (!ok)
inline void half_theta_grad(const KernelSpec& ks, const long double* sums, long double dnoise, bool ok, int n_params, double* grad_out) {
  if (!ok) {
    for (int k = 0; k <= n_params; ++k) grad_out[k] = std::numeric_limits<double>::quiet_NaN();
    return;
  }
  long double acc[MAX_PARAMS];   // n_params <= MAX_PARAMS: make_spec
  for (int k = 0; k < n_params; ++k) acc[k] = 0.5L * sums[k];
  cross_grad_finish(ks, acc, grad_out);
  grad_out[n_params] = (double)(0.5L * dnoise);
}

// ---- gprc_sched.hip ----------------------------------------------------------------------------------
extern std::atomic<bool> g_service_off;
int factor_subpanel(gprc_ctx* ctx, double* packed, int64_t n_pad, int64_t p, int j, int part, double* winv, int* info_dev);
int factor_panel(gprc_ctx* ctx, double* packed, int64_t n_pad, int64_t p, double* winv, int* info_dev);
int factor_all_async(gprc_ctx* ctx, double* packed, int64_t n_pad, double* winv, int* info_dev, double* inv, bool* used_service = nullptr);
int factor_all(gprc_ctx* ctx, double* packed, int64_t n_pad, double* winv, int* info_host, double* inv = nullptr, bool* used_service = nullptr);
int solve_rows(gprc_ctx* ctx, const double* packed, const double* winv, int64_t n_pad, double* vt, int64_t ldv, int64_t m_pad,
               double* sspart = nullptr, int64_t tri_row0 = -1, int64_t p_end = -1);
bool identity_solve_dense();
int64_t predict_partials(int64_t n_pad);
int chunk_workspace(gprc_ctx* ctx, int64_t n_pad, int64_t ns, bool want_tmp, int64_t* rows_out, double** vt, double** part, double** tmp);

// factor_all for callers that can rebuild the matrix.  If THIS call ran under the factor service and a device-side wait timed out
// (see g_service_off), the service is switched off for the process (with one line on stderr: it is a permanent change of schedule),
// the matrix is rebuilt (refill) and factored again with one fused launch per panel.  Decided per call, not once per process: two
// host threads that time out in the same window (each with its own context) both retry.
template <class Refill>
int factor_all_or_refill(gprc_ctx* ctx, double* packed, int64_t n_pad, double* winv, int* info_host, double* inv, Refill refill) {
  bool used_service = false;
  int rc = factor_all(ctx, packed, n_pad, winv, info_host, inv, &used_service);
  if (rc == GPRC_ERR_HIP && *info_host == GPRC_INFO_WAIT_TIMEOUT && used_service) {
    if (!g_service_off.exchange(true))
      std::fprintf(stderr, "gprc: a device-side wait of the factor service timed out (kernels of two streams did not run concurrently, e.g. under "
                           "rocprofv3 --pmc); the service is now OFF for this process and the factorisation is repeated with one launch per panel\n");
    GPRC_TRY(refill());
    rc = factor_all(ctx, packed, n_pad, winv, info_host, inv);
  }
  return rc;
}

// ---- gprc_model.hip ----------------------------------------------------------------------------------
int make_spec(int kernel, const double* params, int n_params, int64_t d, KernelSpec* ks);
void free_model(gprc_model* m);
struct ModelFree { void operator()(gprc_model* m) const { free_model(m); } };
using ModelPtr = std::unique_ptr<gprc_model, ModelFree>;   // owns a model: every return frees it unless release() has handed it on
int ensure_reversed_factor(gprc_model* m);   // packed_rev / winv_rev of a model that owns its buffers, built once and kept

// ---- gprc_paths.hip ----------------------------------------------------------------------------------
// out (rows x S, pitch ld) = [out +] scale * G(A, Bp) B, the generated-operand product over all rows in chunks (launch_gen_gemm's arguments)
int gen_gemm(gprc_ctx* ctx, const KernelSpec* ks, const double* Bp, const double* phase, int64_t cols, const double* A, int64_t rows, int64_t d,
             const double* B, int64_t ldb, int64_t S, double scale, bool accumulate, double* out, int64_t ld);

// ---- gprc_iter.hip -----------------------------------------------------------------------------------
// X (n x S, pitch ldx) = K_y^-1 B (pitch ldb) of a MODEL_IGPR by preconditioned conjugate gradients, DEVICE pointers, asynchronous past
// the last block's statistics.  iters, relres, relres_true: S host entries each or null.  Returns 0, GPRC_ERR_MAXITER (every output
// written from the last iterate) or GPRC_ERR_NOT_PD.
// hist: null, or per column the host vector that receives its conjugate-gradient coefficients, alpha_0, beta_0, alpha_1, beta_1, ...:
// 2 iters[s] entries, the last beta unused (S vectors; iters must then be given).  The bits of every other output do not depend on it.
int igpr_solve_dev(gprc_model* m, const double* B, int64_t ldb, int64_t S, double* X, int64_t ldx, int* iters, double* relres, double* relres_true,
                   std::vector<double>* hist = nullptr);

}  // namespace gprc
