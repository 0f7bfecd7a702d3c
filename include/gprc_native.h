/*
 * gprc_native.h -- C ABI of the MI355X-native GP predict hot path (libgprc_native.so).
 *
 * Drop-in boundary for the R package `gprc` (MoHawastaken/Gaussian-Process-Regression).  The
 * reference has NO FFI today (pure R closures / R6 methods); each entry point below names the
 * reference interface (file:line under the reference root) whose arithmetic it replaces.  The `.Call`
 * shim a maintainer adds on the R side is shown in INTEGRATION.md; the Python host mirror used by the
 * tests binds the same symbols through ctypes.
 *
 * Conventions
 *  - plain C, no R / torch / C++ types; sizes are int64_t; every matrix is column-major fp64;
 *  - X is d x n with one observation per COLUMN (R/GPRclass.R:29,132,137): point i = X[i*d .. i*d+d);
 *  - every data pointer may be HOST memory (the `.Call` case: REAL(x)) or DEVICE memory of the
 *    context's GPU (the resident-data case: bench.py, the multi-GPU driver).  The library asks the HIP
 *    runtime which it is; host data is staged through the context's stream, device data is used in
 *    place.  Inputs are borrowed for the duration of the call only;
 *  - ORDERING of device data: every kernel of a call runs on the CONTEXT'S stream (and on side streams the
 *    library orders behind it), never on the null stream, and a context that creates its own stream creates it
 *    non-blocking -- it is NOT ordered with the caller's streams.  Device inputs must therefore be complete on,
 *    or ordered before, the context's stream when the call is made, and device outputs are ready on that stream
 *    when it returns (the fit / predict entry points also synchronise it; the gprc_dev_* building blocks are
 *    asynchronous).  Two ways to satisfy it: (a) pass YOUR stream to gprc_ctx_create -- data produced and
 *    consumed on that stream needs no synchronisation at all; (b) keep the context's own stream and finish the
 *    producers first (hipStreamSynchronize / hipDeviceSynchronize, or an event the context's stream cannot see
 *    is not enough).  A copy still in flight on another stream when the first kernel starts is a data race
 *    (seen once in this repository's own tests: a 1.8 GB clone overwrote the first panel's update);
 *  - return value: 0 = ok; > 0 = LAPACK-style info (order of the first leading minor that is not
 *    positive definite -- what R's chol() reports, R/GPRclass.R:142); < 0 = gprc_status error, with
 *    text in gprc_last_error().  The library never aborts, exits or throws across this boundary;
 *  - a gprc_ctx is bound to one GPU and one HIP stream; calls on one context are serialised by the
 *    caller (R's single thread).  Different contexts may be used from different threads/processes.
 */
#ifndef GPRC_NATIVE_H
#define GPRC_NATIVE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPRC_ABI_VERSION 1

#if defined(__GNUC__)
#define GPRC_API __attribute__((visibility("default")))
#else
#define GPRC_API
#endif

/* Kernel ids and parameter vectors (the `...` of cov_func, R/GPRclass.R:424-427):
 *   GPRC_CONSTANT     params = {c}               R/GPRclass.R:382
 *   GPRC_LINEAR       params = {sigma} or sigma[d] R/GPRclass.R:386
 *   GPRC_POLYNOMIAL   params = {sigma, p}        R/GPRclass.R:390
 *   GPRC_SQREXP       params = {l}               R/GPRclass.R:394
 *   GPRC_GAMMAEXP     params = {l, gamma}        R/GPRclass.R:398
 *   GPRC_RATQUAD      params = {l, alpha}        R/GPRclass.R:402
 *   GPRC_SQREXP_ARD   params = l[d], every l_k > 0: exp(-1/2 sum_k ((x_k - y_k) / l_k)^2)   (no reference counterpart; d <= 256)
 * Matern kernels (no reference counterpart either).  With r = |x - y| and a = sqrt(3) r / l (3/2) or sqrt(5) r / l (5/2); the ARD forms
 * take r / l -> sqrt(sum_k ((x_k - y_k) / l_k)^2).  Every length scale finite and > 0; ARD: n_params == d <= 256.
 *   GPRC_MATERN32     params = {l}               (1 + a) exp(-a)
 *   GPRC_MATERN52     params = {l}               (1 + a + a^2 / 3) exp(-a)
 *   GPRC_MATERN32_ARD params = l[d]              as GPRC_MATERN32
 *   GPRC_MATERN52_ARD params = l[d]              as GPRC_MATERN52
 * nu = 1/2 has no id of its own: it is GPRC_GAMMAEXP {l, 1}, exp(-r / l), which the fill forms from one square root and one exp. */
typedef enum {
  GPRC_CONSTANT = 0,
  GPRC_LINEAR = 1,
  GPRC_POLYNOMIAL = 2,
  GPRC_SQREXP = 3,
  GPRC_GAMMAEXP = 4,
  GPRC_RATQUAD = 5,
  GPRC_SQREXP_ARD = 6,
  GPRC_MATERN32 = 7,
  GPRC_MATERN52 = 8,
  GPRC_MATERN32_ARD = 9,
  GPRC_MATERN52_ARD = 10
} gprc_kernel_id;

typedef enum {
  GPRC_OK = 0,
  GPRC_ERR_ARG = -1,      /* bad argument (the reference's stopifnot() failures) */
  GPRC_ERR_HIP = -2,      /* HIP runtime error */
  GPRC_ERR_NOMEM = -3,    /* allocation failed */
  GPRC_ERR_NOT_PD = -4,   /* all ten jitter attempts failed: "Inputs lead to non positive definite
                             covariance matrix..." (R/GPRclass.R:149) */
  GPRC_ERR_DIVERGED = -5, /* GPC: "Apparently does not converge." (R/GPCclass.R:90-91) */
  GPRC_ERR_MAXITER = -6,  /* GPC: safety cap on IRLS iterations hit (the reference loops forever) */
  GPRC_ERR_NO_DEVICE = -7 /* no usable gfx950 device */
} gprc_status;

typedef struct gprc_ctx gprc_ctx;     /* one GPU + one stream + scratch */
typedef struct gprc_model gprc_model; /* fitted GPR or GPC: device-resident X, y, L, alpha / f_hat */

/* ---- library / device --------------------------------------------------------------------- */
GPRC_API int gprc_abi_version(void);
/* text of the last error on the calling thread ("" if none); valid until the next failing call */
GPRC_API const char* gprc_last_error(void);
GPRC_API int gprc_device_count(int* count_out);
/* stream: a hipStream_t owned by the caller (e.g. a torch.cuda.Stream's handle), or NULL to let the
 * context create and own a non-blocking one (see "ORDERING of device data" above; note that the legacy
 * default stream's handle IS NULL, so it cannot be handed over this way). */
GPRC_API int gprc_ctx_create(int device, void* stream, gprc_ctx** ctx_out);
GPRC_API int gprc_ctx_destroy(gprc_ctx* ctx);
/* GPR$predict / GPC$predict_class work through the test points in chunks of rows of K*^T.  The chunk is sized from
 * GPRC_CHUNK_BYTES (default 40 GiB) but never beyond what hipMemGetInfo reports free; if an allocation still fails
 * the chunk is halved and tried again (down to 256 rows) before the call returns GPRC_ERR_NOMEM.  Results do not
 * depend on the chunking, bit for bit.
 * Gives the device memory a context keeps for reuse back to the driver: the free-list of blocks released by earlier
 * calls (exact-size reuse; fit() evaluates the same n over and over; capped by GPRC_POOL_BYTES, default 16 GiB, 0 = off)
 * and the predict workspaces.  Never needed for correctness. */
GPRC_API int gprc_ctx_trim(gprc_ctx* ctx);
GPRC_API int gprc_ctx_synchronize(gprc_ctx* ctx);

/* ---- L1: covariance-function layer --------------------------------------------------------- */
/* covariance_matrix(A, B, k) (R/GPRclass.R:355-357): out[i + j*ld_out] = k(A[,i], B[,j]),
 * nA x nB.  ld_out >= nA. */
GPRC_API int gprc_kernel_matrix(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* A, int64_t d,
                       int64_t nA, const double* B, int64_t nB, double* out, int64_t ld_out);
/* the closure contract itself (R/GPRclass.R:353-354, the .matrix methods :382-402): for two d x m
 * matrices, out[c] = k(x[,c], y[,c]).  GPR$predict uses it for k(X*,X*) (R/GPRclass.R:164). */
GPRC_API int gprc_kernel_colwise(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* x,
                        const double* y, int64_t d, int64_t m, double* out);

/* ---- L2: GPR ------------------------------------------------------------------------------ */
/* One Cholesky attempt of GPR$initialize (R/GPRclass.R:138,142,152-153): K = k(X,X),
 * L = chol(K + noise*I)^T, alpha = L^-T L^-1 y, logp.  Returns 0 and a model, or info > 0 (no model)
 * when K + noise*I is not positive definite. */
GPRC_API int gprc_gpr_fit(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d,
                 int64_t n, const double* y, double noise, gprc_model** model_out);
/* The whole of R/GPRclass.R:139-151: attempts noise, noise+0.01, ..., noise+0.09; *noise_used is
 * the `$noise` the reference stores, *attempts > 1 means the reference would warn (:144).
 * Returns GPRC_ERR_NOT_PD when all ten fail (:149). */
GPRC_API int gprc_gpr_fit_retry(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d,
                       int64_t n, const double* y, double noise, gprc_model** model_out, double* noise_used,
                       int* attempts);
/* dens(v), the objective of fit() (R/fit.R:117-124): the log marginal likelihood of (kernel, params) on (X, y, noise),
 * i.e. kernel fill + Cholesky + alpha + logp without keeping a model.  Returns 0 and *logp_out, or info > 0 when
 * K + noise*I is not positive definite.  The reference guards with min(det(leading minors)) > 0 (:119, O(n^4));
 * the Cholesky's own info is the same test in exact arithmetic. */
GPRC_API int gprc_gpr_log_marginal(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d,
                          int64_t n, const double* y, double noise, double* logp_out);
/* dens_deriv(v), the gradient fit() hands to optim(method = "BFGS") (R/fit.R:126-139), reproduced with its quirks:
 * K is the NOISE-FREE kernel matrix, alpha = K^-1 y, and component i is
 *   0.5 * sum( diag(alpha alpha^T - K^-1) %*% dK/dv_i )      -- a vector %*% matrix, not a trace (:138);
 * dK/dv comes from cov_dict$<kernel>$deriv (R/fit.R:4-31) with v bound positionally in deriv's OWN argument order
 * (gammaexp: (gamma, l), rationalquadratic: (alpha, l) -- the opposite of the kernels' own order, :10,25).
 * Defined for sqrexp, gammaexp, polynomial, rationalquadratic (:125).  gammaexp's first component is NaN by
 * construction (0 * log 0 on the diagonal).  grad_out: n_params doubles in HOST memory.  Returns 0, or info > 0 when
 * K is not (numerically) positive definite -- the reference's solve(K) fails there with "computationally singular". */
GPRC_API int gprc_fit_gradient(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d,
                      int64_t n, const double* y, double* grad_out);
/* log marginal likelihood of GPR(X, y, noise, kernel(params)) and its exact gradient
 *   d logp / d theta = 1/2 sum_ij (alpha_i alpha_j - (K_y^-1)_ij) dK_y,ij / d theta,   K_y = K + noise * I,  alpha = K_y^-1 y
 * (no reference counterpart: R/fit.R:126-139 and gprc_fit_gradient above keep the reference's form).
 * grad_out: n_params + 1 doubles in HOST memory: d logp / d params[i] in the ABI's parameter order
 * (GPRC_SQREXP {l}; GPRC_GAMMAEXP {l, gamma}; GPRC_RATQUAD {l, alpha}; GPRC_SQREXP_ARD {l_1..l_d}; GPRC_MATERN32, GPRC_MATERN52 {l};
 * GPRC_MATERN32_ARD, GPRC_MATERN52_ARD {l_1..l_d}),
 * then d logp / d noise (noise enters as K + noise * I, un-squared, R/GPRclass.R:139).
 * gammaexp's d/d gamma takes u log(r / l) = 0 at r = 0 (the limit, not the reference's NaN).
 * The whole of L^-1 and of K_y^-1 is held on the device: 2 * gprc_pad(n)^2 doubles of the context's workspace
 * (GPRC_ERR_NOMEM when that does not fit; gprc_ctx_trim releases it).
 * No jitter retry: returns info > 0 (leading minor) when K + noise * I is not positive definite.
 * Other kernel ids: GPRC_ERR_ARG. */
GPRC_API int gprc_gpr_logp_grad(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d,
                                int64_t n, const double* y, double noise, double* logp_out, double* grad_out);
/* gprc_gpr_logp_grad for B small models in one call ("Small models in batches"): one model of at most
 * GPRC_BATCH_MAX_N points per workgroup -- fill, factorisation, alpha, logp and the gradient's contraction without leaving the CU -- so a
 * multi-start search, many outputs over the same inputs or many local models cost one launch per 256 models, not a few per model.
 *   params   HOST: model b's n_params parameters (the ABI's order) at params + b * ld_params, ld_params >= n_params
 *   noise    HOST: B values, each finite and >= 0
 *   X        host or device: model b's points (d x n_max, one point per column, as everywhere) at X + b * x_stride; x_stride = 0: every
 *            model shares one data set; otherwise x_stride >= d * n_max
 *   y        likewise: n_max values at y + b * y_stride; y_stride = 0 (shared) or >= n_max
 *   n_each   HOST, may be NULL (every model has n_max points): 1 <= n_each[b] <= n_max; what lies behind a model's n_each[b] points in
 *            its part of X and y is never read
 *   logp_out HOST, B;   grad_out HOST, B x (n_params + 1), d / d noise last, or NULL (values only);   alpha_out HOST, B x n_max, zero
 *            beyond n_each[b], or NULL;   info_out HOST, B: 0 or the leading minor that is not positive definite
 * A model that is not positive definite does not fail the call: the call returns GPRC_OK, info_out[b] > 0 and that model's logp, gradient
 * and alpha are NaN; no jitter is added.  A model's outputs are the same bits alone (B = 1) and anywhere in any batch, with shared and
 * with strided data, from host and from device pointers, with and without grad_out / alpha_out.  Against gprc_gpr_logp_grad they
 * agree to rounding, not to the bit (another order of multiplications in the kernel value).  Kernels: those of gprc_gpr_logp_grad, any
 * other id is GPRC_ERR_ARG; so are n_max > GPRC_BATCH_MAX_N (use the single-model entry points), an n_each outside 1 .. n_max, a noise
 * that is negative or not finite, a stride that is neither 0 nor at least one model's extent, null params, noise, X, y, logp_out or
 * info_out.  B = 0 returns GPRC_OK.  MEMORY: 2 * 128^2 doubles per model of a launch, at most 64 MiB, from the context's pool. */
#define GPRC_BATCH_MAX_N 128
GPRC_API int gprc_gpr_batch_logp_grad(gprc_ctx* ctx, int kernel, int64_t B, const double* params, int n_params, int64_t ld_params,
                                      const double* noise, const double* X, int64_t d, int64_t n_max, int64_t x_stride, const double* y,
                                      int64_t y_stride, const int64_t* n_each, double* logp_out, double* grad_out, double* alpha_out,
                                      int* info_out);
/* A fitted batch ("Batched predict"): gprc_gpr_batch_logp_grad's models kept as an object that predicts.
 * gprc_gpr_batch_fit takes gprc_gpr_batch_logp_grad's arguments, layout rules and argument errors (model_out must not be NULL either)
 * and runs the same kernel without the gradient: logp_out, info_out and gprc_gpr_batch_get_alpha's values are bit for bit what
 * gprc_gpr_batch_logp_grad returns for the same inputs.  A model that is not positive definite is flagged (info_out[b] > 0, logp NaN)
 * and does not fail the call.  B = 0 returns GPRC_OK and *model_out = NULL.  The object belongs to ctx and owns device copies of the
 * points, alpha, L^-1 of every model, the per-model parameter records, the counts and info; the caller's arrays are not referenced again.
 * MEMORY: 128^2 doubles (128 KiB) per model for L^-1, held until gprc_batch_model_free, plus 128 + d * n_max (or x_stride) + n_max (or
 * y_stride: the targets, which gprc_gpr_batch_loo reads) + n_params + 6 doubles per model; during the fit another 128^2 doubles per model of a launch, at most 32 MiB, from the context's pool.
 *
 * gprc_gpr_batch_predict: the posterior mean and the LATENT variance k(x*, x*) - |L^-1 k*|^2 (unclamped, as gprc_gpr_predict(pointwise = 1))
 * of every model at its own test points, one launch.
 *   X_star   host or device: model b's points (d x ns_max, one point per column) at X_star + b * xs_stride; xs_stride = 0: one set shared
 *            by every model; otherwise xs_stride >= d * ns_max
 *   ns_each  HOST, may be NULL (every model has ns_max points): 1 <= ns_each[b] <= ns_max; what lies behind a model's count is never read
 *   mean_out, var_out   host or device, model b's values at [b * ld_out + j], ld_out >= ns_max; either may be NULL, not both (without
 *            var_out the product with L^-1 is skipped; the mean keeps its bits); entries behind ns_each[b] are left as they were
 * A flagged model's outputs are NaN, its neighbours are unaffected.  A test point's bits depend on its model and its coordinates alone:
 * not on the other test points, their number, the batch, strides, host or device pointers, or which outputs are asked for.  Against
 * gprc_gpr_fit + gprc_gpr_predict they agree to rounding, not to the bit.  GPRC_ERR_ARG: a null model, X_star or both outputs NULL,
 * ns_max < 1, an ns_each outside 1 .. ns_max, a stride that is neither 0 nor at least one model's extent, ld_out < ns_max, a model whose
 * context has been destroyed.
 * gprc_gpr_batch_get_alpha: alpha_out HOST, B x n_max, as gprc_gpr_batch_logp_grad's alpha_out.  gprc_batch_model_dims: each output may
 * be NULL.  gprc_batch_model_free accepts NULL and a model whose context went first. */
typedef struct gprc_batch_model gprc_batch_model;
GPRC_API int gprc_gpr_batch_fit(gprc_ctx* ctx, int kernel, int64_t B, const double* params, int n_params, int64_t ld_params,
                                const double* noise, const double* X, int64_t d, int64_t n_max, int64_t x_stride, const double* y,
                                int64_t y_stride, const int64_t* n_each, gprc_batch_model** model_out, double* logp_out, int* info_out);
GPRC_API int gprc_gpr_batch_predict(gprc_batch_model* model, const double* X_star, int64_t ns_max, int64_t xs_stride, const int64_t* ns_each,
                                    double* mean_out, double* var_out, int64_t ld_out);
/* gprc_gpr_batch_predict with the gradients with respect to the test points, one launch ("Batched prediction
 * gradients and LOO"); the formulas, the conventions and the kernels are gprc_gpr_predict_grad's:
 *   d mean / d x*_c = sum_k alpha_k dk(x*, x_k) / d x*_c,     d var / d x*_c = -2 sum_k u_k dk(x*, x_k) / d x*_c,  u = K_y^-1 k*,
 * dk / d x*_c = -h (x*_c - x_kc) t_c; a gammaexp pair at distance 0 contributes 0; Matern is finite at a training point.
 *   X_star, ns_max, xs_stride, ns_each, mean_out, var_out, ld_out   exactly gprc_gpr_batch_predict's
 *   dmean_out, dvar_out   host or device: model b's gradient of test point j with respect to coordinate c at [b * ld_grad + d * j + c]
 *            (X_star's own layout, as gprc_gpr_predict_grad), ld_grad >= d * ns_max; entries behind ns_each[b] points are left as they were
 * Each of the four outputs may be NULL, not all four; without dvar_out the product with L^-T is not formed, without var_out and dvar_out
 * L^-1 is not read.  mean_out and var_out are bit for bit gprc_gpr_batch_predict's, whichever outputs are asked for.  The gradient bits
 * of a test point depend on its model and its coordinates alone: not on the other test points, their number, the batch, strides, host or
 * device pointers, or which outputs are asked for.  A flagged model's outputs are NaN, its neighbours are unaffected.  Against
 * gprc_gpr_fit + gprc_gpr_predict_grad they agree to rounding, not to the bit.  GPRC_ERR_ARG: gprc_gpr_batch_predict's (all four outputs
 * NULL in place of both), and ld_grad < d * ns_max with a gradient asked for.
 *
 * gprc_gpr_batch_loo: leave-one-out cross-validation of every model in closed form, one launch, from what the object keeps: with
 * p_i = sum_{k >= i} (L^-1)_ki^2 = (K_y^-1)_ii, for i < n_b
 *   mean_i = y_i - alpha_i / p_i,     var_i = 1 / p_i  (of the NOISY y_i, as gprc_gpr_loo),
 *   logdens_i = 1/2 log p_i - alpha_i^2 / (2 p_i) - 1/2 log(2 pi).
 *   mean_out, var_out, logdens_out   host or device: model b's values at [b * ld_out + i], ld_out >= n_max; entries behind n_b are left
 *            as they were
 *   loo_out  HOST, B: sum_i logdens_i of every model, summed on the device in a fixed order (entries i and i + 64 first, then a binary
 *            tree over the 64 pairs): the same bits on every call and in any batch
 * Each of the four may be NULL, not all four.  A flagged model gets NaN.  GPRC_ERR_ARG: a null model, all four outputs NULL,
 * ld_out < n_max with one of the three arrays asked for, a model whose context has been destroyed. */
GPRC_API int gprc_gpr_batch_predict_grad(gprc_batch_model* model, const double* X_star, int64_t ns_max, int64_t xs_stride,
                                         const int64_t* ns_each, double* mean_out, double* var_out, int64_t ld_out, double* dmean_out,
                                         double* dvar_out, int64_t ld_grad);
GPRC_API int gprc_gpr_batch_loo(gprc_batch_model* model, double* mean_out, double* var_out, double* logdens_out, int64_t ld_out,
                                double* loo_out);
GPRC_API int gprc_gpr_batch_get_alpha(gprc_batch_model* model, double* alpha_out);
GPRC_API int gprc_batch_model_dims(const gprc_batch_model* model, int64_t* B_out, int64_t* d_out, int64_t* n_max_out);
GPRC_API int gprc_batch_model_free(gprc_batch_model* model);
/* Laplace GP classifiers in batches ("Batched and local GPC"): gprc_gpc_fit (flags = 0) for B small models in one
 * call, one model of at most GPRC_BATCH_MAX_N points per workgroup -- K, every Newton iteration of the mode search from f = 0, the stop
 * rule |objective - last| < epsilon and the final factorisation of B = I + sqrt(W) K sqrt(W) without leaving the CU or asking the host.
 *   params, X, y, n_each, the strides   exactly gprc_gpr_batch_fit's (there is no noise); y in {-1, +1}, not checked on the device
 *   epsilon    > 0, the absolute stop threshold;   max_iter <= 0 selects 100, at most 1000
 *   logq_out   HOST, B: objective - sum log L_ii at the mode, the Laplace log evidence (gprc_gpc_logq_grad's value)
 *   iters_out  HOST, B, may be NULL: the Newton iterations taken
 *   info_out   HOST, B: 0 converged; k > 0 the first non-positive pivot of B, 1-based (B has eigenvalues >= 1: only non-finite input gives
 *              one); GPRC_BATCH_GPC_MAXITER the cap was reached; GPRC_BATCH_GPC_NONFINITE the objective was not finite
 * A flagged model (info != 0) stops at once, is not retried and does not fail the call: GPRC_OK, and its logq, f_hat and every
 * prediction are NaN; the other models are unaffected.  A model's outputs are the same bits alone (B = 1) and anywhere in any batch --
 * however long the other models iterate --, with shared and with strided data, from host and from device pointers, with and without
 * iters_out, on every call.  Against gprc_gpc_fit they agree to rounding, and the iteration counts to one step where a decrement lies
 * within rounding of epsilon.  The object is a gprc_batch_model of the classifier kind: gprc_batch_model_dims and gprc_batch_model_free
 * serve it; gprc_gpr_batch_predict, _predict_grad, _loo and _get_alpha return GPRC_ERR_ARG for it, as the gprc_gpc_batch_* calls do for a
 * regression batch.  B = 0 returns GPRC_OK and *model_out = NULL.
 * MEMORY: 128^2 doubles (128 KiB) per model for L^-1 diag(sqrt(W)), held until gprc_batch_model_free, plus 2 * 128 + d * n_max (or
 * x_stride) + n_max (or y_stride) + n_params + 6 doubles per model; during the fit another 128^2 doubles (K) per model of a launch, at
 * most 32 MiB, from the context's pool.
 * GPRC_ERR_ARG: gprc_gpr_batch_fit's cases (a null context, params, X, y, model_out, logq_out or info_out, a kernel outside the eight,
 * n_max > GPRC_BATCH_MAX_N, n_max < 1, d < 1, n_params < 1, ld_params < n_params, a stride that is neither 0 nor at least one model's
 * extent, an n_each outside 1 .. n_max), epsilon not > 0, max_iter > 1000.
 *
 * gprc_gpc_batch_predict_latent: fs_bar = k*^T g and Vfs = k(x*, x*) - |L^-1 (sqrt(W) o k*)|^2 (R/GPCclass.R:112-115, as
 * gprc_gpc_predict_latent) of every model at its own test points: gprc_gpr_batch_predict's launch, arguments, layout, bit rules and
 * argument errors, on the stored g and L^-1 diag(sqrt(W)); either output may be NULL, not both.
 * gprc_gpc_batch_predict_class: P(y* = +1) of every model at its test points, gprc_gpc_predict_class's integral (the reference's use of
 * the variance as dnorm's sd included) over the latent prediction; prob_out host or device, model b's values at [b * ld_out + j],
 * entries behind ns_each[b] are left as they were; MEMORY: 2 * B * ld_out doubles from the context's pool.  GPRC_ERR_ARG: the latent
 * call's cases, a null prob_out.
 * gprc_gpc_batch_get_f_hat: f_hat_out HOST, B x n_max: the modes, zero behind n_b, NaN for a flagged model. */
#define GPRC_BATCH_GPC_MAXITER (-1)
#define GPRC_BATCH_GPC_NONFINITE (-2)
GPRC_API int gprc_gpc_batch_fit(gprc_ctx* ctx, int kernel, int64_t B, const double* params, int n_params, int64_t ld_params, const double* X,
                                int64_t d, int64_t n_max, int64_t x_stride, const double* y, int64_t y_stride, const int64_t* n_each,
                                double epsilon, int max_iter, gprc_batch_model** model_out, double* logq_out, int* iters_out,
                                int* info_out);
GPRC_API int gprc_gpc_batch_predict_latent(gprc_batch_model* model, const double* X_star, int64_t ns_max, int64_t xs_stride,
                                           const int64_t* ns_each, double* fs_bar_out, double* Vfs_out, int64_t ld_out);
GPRC_API int gprc_gpc_batch_predict_class(gprc_batch_model* model, const double* X_star, int64_t ns_max, int64_t xs_stride,
                                          const int64_t* ns_each, double* prob_out, int64_t ld_out);
GPRC_API int gprc_gpc_batch_get_f_hat(gprc_batch_model* model, double* f_hat_out);
/* Exact k-nearest-neighbours by brute force in float64 ("Local GPR"): for every test point j the m training points
 * with the smallest key (dist2, index), lexicographic -- the lower index first among equal distances -- in ascending key order,
 *   dist2(j, i) = sum_c ((x*_jc - x_ic) * s_c)^2,   c ascending, one fused multiply-add per term;  s_c = 1 without a scale.
 * The difference is taken before the scaling: a test point that coincides with a training point has distance exactly 0.
 *   X, X_star   host or device, d x n and d x n_star, one point per column;  n < 2^31, any d >= 1, n_star >= 0 (0: nothing is done)
 *   scale       HOST, d values, finite and > 0, or NULL
 *   m           1 <= m <= min(n, 128)
 *   idx_out, dist_out   host or device (both of one kind), the result of point j at [j * ld_out + r], r < m; ld_out >= m; what lies
 *               between m and ld_out is left as it was; dist_out may be NULL
 * Indices and distance bits are a function of (X, X_star, scale, m) alone: not of n_star, a point's place in the call, the tiling, or
 * host versus device pointers.  A distance that is NaN is never selected; a rank that no comparable candidate fills reports index -1
 * and distance +inf.  n * n_star * d multiply-adds, no n x n_star memory.  GPRC_ERR_ARG: a null context, X, X_star or idx_out, d < 1,
 * n < 1, n >= 2^31, m outside 1 .. min(n, 128), ld_out < m, a scale that is not finite and > 0 or not in host memory.
 *
 * The local GPR: every test point is predicted from the exact GP of its own m nearest training points (local kriging).
 * gprc_lgpr_create copies X and y to the device once and factorises nothing; kernels: those of gprc_gpr_batch_logp_grad; m is clamped
 * to min(m, n, 128).  The neighbours are those of gprc_dev_knn, for the ARD kernels with s_c = 1 / l_c from the parameters -- the
 * points of largest prior correlation -- and Euclidean for the others.  gprc_lgpr_set_params swaps parameters and noise without
 * another upload.  gprc_lgpr_predict: per chunk of at most 2048 test points the neighbour search, then gprc_gpr_batch_fit and
 * gprc_gpr_batch_predict on one model per point, its points in neighbour order.
 *   X_star              host or device, d x n_star
 *   mean_out, var_out   host or device, n_star values; the LATENT variance, as gprc_gpr_batch_predict's; var_out may be NULL
 *   info_out            HOST, n_star ints, may be NULL: 0, or the leading minor of point j's local model that is not positive definite;
 *                       such a point's mean and variance are NaN, the call does not fail and the other points are unaffected
 * A test point's bits depend on the model, the parameters and its own coordinates only: not on n_star, the chunk it falls into or its
 * place.  MEMORY: d * n + n doubles held by the object; during a predict 128 KiB + (d + 2) m doubles per point of a chunk, at most 256 MiB
 * + the slabs, from the context's pool.  gprc_lgpr_neighbours: gprc_dev_knn with the model's points, m and metric.
 * GPRC_ERR_ARG: a null context, model or pointer (var_out, info_out, dist_out may be NULL), a kernel outside the eight, bad parameters or
 * noise (gprc_gpr_batch_fit's rules), m < 1, n >= 2^31, ld_out < m, a model whose context has been destroyed.  gprc_lgpr_free accepts NULL
 * and a model whose context went first; gprc_lgpr_dims: each output may be NULL. */
GPRC_API int gprc_dev_knn(gprc_ctx* ctx, const double* X, int64_t d, int64_t n, const double* X_star, int64_t n_star, const double* scale,
                          int64_t m, int* idx_out, double* dist_out, int64_t ld_out);
typedef struct gprc_local_model gprc_local_model;
GPRC_API int gprc_lgpr_create(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n,
                              const double* y, double noise, int64_t m, gprc_local_model** model_out);
GPRC_API int gprc_lgpr_set_params(gprc_local_model* model, const double* params, int n_params, double noise);
GPRC_API int gprc_lgpr_predict(gprc_local_model* model, const double* X_star, int64_t n_star, double* mean_out, double* var_out,
                               int* info_out);
GPRC_API int gprc_lgpr_neighbours(gprc_local_model* model, const double* X_star, int64_t n_star, int* idx_out, double* dist_out,
                                  int64_t ld_out);
GPRC_API int gprc_lgpr_dims(const gprc_local_model* model, int64_t* n_out, int64_t* d_out, int64_t* m_out);
GPRC_API int gprc_lgpr_free(gprc_local_model* model);
/* The local classifier ("Batched and local GPC"): every test point is classified by the Laplace GPC of its own m
 * nearest training points.  gprc_lgpc_create is gprc_lgpr_create without the noise and with the mode search's epsilon (> 0) and max_iter
 * (<= 0 selects 100, at most 1000); y in {-1, +1}; the object is a gprc_local_model of the classifier kind: gprc_lgpr_neighbours,
 * gprc_lgpr_dims and gprc_lgpr_free serve it; gprc_lgpr_predict, gprc_lgpr_set_params and the three gprc_lgpr_vecchia_* calls return
 * GPRC_ERR_ARG for it, as the gprc_lgpc_* calls do for a regression object.  gprc_lgpc_set_params swaps the parameters without another
 * upload.  gprc_lgpc_predict: per chunk of at most 2048 test points the neighbour search in the model's metric, the gather,
 * gprc_gpc_batch_fit on one model per point (its points in neighbour order), the latent prediction and the class probability.
 *   X_star                           host or device, d x n_star
 *   fs_bar_out, Vfs_out, prob_out    host or device, n_star values each: gprc_gpc_batch_predict_latent's and _class's; each may be NULL,
 *                                    not all three; the others keep their bits
 *   iters_out, info_out              HOST, n_star ints, may be NULL: gprc_gpc_batch_fit's of point j's local model; a flagged point's
 *                                    outputs are NaN, the call does not fail and the other points are unaffected
 * A test point's bits depend on the model, the parameters and its own coordinates only: not on n_star, the chunk it falls into or its
 * place.  MEMORY: d * n + n doubles held by the object; during a predict 128 KiB + (d + 2) m + 2 * 128 doubles per point of a chunk, at most
 * 256 MiB + the slabs and 32 MiB of K, from the context's pool.
 * GPRC_ERR_ARG: gprc_lgpr_create's and gprc_lgpr_predict's cases, epsilon not > 0, max_iter > 1000, all three outputs NULL, iters_out or
 * info_out in device memory, an object of the other kind. */
GPRC_API int gprc_lgpc_create(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n,
                              const double* y, int64_t m, double epsilon, int max_iter, gprc_local_model** model_out);
GPRC_API int gprc_lgpc_set_params(gprc_local_model* model, const double* params, int n_params);
GPRC_API int gprc_lgpc_predict(gprc_local_model* model, const double* X_star, int64_t n_star, double* fs_bar_out, double* Vfs_out,
                               double* prob_out, int* iters_out, int* info_out);
/* The predecessor-constrained search (the conditioning sets of the Vecchia likelihood below): for every query i in [first, first + count),
 * a column of X itself, the m smallest keys (dist2, j) among the columns j < i of X.  Distance formula, key, tie rule, NaN rule and the
 * layout of idx_out / dist_out (query i at row i - first) are exactly gprc_dev_knn's; ranks that no candidate fills (i < m) report -1
 * and +inf.  1 <= m <= 128 (m may exceed n), n < 2^31, 0 <= first, 0 <= count (0: nothing is done), first + count <= n.  Results are a
 * function of (X, scale, m, i) alone: not of first, count, the tiling, the split, or host versus device pointers.  About half the pair
 * work of gprc_dev_knn with n_star = n.  GPRC_ERR_ARG: gprc_dev_knn's cases, and a window outside 0 .. n.
 *
 * The Vecchia likelihood of the local GPR ("Vecchia likelihood"; the likelihood of a nearest-neighbour GP): with
 * the order of conditioning the column order of X,
 *   log p_V(y) = sum_i log p(y_i | y_N(i)),   N(i) = the min(m_cond, i) points j < i with the smallest key (dist2, j),
 * the exact log marginal likelihood when m_cond >= n - 1, n independent models of at most m_cond + 1 points, and its exact gradient.
 * gprc_lgpr_vecchia_prepare searches once (gprc_dev_knn_before) in the model's CURRENT metric -- 1 / l_c from the parameters of
 * gprc_lgpr_create or gprc_lgpr_set_params for the ARD kernels, Euclidean otherwise -- and keeps n x m_cond 32-bit indices on the device
 * in the object; 1 <= m_cond <= 127, clamped to n - 1 (n = 1 keeps nothing: the sum is the one marginal).  A second prepare replaces the
 * first; gprc_lgpr_set_params does not touch the stored neighbours: they are frozen until the next prepare, so the objective is smooth
 * in the parameters.  gprc_lgpr_vecchia_logp_grad evaluates at the GIVEN parameters and noise (the object's own are unchanged):
 *   grad_out     HOST, n_params + 1 entries, d / d noise last; may be NULL for the value alone, with the same value bits
 *   cond_out     host or device, n entries log p(y_i | y_N(i)), or NULL
 *   flagged_out  HOST, the number of points whose model is not positive definite, or NULL.  With any flagged point *logp_out and grad_out
 *                are NaN and the call returns GPRC_OK; cond_out is NaN exactly at the flagged points, the others keep their bits
 * Kernels: those of gprc_gpr_batch_logp_grad.  One model per workgroup, factored in LDS (Cholesky only: no inverse, nothing of size
 * (m_cond + 1)^2 leaves the CU); launches of at most GPRC_VECCHIA_CHUNK points, a multiple of 256; the device adds groups of 256
 * consecutive points by global index in a fixed order and the host adds the groups' rows in order in long double: value, gradient and
 * cond_out have the same bits on every call, for host and device pointers and whichever outputs are asked for, and cond_i depends on
 * (X, y, N(i), the parameters) alone.  MEMORY: d * n + n doubles (as before) + 4 * n * m_cond bytes held by the object; per launch
 * (n_params + 2) doubles and one int a point, n_params + 3 doubles per 256 points of the call.
 * gprc_lgpr_vecchia_neighbours: the stored indices, row i at idx_out + i * ld_out (host or device; ld_out >= m_cond), -1 at ranks >= i.
 * GPRC_ERR_ARG: a null model or pointer (grad_out, cond_out, flagged_out may be NULL), m_cond outside 1 .. 127, bad parameters or noise
 * (gprc_lgpr_create's rules), no prepare yet (n > 1), ld_out < m_cond, a model whose context has been destroyed. */
#define GPRC_VECCHIA_CHUNK 16384
GPRC_API int gprc_dev_knn_before(gprc_ctx* ctx, const double* X, int64_t d, int64_t n, int64_t first, int64_t count, const double* scale,
                                 int64_t m, int* idx_out, double* dist_out, int64_t ld_out);
GPRC_API int gprc_lgpr_vecchia_prepare(gprc_local_model* model, int64_t m_cond);
GPRC_API int gprc_lgpr_vecchia_logp_grad(gprc_local_model* model, const double* params, int n_params, double noise, double* logp_out,
                                         double* grad_out, double* cond_out, int64_t* flagged_out);
GPRC_API int gprc_lgpr_vecchia_neighbours(gprc_local_model* model, int* idx_out, int64_t ld_out);
/* Leave-one-out cross-validation of a fitted GPR model in closed form (Rasmussen & Williams 5.4.2; no reference counterpart).  With
 * K_y = K + noise * I, P = K_y^-1, alpha = P y and p_i = P_ii, the prediction of y_i from the other n - 1 observations is
 *   mean_i = y_i - alpha_i / p_i,     var_i = 1 / p_i,     logdens_i = 1/2 log p_i - alpha_i^2 / (2 p_i) - 1/2 log(2 pi),
 * and *loo_out = sum_i logdens_i, the LOO log predictive probability.  var_i is the variance of the NOISY observation y_i: it contains
 * `noise` (gprc_gpr_predict's variance on the other n - 1 points is var_i - noise).  mean_out, var_out, logdens_out: n doubles each,
 * host or device pointers as gprc_gpr_predict's; loo_out: one double in HOST memory, the sum taken in index order in long double (two
 * calls give the same bits).  Each of the four may be NULL (not all).  p_i = sum_k (L^-1)_ki^2 comes from the rows of L^-T, chunk by
 * chunk as gprc_fit_gradient: n^3 / 3 flop, MEMORY: the context's predict chunk, no n^2 buffer -- the call works at every n a fit
 * works at -- and the results do not depend on the chunking, bit for bit.  The model is only read: every GPR model is accepted, the
 * borrowed ones (gprc_gpr_model_from_device, gprc_mgpu_model_rank) included, with every kernel id.
 * GPRC_ERR_ARG: a GPC model, all four outputs NULL. */
GPRC_API int gprc_gpr_loo(gprc_model* model, double* mean_out, double* var_out, double* logdens_out, double* loo_out);
/* The LOO log predictive probability of GPR(X, y, noise, kernel(params)), *loo_out as gprc_gpr_loo's, and its exact gradient: with
 * w_i = alpha_i / p_i, c_i = (p_i + alpha_i^2) / p_i^2, u = P w,
 *   d LOO / d theta = 1/2 sum_ij M_ij dK_ij / d theta,   M = u alpha^T + alpha u^T - P diag(c) P,     d LOO / d noise = 1/2 sum_i M_ii.
 * The contract is gprc_gpr_logp_grad's: grad_out: n_params + 1 doubles in HOST memory, d LOO / d params[i] in the ABI's parameter
 * order, then d LOO / d noise; kernels GPRC_SQREXP, GPRC_GAMMAEXP, GPRC_RATQUAD, GPRC_SQREXP_ARD, GPRC_MATERN32, GPRC_MATERN52,
 * GPRC_MATERN32_ARD, GPRC_MATERN52_ARD (other ids: GPRC_ERR_ARG); gammaexp's d/d gamma takes u log(r / l) = 0 at r = 0.
 * MEMORY: P and its column-scaled full copy P diag(sqrt c) are held whole, 2 * gprc_pad(n)^2 doubles of the context's workspace
 * (GPRC_ERR_NOMEM when that does not fit; gprc_ctx_trim releases it).  About 2 n^3 flop: the fit, the inverse and one n^3 product.
 * No jitter retry: returns info > 0 (leading minor) when K + noise * I is not positive definite. */
GPRC_API int gprc_gpr_loo_grad(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d,
                               int64_t n, const double* y, double noise, double* loo_out, double* grad_out);
/* GPR$predict (R/GPRclass.R:155-170).  X_star is d x n_star.
 * pointwise != 0: mean_out[n_star], var_out[n_star] = k(x*,x*) - colSums(v*v)      (:164-165)
 * pointwise == 0: mean_out[n_star], var_out = n_star x n_star K(X*,X*) - t(v) %*% v (:167-168) */
GPRC_API int gprc_gpr_predict(gprc_model* model, const double* X_star, int64_t n_star, int pointwise, double* mean_out,
                     double* var_out);
/* The posterior mean and pointwise variance at the test points AND their gradients with respect to the test points -- what maximising
 * an acquisition function over x* needs (no reference counterpart).  With k*_j = k(x*, x_j), v = L^-1 k*, w = L^-T v = K_y^-1 k*:
 *   d mu / d x*_c = sum_j alpha_j dk(x*, x_j) / d x*_c,     d sigma^2 / d x*_c = -2 sum_j w_j dk(x*, x_j) / d x*_c
 * (d k(x*, x*) / d x* = 0: the kernels are stationary).  X_star: d x n_star.  mean_out, var_out: n_star doubles each, bit for bit what
 * gprc_gpr_predict(pointwise = 1) returns; dmean_out, dvar_out: d x n_star column-major (X_star's layout).  Each of the four may be
 * NULL (not all): without dvar_out the second solve is skipped, without var_out as well the first one too -- the mean's gradient alone
 * is one pass over the pairs.  All pointers host or device, as gprc_gpr_predict.  Results do not depend on the chunking, bit for bit.
 * Kernels: GPRC_SQREXP, GPRC_SQREXP_ARD, GPRC_GAMMAEXP, GPRC_RATQUAD, GPRC_MATERN32, GPRC_MATERN52, GPRC_MATERN32_ARD, GPRC_MATERN52_ARD
 * (the Matern derivatives hold no 1 / r: a test point on a training point contributes an exact 0 without a convention).  gammaexp at a test point that EQUALS a training point (r = 0):
 * that pair contributes 0 -- the limit for gamma > 1, a convention for gamma <= 1, where the kernel is not differentiable there.
 * MEMORY: the variance's gradient needs W = V L^-1, which the row solve (V L^-T only) computes with the REVERSED factor J L^T J.  It is
 * built by the first call that passes dvar_out and kept in the model: a second copy of the factor and of its block inverses,
 * gprc_packed_size + gprc_winv_size doubles (17 GB at n = 65536).  GPRC_ERR_NOMEM, with the size in the text, when it cannot be
 * allocated: the model stays usable for everything else.  gprc_model_free releases it, gprc_gpr_extend drops it (the next call
 * rebuilds it); gprc_ctx_trim does NOT release it: it belongs to the model, not to the context's workspace.
 * GPRC_ERR_ARG: a GPC model, a borrowed model (gprc_gpr_model_from_device, gprc_mgpu_model_rank), n_star < 1, all four outputs NULL,
 * a kernel without a gradient (constant, linear, polynomial). */
GPRC_API int gprc_gpr_predict_grad(gprc_model* model, const double* X_star, int64_t n_star, double* mean_out, double* var_out,
                                   double* dmean_out, double* dvar_out);
/* Posterior sample paths by pathwise conditioning (Matheron's rule; Wilson et al. 2020; no reference counterpart): S functions drawn
 * from the posterior of a fitted GPR model that can be evaluated anywhere, again and again, at O(D + n) per test point and path:
 *   f_s(x) = sqrt(2 / D) sum_k cos 2 pi(nu_k . x + u_k) W[k, s]  +  sum_j k(x, x_j) U[j, s]
 *   U[:, s] = K_y^-1 (y - sqrt(2 / D) Phi(X) W[:, s] - sqrt(noise) E[:, s]),     K_y = K + noise I
 * with the model's stored noise (the variance, a jitter of the fit included) and its factor.  The caller draws, the library is
 * deterministic: Nu (d x D, one frequency per column, in CYCLES: omega / 2 pi, from the kernel's spectral density), phase (D, in
 * TURNS, uniform on [0, 1)), W (D x S) and E (n x S) standard normal, all column-major, host or device.  The mean of the paths over
 * W and E is the exact posterior mean whatever the features.
 * create computes U once (the model's row solve on S right-hand sides, then the same with the REVERSED factor: memory and failure text
 * of that second copy of the factor exactly as for gprc_gpr_predict_grad's variance gradient, and kept in the model likewise).  A
 * gprc_paths holds its own copies of X, the kernel, Nu, phase, W and U: it describes the posterior AT CREATION and stays valid after
 * gprc_gpr_extend or gprc_model_free of the model; it dies with gprc_gpr_paths_free.  After its context is destroyed every call on it
 * but free and dims returns GPRC_ERR_ARG.
 * eval: out[i + s ld_out] = f_s(X_star[, i]), n_star x S column-major; X_star (d x n_star) and out host or device.  Chunked over the
 * test points, rows x S x (1 + stripes) doubles of workspace per chunk and no n_star x n buffer; bit for bit the same under every
 * chunking, and for a point evaluated alone or in a batch.
 * get_weights: U (n x S, column-major, host or device).  dims: any output may be NULL.
 * GPRC_ERR_ARG, each with text: a GPC, sparse or borrowed model; a kernel outside GPRC_SQREXP, GPRC_SQREXP_ARD, GPRC_GAMMAEXP,
 * GPRC_RATQUAD and the four Matern ids; D < 1, S < 1, n_star < 1, null pointers; ld_out < n_star. */
typedef struct gprc_paths gprc_paths;
GPRC_API int gprc_gpr_paths_create(gprc_model* model, const double* Nu, const double* phase, int64_t D, const double* W, const double* E,
                                   int64_t S, gprc_paths** paths_out);
GPRC_API int gprc_gpr_paths_eval(gprc_paths* paths, const double* X_star, int64_t n_star, double* out, int64_t ld_out);
/* The gradient of every path with respect to the test point, and optionally the values with it:
 *   dout[i + ld_dout (s + S c)] = d f_s / d x_c at X_star[, i]
 *     = -2 pi sqrt(2 / D) sum_k Nu[c, k] sin 2 pi(nu_k . x + u_k) W[k, s]  -  t_c sum_j h(x, x_j) (x_c - x_jc) U[j, s]
 * n_star x S x d, the coordinate slowest; h and t_c as for gprc_gpr_predict_grad (gammaexp: h = 0 at a training point; Matern: finite
 * there).  out: NULL, or n_star x S with the bits of gprc_gpr_paths_eval (its launches with its arguments).  Host or device pointers.
 * Both terms are generated-operand products as in eval, one operand per coordinate: the weight of a pair is formed once, the direct
 * difference x_c - x_jc is taken per coordinate.  Chunked over the test points: rows x S x d x stripes doubles of workspace per chunk
 * (at most 1 GiB or the context's chunk budget, never below 128 rows); the same bits under every chunking and for a point alone.
 * GPRC_ERR_ARG, each with text: a null paths object, X_star or dout; n_star < 1; ld_dout < n_star; out given and ld_out < n_star;
 * a paths object whose context has been destroyed. */
GPRC_API int gprc_gpr_paths_eval_grad(gprc_paths* paths, const double* X_star, int64_t n_star, double* out, int64_t ld_out, double* dout,
                                      int64_t ld_dout);
GPRC_API int gprc_gpr_paths_get_weights(gprc_paths* paths, double* U_out);
GPRC_API int gprc_gpr_paths_dims(const gprc_paths* paths, int64_t* n_out, int64_t* d_out, int64_t* D_out, int64_t* S_out);
GPRC_API int gprc_gpr_paths_free(gprc_paths* paths);
/* Append m observations (X_new: d x m, y_new: m) to a fitted GPR model in place of GPR$new on
 * cbind(X, X_new), c(y, y_new) with the model's kernel, parameters and stored $noise (jitter kept, never re-tried).
 * Only the factor's columns behind the last panel boundary n0 = floor(n / 512) 512 are recomputed: the new rows of the
 * kept columns by a triangular solve with the old factor (m n0^2 flop), the trailing block by the ordinary factorisation.
 * The result is built in new buffers: peak device memory is the old model plus the extended one.  X_new, y_new may be
 * host or device pointers.
 * Returns 0; info > 0 (global 1-based column, model unchanged) when the extended matrix is not PD;
 * GPRC_ERR_ARG for m < 1, null pointers, a GPC model, or a borrowed model (gprc_gpr_model_from_device, gprc_mgpu_model_rank). */
GPRC_API int gprc_gpr_extend(gprc_model* model, const double* X_new, int64_t m, const double* y_new);
/* active bindings (R/GPRclass.R:230-280).  get_L materialises the n x n lower factor (upper = 0,
 * as t(chol(.)) has it) -- lazily, only when asked: it is 32 GiB at n = 65536. */
GPRC_API int gprc_model_dims(const gprc_model* model, int64_t* n_out, int64_t* d_out);
GPRC_API int gprc_model_get_L(gprc_model* model, double* L_out, int64_t ld_out);
GPRC_API int gprc_gpr_get_alpha(gprc_model* model, double* alpha_out);
GPRC_API int gprc_gpr_get_logp(gprc_model* model, double* logp_out);
GPRC_API int gprc_gpr_get_noise(gprc_model* model, double* noise_out);
GPRC_API int gprc_model_free(gprc_model* model);

/* ---- L2: sparse GPR with inducing points (Titsias' variational bound, collapsed; no reference counterpart) -------- *
 * X: d x n, y: n, noise = sigma^2 > 0 (the variance), Z: d x m inducing points, jitter >= 0, any kernel id.
 *   K_uu = k(Z,Z) + jitter I = L_u L_u^T            V = K(X,Z) L_u^-T  (n x m, row i = v_i^T)
 *   B    = I + V^T V / sigma^2 = L_B L_B^T          b = V^T y,   c = L_B^-1 b / sigma^2
 *   t    = sum_i ( k(x_i,x_i) - |v_i|^2 )           (the trace term, >= 0 up to rounding)
 *   elbo = -n/2 log(2 pi sigma^2) - sum_j log (L_B)_jj - y^T y / (2 sigma^2) + c^T c / 2 - t / (2 sigma^2)
 * elbo <= log p(y) (gprc_gpr_log_marginal) for every Z and jitter >= 0, with equality at Z = X, jitter = 0.  The fit is one pass
 * over the training points in row chunks (GPRC_CHUNK_BYTES as for predict, 256-row granularity), 2 n m^2 flop; MEMORY: two packed
 * m x m factors with their block inverses (2 x (gprc_packed_size + gprc_winv_size)(gprc_pad(m)) doubles, the model's) and one chunk of
 * the context's workspace -- never n x n, never X: X and y may be host or device pointers, host data is staged chunk by chunk.  The
 * model keeps Z, both factors and c, not X or y.  No jitter retry: returns info > 0 (the leading minor) when K_uu + jitter I or B is not
 * positive definite; the error text says which.  Every result -- elbo, t, c, both factors, every prediction -- is the same bit for bit
 * under every chunking: t and y^T y are summed on the host in index order in long double.  m > n is allowed.
 * GPRC_ERR_ARG: m < 1, n < 1, noise <= 0 or not finite, jitter < 0 or not finite, null pointers.
 * A sparse model answers gprc_model_dims with (m, d) and is released by gprc_model_free; gprc_gpr_predict, gprc_gpr_predict_grad,
 * gprc_gpr_loo, gprc_gpr_extend, gprc_model_get_L, the gprc_gpr_get_* getters and the GPC calls return GPRC_ERR_ARG for it, as the
 * gprc_sgpr_* calls that take a model do for a GPR or GPC model. */
GPRC_API int gprc_sgpr_fit(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n,
                           const double* y, double noise, const double* Z, int64_t m, double jitter, gprc_model** model_out);
/* The objective without keeping a model: *elbo_out and (may be NULL) *trace_out = t, the bits gprc_sgpr_fit + gprc_sgpr_get_elbo give */
GPRC_API int gprc_sgpr_elbo(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n,
                            const double* y, double noise, const double* Z, int64_t m, double jitter, double* elbo_out, double* trace_out);
/* The bound AND its exact gradient with respect to the kernel parameters, the noise and the inducing points (no reference
 * counterpart; DESIGN.md section 7, "Sparse GPR gradient").  Arguments as gprc_sgpr_elbo; kernels as gprc_gpr_logp_grad (sqrexp,
 * gammaexp, rationalquadratic, sqrexp_ard, matern32, matern52, matern32_ard, matern52_ard; any other id: GPRC_ERR_ARG).
 *   *elbo_out   the bits gprc_sgpr_elbo returns
 *   grad_out    n_params + 1 doubles, HOST: d elbo / d params[k] in the ABI's order, then d elbo / d noise (noise = sigma^2)
 *   dZ_out      d x m doubles in Z's layout, host or device, or NULL: d elbo / d Z[c, j].  With NULL the column sums are not formed
 *               (another instantiation of the contraction kernel); grad_out has the same bits either way.
 * With q = L_B^-T c, mu = L_u^-T q, r = y - V q:
 *   G_fu = [ V (I - B^-1) L_u^-1 + r mu^T ] / sigma^2,   G_uu = 1/2 L_u^-T (2 I - B^-1 - B) L_u^-1 - 1/2 mu mu^T
 *   d elbo / d theta = sum_ij G_fu,ij dk(x_i,z_j)/d theta + sum_jk G_uu,jk dk(z_j,z_k)/d theta       (the jitter is a constant)
 *   d elbo / d z_jc  = sum_i G_fu,ij dk(x_i,z_j)/d z_jc + 2 sum_k G_uu,jk dk(z_k,z_j)/d z_jc
 *   d elbo / d sigma^2 = [ -n + m - tr B^-1 - c^T c - q^T q ] / (2 sigma^2) + [ y^T y + t ] / (2 sigma^4)      (host, long double)
 * Whitened throughout: no K_uu^-1 is formed.  FLOP: the fit (2 n m^2) plus a second pass over the training points with one more
 * row solve (n m^2) and one n x m x m product (2 n m^2), about 14 m^3 for the m x m algebra, and the contraction (n m (3 d + 50), exp-bound):
 * 2.5 x the fit at n >> m.  MEMORY: the fit's, plus B once more (packed) and four m_pad^2 matrices (m_pad = gprc_pad(m)); the second
 * pass keeps V and G_fu of a chunk side by side in the context's chunk workspace, so its chunks have half the rows of the fit's --
 * never n x n, never X.  info > 0 as gprc_sgpr_fit.
 * Two calls give the same bits (no atomics; the order of summation is fixed by the chunking: K_uu's part, then the chunks in order).
 * Another chunking (GPRC_CHUNK_BYTES) sums in another order: the gradient then agrees to rounding, the bound bit for bit. */
GPRC_API int gprc_sgpr_elbo_grad(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n,
                                 const double* y, double noise, const double* Z, int64_t m, double jitter, double* elbo_out,
                                 double* grad_out, double* dZ_out);
/* At x*: v* = L_u^-1 k(Z,x*), w* = L_B^-1 v*, mean = w*^T c, var = k(x*,x*) - |v*|^2 + |w*|^2 -- the LATENT variance, without the noise,
 * as gprc_gpr_predict(pointwise = 1).  X_star: d x n_star; mean_out, var_out: n_star doubles, host or device; either may be NULL, not
 * both.  Chunked over the test points, O(m^2) flop per point, chunk-invariant bit for bit. */
GPRC_API int gprc_sgpr_predict(gprc_model* model, const double* X_star, int64_t n_star, double* mean_out, double* var_out);
GPRC_API int gprc_sgpr_get_elbo(gprc_model* model, double* elbo_out, double* trace_out /* may be NULL */);
/* c = L_B^-1 V^T y / sigma^2 (m doubles, host or device): the vector the predictive mean is a product with */
GPRC_API int gprc_sgpr_get_c(gprc_model* model, double* c_out);

/* ---- L2: iterative exact GPR (preconditioned conjugate gradients, matrix-free; no reference counterpart) ---------- *
 * The exact model without its n x n factor: every solve with K_y = K(X, X) + noise I is a conjugate-gradient loop on the generated-
 * operand product of gprc_dev_kernel_gemm, which stores no kernel value ("Iterative GPR").  Kernels: those of
 * gprc_gpr_paths_create (stationary, k(x, x) = 1); any other id: GPRC_ERR_ARG.  noise = sigma^2, finite and > 0; tol > 0.
 * MEMORY: 5 n x 64 doubles for a block of right-hand sides, the product's partials (at most 1 GiB), 2 n x rank for the preconditioner
 * (Q, and L for the probes of gprc_igpr_logp_grad), and X, y, alpha.  FLOP per iteration: one n x n generated product (n^2 (3 d + 40) + 2 n^2 S) and 4 n rank S for the preconditioner.
 * Preconditioner: precond_rank steps of the pivoted Cholesky of K (gprc_dev_pivoted_cholesky) give L (n x rank); P = L L^T + noise I is
 * applied as P^-1 V = (V - Q (Q^T V)) / noise, Q formed once per model.  precond_rank = 0: none; clipped to n; < 0 or > 1024: GPRC_ERR_ARG.
 * Loop: right-hand sides in blocks of 64 columns; a column stops when its recurrence residual has |r| <= tol |b| (tested as
 * |r|^2 <= tol^2 |b|^2) and is then frozen; a zero column returns x = 0 after 0 iterations; max_iter <= 0 selects 1000.
 * After the loop one more product gives the TRUE residual |b - K_y x| / |b| of every column: that is what is reported, the recurrence
 * drifts from it.  A column's bits are the same alone or in any batch, on every call, and from host or device pointers.
 * GPRC_ERR_MAXITER: a column did not meet tol within max_iter; gprc_igpr_solve and gprc_igpr_predict have then written every output
 * from the last iterate, gprc_igpr_fit returns no model.  GPRC_ERR_NOT_PD: p^T K_y p was not finite or not positive.
 * fit: alpha = K_y^-1 y.  The model holds X, y, alpha, Q, L, log det P and the statistics of that solve; it answers gprc_model_dims with (n, d), is
 * released by gprc_model_free and is accepted by gprc_gpr_paths_create (U is then the conjugate-gradient solve of the paths' right-hand
 * sides; no reversed factor).  Every other gprc_gpr_*, gprc_sgpr_*, gprc_gpc_* call and gprc_model_get_L return GPRC_ERR_ARG for it, as
 * the gprc_igpr_* calls do for any other model.
 * solve: Xout (n x S, pitch ldx >= n) = K_y^-1 B (n x S, pitch ldb >= n), host or device; iters_out, relres_true_out: S entries each in
 * HOST memory, or NULL.
 * predict: mean_i = sum_j k(x*_i, x_j) alpha_j through the product; var may be NULL, else var_i = 1 - k*_i^T K_y^-1 k*_i, the latent
 * variance as gprc_gpr_predict(pointwise = 1).  THE VARIANCE COSTS A FULL CONJUGATE-GRADIENT SOLVE PER 64 TEST POINTS: it is meant for
 * a modest n_star.  With var = NULL the mean has the same bits.
 * stats: of the fit's solve -- iterations, recurrence and true relative residual -- and the preconditioner's rank; each may be NULL. */
GPRC_API int gprc_igpr_fit(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n,
                           const double* y, double noise, double tol, int max_iter, int64_t precond_rank, gprc_model** model_out);
GPRC_API int gprc_igpr_solve(gprc_model* model, const double* B, int64_t ldb, int64_t S, double* Xout, int64_t ldx, int* iters_out,
                             double* relres_true_out);
GPRC_API int gprc_igpr_predict(gprc_model* model, const double* X_star, int64_t n_star, double* mean, double* var);
GPRC_API int gprc_igpr_get_alpha(gprc_model* model, double* alpha_out);
GPRC_API int gprc_igpr_stats(gprc_model* model, int* iterations_out, double* relres_recurrence_out, double* relres_true_out, int64_t* rank_out);
/* The log marginal likelihood of an iterative model and its gradient, from the conjugate-gradient loop itself (DESIGN.md section 7,
 * "Iterative GPR evidence"): stochastic Lanczos quadrature for log det K_y and a Hutchinson estimate of the trace in the gradient, both
 * DETERMINISTIC functions of caller-supplied standard normals G1 (rank x T, pitch ldg1 >= rank; rank = gprc_igpr_stats' rank_out, ignored
 * and may be NULL at rank 0) and G2 (n x T, pitch ldg2 >= n), host or device.  With P = L L^T + noise I the model's preconditioner (at
 * rank 0: P = I) and sigma = sqrt(noise):
 *   probes  z_s = L g1_s + sigma g2_s ~ N(0, P) (rank 0: z_s = g2_s);  w_s = P^-1 z_s;  u_s = K_y^-1 z_s by the model's loop, 64 columns a block
 *   q_s     = (z_s^T w_s) e_1^T log(T_s) e_1,  T_s the Lanczos tridiagonal of P^-1/2 K_y P^-1/2 from the coefficients of the column's own
 *           m = iterations steps: T[0,0] = 1 / alpha_0, T[j,j] = 1 / alpha_j + beta_{j-1} / alpha_{j-1}, T[j,j+1] = sqrt(beta_j) / alpha_j;
 *           E q_s = log det K_y - log det P, and log det P = n log noise + 2 sum log diag(C), C the factor of I + L^T L / noise (rank 0: 0)
 *   logp    = -1/2 y^T alpha - 1/2 (log det P + mean_s q_s) - n/2 log 2 pi;   se = 1/2 std(q, ddof = 1) / sqrt(T)
 *   grad_k  = sum_ij G_ij dk(x_i, x_j) / dtheta_k,  G = 1/2 alpha alpha^T - 1/(2T) sum_s u_s w_s^T, never formed (gprc_dev_lowrank_grad);
 *   d / d noise = 1/2 alpha^T alpha - 1/(2T) sum_s u_s^T w_s, last: the order of gprc_gpr_logp_grad.
 * probes: Z_out (n x T, pitch ldz >= n, host or device) = the z_s alone.
 * logp_grad: T >= 1; logp_out and grad_out (n_params + 1 doubles) on the HOST; se_out (host) may be NULL and needs T >= 2; terms_out (host,
 * T doubles: the q_s) may be NULL.  Other arguments out of range, a model that is not iterative or whose context is gone: GPRC_ERR_ARG.
 * GPRC_ERR_MAXITER as gprc_igpr_solve: every output is written, from the last iterates.  GPRC_ERR_NOT_PD as gprc_igpr_solve, and when a
 * tridiagonal has an eigenvalue <= 0.  A second call gives the same bits, host and device pointers give the same bits, and q_s does not
 * depend on which other probes are in the call.  The model is not changed.
 * MEMORY: beside the solve's, 4 n (T + 1) doubles (z, w, u and the scaled copies) and max_iter x 128 doubles of coefficients; the model
 * itself keeps L beside Q from the fit on, another n x rank doubles.  FLOP: T / 64 blocks of the solve, and the contraction below with
 * R = T + 1. */
GPRC_API int gprc_igpr_probes(gprc_model* model, const double* G1, int64_t ldg1, const double* G2, int64_t ldg2, int64_t T, double* Z_out,
                              int64_t ldz);
GPRC_API int gprc_igpr_logp_grad(gprc_model* model, const double* G1, int64_t ldg1, const double* G2, int64_t ldg2, int64_t T, double* logp_out,
                                 double* se_out, double* grad_out, double* terms_out);

/* ---- L2: GPC ------------------------------------------------------------------------------ */
/* GPC$initialize (R/GPCclass.R:66-107): Laplace mode by Newton/IRLS; y in {-1,+1}.
 * max_iter <= 0 selects 1000.  *iters_out = the "Convergence after %s iterations" count (:98).
 * flags: GPRC_GPC_REFERENCE_STOP reproduces the reference's stop rule of :90-91 verbatim
 * (`least_objective + 10 < objective` -> GPRC_ERR_DIVERGED; note it fires whenever the maximised objective
 * IMPROVES by more than 10 over iteration 1, i.e. for most problems beyond a few hundred points);
 * 0 switches that rule off and iterates to |delta objective| < epsilon. */
#define GPRC_GPC_REFERENCE_STOP 1
GPRC_API int gprc_gpc_fit(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d,
                 int64_t n, const double* y, double epsilon, int max_iter, int flags, gprc_model** model_out,
                 int* iters_out);
/* the hot part of GPC$predict_class (R/GPCclass.R:109-115): fs_bar and Vfs for X_star. */
GPRC_API int gprc_gpc_predict_latent(gprc_model* model, const double* X_star, int64_t n_star, double* fs_bar_out,
                            double* Vfs_out);
/* GPC$predict_class (R/GPCclass.R:108-118): prob_out[i] = integral of sigmoid(z) dnorm(z, fs_bar[i], sd = Vfs[i]) dz.
 * The latent stage is gprc_gpc_predict_latent(); the 1-D integrals (stats::integrate / QUADPACK in the reference,
 * rel.tol 1.2e-4) run as one batched device kernel (composite Gauss-Legendre, ~1e-14).  The reference's use of the
 * VARIANCE as dnorm's sd (:117) is reproduced.  Vfs <= 0 gives NaN. */
GPRC_API int gprc_gpc_predict_class(gprc_model* model, const double* X_star, int64_t n_star, double* prob_out);
/* the integral alone, for callers that already hold fs_bar / Vfs */
GPRC_API int gprc_class_probability(gprc_ctx* ctx, const double* fs_bar, const double* Vfs, int64_t n, double* prob_out);
GPRC_API int gprc_gpc_get_f_hat(gprc_model* model, double* f_hat_out);
GPRC_API int gprc_gpc_get_logq(gprc_model* model, double* logq_out);
/* The Laplace approximation of the log evidence, log q(y | X, theta), and its exact gradient with respect to the kernel parameters
 * (Rasmussen & Williams, Algorithm 5.1, logistic likelihood, y in {-1, +1}; no reference counterpart).  The mode f_hat is found by the
 * loop of gprc_gpc_fit with flags = 0: from f = 0 until |delta objective| < epsilon; max_iter <= 0 selects 1000, GPRC_ERR_MAXITER when
 * the cap is reached; *iters_out (may be NULL) = iterations used.  With a = K^-1 f_hat, B = I + sqrt(W) K sqrt(W) = L L^T:
 *   *logq_out = -1/2 a.f_hat + sum_i log sigmoid(y_i f_hat_i) - sum_i log L_ii
 * This is the TRUE Laplace evidence (the LOG of the factor's diagonal), NOT what gprc_gpc_get_logq returns: that reproduces the
 * reference's sum(diag(L)) (R/GPCclass.R:103) and is no objective.  For a model fitted with the same epsilon and flags = 0:
 *   *logq_out = gprc_gpc_get_logq + sum_i L_ii - sum_i log L_ii.
 * grad_out: n_params doubles in HOST memory, d log q / d params[i] in the ABI's parameter order (GPRC_SQREXP {l}; GPRC_GAMMAEXP
 * {l, gamma}; GPRC_RATQUAD {l, alpha}; GPRC_SQREXP_ARD {l_1..l_d}; GPRC_MATERN32, GPRC_MATERN52 {l}; GPRC_MATERN32_ARD,
 * GPRC_MATERN52_ARD {l_1..l_d}); explicit and implicit (through f_hat) parts together.  The
 * gradient is that of the converged mode: epsilon = 1e-10 is what the 1e-10 accuracy of the gradient needs (with GPC$new's default
 * 1e-5 the mode can be one Newton step short: 2.6e-9 at n = 3000).  X, y: host or device pointers.
 * The dense K, the factor, L^-1 and B^-1 are held whole on the device: about 3.5 * gprc_pad(n)^2 doubles (GPRC_ERR_NOMEM when that
 * does not fit; gprc_ctx_trim releases the workspace part).  Other kernel ids, null outputs, epsilon <= 0: GPRC_ERR_ARG. */
GPRC_API int gprc_gpc_logq_grad(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n,
                                const double* y, double epsilon, int max_iter, double* logq_out, double* grad_out, int* iters_out);

/* ---- device-level building blocks (multi-GPU driver, bench) ------------------------------- *
 * All pointers below are DEVICE pointers on the context's GPU.  The factor lives in the packed
 * block-column layout described in DESIGN.md: n_pad = gprc_pad(n); panel p holds rows
 * [p*NB, n_pad) x columns [p*NB, (p+1)*NB), column-major with leading dimension n_pad - p*NB, at
 * element offset gprc_panel_offset(n_pad, p); NB = gprc_panel_width().  Every panel is therefore one
 * contiguous buffer: the unit RCCL broadcasts.  winv holds one 128 x 128 block per 128 columns
 * (the inverse of the diagonal block of L), gprc_winv_size(n_pad) doubles. */
GPRC_API int64_t gprc_panel_width(void);
GPRC_API int64_t gprc_pad(int64_t n);
GPRC_API int64_t gprc_panel_count(int64_t n_pad);
GPRC_API int64_t gprc_panel_offset(int64_t n_pad, int64_t p);
GPRC_API int64_t gprc_panel_elems(int64_t n_pad, int64_t p);
GPRC_API int64_t gprc_packed_size(int64_t n_pad);
GPRC_API int64_t gprc_winv_size(int64_t n_pad);
/* fill panel p of K + noise*I (identity in the padding) */
GPRC_API int gprc_dev_fill_panel(gprc_ctx* ctx, int kernel, const double* params_host, int n_params, const double* X,
                        int64_t d, int64_t n, int64_t n_pad, double noise, double* packed, int64_t p);
/* factor panel p in place (diagonal blocks in LDS, panel solves, in-panel updates); info_dev is a
 * device int the first non-PD column (1-based) is written to (must be zeroed by the caller) */
GPRC_API int gprc_dev_factor_panel(gprc_ctx* ctx, double* packed, int64_t n_pad, int64_t p, double* winv, int* info_dev);
/* the same in steps, j = 0..3 (128 columns each, in order).  part 1 (or 0): block j's columns receive the contributions of
 * the blocks 0..j-1 of the panel (one K = 128 j pass), the diagonal block is factored + inverted and the rows below it
 * are solved -- after it the columns [128 j, 128 (j+1)) of the panel, a contiguous range of the packed buffer, are
 * final, so a multi-rank driver can start broadcasting them.  part 2: nothing (accepted so that drivers written for a
 * right-looking "factor, then update the rest of the panel" split keep working). */
GPRC_API int gprc_dev_factor_subpanel(gprc_ctx* ctx, double* packed, int64_t n_pad, int64_t p, int j, int part, double* winv,
                             int* info_dev);
/* All panels of an already filled packed matrix on ONE GPU, asynchronously on the context's stream (the one-rank form of
 * the factor_panel / update_trailing sweep: the panels in groups, a left-looking pass per group, inside the group two persistent
 * launches side by side -- the factor service (the panels' dependent chains) and the sweep kernel (every other tile and strip of the
 * group, dealt by tickets; GPRC_SWEEP=0: one launch per panel instead); one group below n_pad = 20480): results bit-identical to that sweep.
 * Below n_pad = 20480 the chain's 128^3 tiles are split in 32-row slices over four helper workgroups of the service (GPRC_CHAIN_SPLIT=0 / 1
 * forces the form); from n_pad = 13312 the service's 4-wave roles share their CUs with one sweep workgroup each (GPRC_SERVICE_SHARE=0 / 1).
 * Every combination gives the same bits.
 * info_dev: one device int, zeroed by the caller, receives LAPACK's info (first non-PD leading minor) if any.
 * inv: NULL, or gprc_solve_inv_size(n_pad) doubles that receive what gprc_dev_solve_prepare would compute for all panels. */
GPRC_API int gprc_dev_factor_all(gprc_ctx* ctx, double* packed, int64_t n_pad, double* winv, int* info_dev, double* inv);
/* The factor service (one persistent launch carrying the panel chains beside the caller's kernels) needs kernels of two streams to
 * run CONCURRENTLY.  Where they cannot -- a tool that serialises dispatches, e.g. rocprofv3 --pmc -- its device-side waits run out
 * after a few seconds and info becomes GPRC_INFO_WAIT_TIMEOUT (-99).  The fit entry points (gprc_gpr_fit*, gprc_gpc_fit, ...) then
 * switch the service off for the process, rebuild the matrix and factor again with one launch per panel; callers of
 * gprc_dev_factor_all (asynchronous: info stays on the device) do the same with this switch: on = 0 off, 1 on, -1 query;
 * returns the previous state.  (GPRC_SERVICE=0 in the environment never uses it.) */
GPRC_API int gprc_factor_service(int on);
#define GPRC_INFO_WAIT_TIMEOUT (-99)
/* trailing update of panels q = q_begin, q_begin + q_stride, ... < q_end with factored panel p */
GPRC_API int gprc_dev_update_trailing(gprc_ctx* ctx, double* packed, int64_t n_pad, int64_t p, int64_t q_begin,
                             int64_t q_end, int64_t q_stride);
/* the same for a RANGE of source panels [p_begin, p_end) in one pass (the C tiles stay in the accumulators across the
 * whole range): bit-identical to p_end - p_begin single-panel updates in order.  Targets q_begin, q_begin + q_stride,
 * ... < q_end must all lie behind the range (q_begin >= p_end). */
GPRC_API int gprc_dev_update_range(gprc_ctx* ctx, double* packed, int64_t n_pad, int64_t p_begin, int64_t p_end, int64_t q_begin,
                          int64_t q_end, int64_t q_stride);
/* The solves with VECTORS (alpha <- solve(t(L), solve(L, y)), R/GPRclass.R:152, R/GPCclass.R:82-83) work with the explicit inverse
 * of every panel's NB x NB diagonal block: inv, gprc_solve_inv_size(n_pad) doubles, panel p's inverse (transposed, ld = NB) at
 * inv + p NB NB.  gprc_dev_solve_prepare computes it for the factored panels [p_begin, p_end) from packed and winv (one launch);
 * gprc_dev_factor_all does it itself when given inv. */
GPRC_API int64_t gprc_solve_inv_size(int64_t n_pad);
GPRC_API int gprc_dev_solve_prepare(gprc_ctx* ctx, const double* packed, const double* winv, int64_t n_pad, double* inv, int64_t p_begin,
                           int64_t p_end);
/* b := L^-1 b (transpose == 0) or L^-T b (transpose != 0), one launch per panel (launch p: the product of panel p and the
 * diagonal step of the next panel); work: gprc_trsv_work_size(n_pad) doubles */
GPRC_API int64_t gprc_trsv_work_size(int64_t n_pad);
GPRC_API int gprc_dev_trsv(gprc_ctx* ctx, const double* packed, const double* inv, int64_t n_pad, double* b, int transpose,
                  double* work);
/* one panel step of that solve (forward: p = 0, 1, ...; transposed: p = P-1, ..., 0): x_p, then its contribution to the
 * rest of the right-hand side.  The forward solve needs only panels <= p, so a sweep that produces the panels in order can
 * run it beside the factorisation.  Element by element the arithmetic of gprc_dev_trsv: identical bits.  work as above (one
 * buffer for the whole sequence of steps). */
GPRC_API int gprc_dev_trsv_step(gprc_ctx* ctx, const double* packed, const double* inv, int64_t n_pad, double* b, int transpose,
                       int64_t p, double* work);
/* vt (m_pad x n_pad, leading dimension ld >= m_pad, ld even, m_pad % 128 == 0) = K(X_star, X), zero in the
 * padding.  Keep ld off powers of two (e.g. m_pad + 128): a 2^k-byte column stride aliases HBM channels. */
GPRC_API int gprc_dev_fill_cross(gprc_ctx* ctx, int kernel, const double* params_host, int n_params, const double* X_star,
                        int64_t d, int64_t m, int64_t m_pad, const double* X, int64_t n, int64_t n_pad, double* vt,
                        int64_t ld);
/* out[i] = sum_j vt[i + j*ld] * w[j]  (w == NULL: sum_j vt[i,j]^2); work: rows * gprc_rowreduce_splits(cols) */
GPRC_API int64_t gprc_rowreduce_splits(int64_t cols);
GPRC_API int gprc_dev_row_reduce(gprc_ctx* ctx, const double* vt, int64_t ld, int64_t rows, int64_t cols, const double* w,
                        double* out, double* work);
/* out_dev[0] = -0.5 y.alpha - sum(log(diag L)) - n/2 log(2 pi)  (R/GPRclass.R:153) */
GPRC_API int gprc_dev_logp(gprc_ctx* ctx, const double* packed, int64_t n_pad, int64_t n, const double* y, const double* alpha,
                  double* out_dev);
/* Wrap device buffers a driver factored itself (multi-GPU: every rank ends up with the full packed L,
 * winv and alpha) into a model handle so gprc_gpr_predict() can run on this rank's slice of X_star.
 * Nothing is copied or computed; the buffers are BORROWED and must outlive the handle.
 * y and alpha hold n_pad doubles (zero padded). */
GPRC_API int gprc_gpr_model_from_device(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X,
                               int64_t d, int64_t n, const double* y, double* packed, double* winv, double* alpha,
                               double noise, double logp, gprc_model** model_out);
/* vt := vt * L^-T  (row i becomes (L^-1 k_i)^T) */
GPRC_API int gprc_dev_solve_rows(gprc_ctx* ctx, const double* packed, const double* winv, int64_t n_pad, double* vt,
                        int64_t ld, int64_t m_pad);
/* The reversed factor: with J the reversal of n_pad indices, M = J L^T J is lower triangular (M[i, j] = L[n_pad - 1 - j, n_pad - 1 - i]) and
 * V L^-1 = ((V J) M^-T) J, so gprc_dev_solve_rows(packed_rev, winv_rev) on a column-reversed chunk is the backward solve.  packed_rev,
 * winv_rev: the sizes and layout of packed, winv; the part of M's diagonal blocks above the diagonal is written as zero; block b of
 * winv_rev = J winv_block(n_pad / 128 - 1 - b)^T J.  Pure data movement: exact.  Asynchronous, as the other gprc_dev_*. */
GPRC_API int gprc_dev_reverse_factor(gprc_ctx* ctx, const double* packed, const double* winv, int64_t n_pad, double* packed_rev,
                                     double* winv_rev);
/* C[M x N] -= A[M x K] B[N x K]^T on the 128 x 128 MFMA tile core (column-major, M, N multiples of 128, K a multiple of 32 and >= 64,
 * lda, ldb even); lower != 0: only the tiles on or below the block diagonal.  Counted under profiling kind 8.  The yardstick
 * tools/sgpr_bench.py holds gprc_dev_gram_rows against: the same tiles and flops with k along the leading dimension. */
GPRC_API int gprc_dev_gemm_nt(gprc_ctx* ctx, double* C, int64_t ldc, const double* A, int64_t lda, const double* B, int64_t ldb, int64_t M,
                              int64_t N, int64_t K, int lower);
/* The sparse GPR's two reductions over the ROWS of a solved chunk (device pointers, asynchronous).  vt: rows x n_pad (x cols),
 * column-major, leading dimension ld >= rows, ld even; rows % 256 == 0; 16-byte aligned buffers.
 * gram_rows: packed(lower) += vt^T vt straight into the packed block-column layout of an n_pad x n_pad matrix (n_pad % 512 == 0): the
 * 128 x 128 tiles on or below the block diagonal (a diagonal tile is written whole; the tiles above the diagonal inside a panel's
 * diagonal block are not touched).  col_reduce: out[j] += sum_i vt[i,j] w[i], j < cols; w: `rows` doubles.
 * Both add an element's rows in ascending order to the stored value, in groups that end at multiples of 256 rows: one call with
 * r1 + r2 rows gives the bits of two calls with r1, then r2 rows. */
GPRC_API int gprc_dev_gram_rows(gprc_ctx* ctx, const double* vt, int64_t ld, int64_t rows, int64_t n_pad, double* packed);
GPRC_API int gprc_dev_col_reduce(gprc_ctx* ctx, const double* vt, int64_t ld, int64_t rows, int64_t cols, const double* w, double* out);
/* The contraction kernel of gprc_sgpr_elbo_grad alone, on a caller-supplied matrix.  G: DEVICE, column-major with pitch ld, allocated
 * for ceil(rows / 128) * 128 rows and ceil(cols / 64) * 64 columns (what lies past rows x cols is never used), 16-byte aligned, ld even;
 * A: d x rows and Z: d x cols, DEVICE, one point per column; kernels as gprc_gpr_logp_grad.
 *   grad_out[k] = f * sum_ij G_ij dk(a_i, z_j) / d params[k]            n_params doubles, HOST
 *   dZ[c + d j] += f * sum_i G_ij dk(a_i, z_j) / d z_jc                 d x cols doubles, DEVICE, ADDED to; NULL: not formed
 * Synchronous (grad_out is complete on return).  Fixed order of summation, no atomics: the same bits on every call. */
GPRC_API int gprc_dev_cross_grad(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* G, int64_t ld, const double* A,
                                 int64_t rows, const double* Z, int64_t cols, int64_t d, double f, double* grad_out, double* dZ);
/* The two generated-operand products of the sample paths alone (DEVICE pointers, synchronous):
 *   out[i + s ld] = scale * sum_j g(a_i, b_j) B[j + s ldb],   i < rows, s < S, j < cols,   any rows, cols, S, d >= 1
 * with the left operand never stored: each element is computed from the points in the lane that feeds it to v_mfma_f64_16x16x4_f64.
 * A: d x rows, one point per column.
 * feature_gemm: g = cos 2 pi(sum_c Nu[c, j] a_i[c] + phase[j]); Nu: d x D in cycles, phase: D in turns, B = W (D x S, pitch ldw >= D).
 * kernel_gemm: g = k(a_i, b_j), Bpts: d x cols, B = U (cols x S, pitch ldu >= cols), scale 1; kernels as gprc_gpr_paths_create.
 * j is added in ascending groups of four inside stripes that depend on cols alone, the stripes in order: fixed bits, and a row's
 * result does not depend on which other rows are in the call. */
GPRC_API int gprc_dev_feature_gemm(gprc_ctx* ctx, const double* Nu, const double* phase, int64_t D, const double* A, int64_t rows, int64_t d,
                                   const double* W, int64_t ldw, int64_t S, double scale, double* out, int64_t ld);
GPRC_API int gprc_dev_kernel_gemm(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* A, int64_t rows,
                                  const double* Bpts, int64_t cols, int64_t d, const double* U, int64_t ldu, int64_t S, double* out, int64_t ld);
/* Their gradients with respect to the row points (DEVICE pointers, synchronous), arguments as above and the d-fold output:
 *   dout[i + ld (s + S c)] = d out[i + s ld] / d a_i[c],   c < d:   rows x S x d, pitch ld >= rows
 * feature_gemm_grad: -2 pi scale sum_j Nu[c, j] sin 2 pi(t_ij) B[j + s ldw];  kernel_gemm_grad: -t_c sum_j h(a_i, b_j) (a_ic - b_jc) B[j + s ldu].
 * The same stripes and order of summation per (c, s, i) as the value products. */
GPRC_API int gprc_dev_feature_gemm_grad(gprc_ctx* ctx, const double* Nu, const double* phase, int64_t D, const double* A, int64_t rows, int64_t d,
                                        const double* W, int64_t ldw, int64_t S, double scale, double* dout, int64_t ld);
GPRC_API int gprc_dev_kernel_gemm_grad(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* A, int64_t rows,
                                       const double* Bpts, int64_t cols, int64_t d, const double* U, int64_t ldu, int64_t S, double* dout, int64_t ld);
/* The low-rank-weighted contraction alone: grad_out[k] = sum_{i,j<n} (sum_{r<R} A[i + r lda] B[j + r ldb]) dk(x_i, x_j) / dtheta_k, k <
 * n_params, in O(n^2 (R + d)) flop and O(n R) memory: the weight is formed tile by tile on the f64 matrix cores and never stored.  X (d x
 * n), A and B (n x R, pitches lda, ldb >= n): host or device; grad_out: n_params doubles on the HOST; synchronous.  Kernels: those of
 * gprc_igpr_fit, ARD with d <= 256.  R > 64 runs in blocks of 64 columns that are added in order.  No atomics: the same bits on every call. */
GPRC_API int gprc_dev_lowrank_grad(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n,
                                   const double* A, int64_t lda, const double* B, int64_t ldb, int64_t R, double* grad_out);
/* The partial pivoted Cholesky of K(X, X), matrix-free (kernels as gprc_igpr_fit: k(x, x) = 1): from dg = 1, for j = 0 .. r - 1: p = the
 * lowest index among the maxima of dg over the points not yet chosen; stop when dg_p <= n 2^-52; L[p, j] = sqrt(dg_p);
 * L[i, j] = (k(x_i, x_p) - sum_{t < j} L[i, t] L[p, t]) / L[p, j] (t ascending) for every point not yet chosen, 0 for the earlier pivots;
 * dg_i = max(dg_i - L[i, j]^2, 0).  L: n x r column-major, pitch ldl >= n; piv_out: r indices; *rank_out (HOST): the steps taken.
 * From the rank on the columns of L are zero and piv_out is -1.  X, L, piv_out host or device.  1 <= r <= min(n, 1024).  n r^2 / 2
 * flop in 2 r small launches; fixed order, no atomics: two calls give the same bits.  Synchronous. */
GPRC_API int gprc_dev_pivoted_cholesky(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* X, int64_t d, int64_t n,
                                       int64_t r, double* L, int64_t ldl, int64_t* piv_out, int64_t* rank_out);

/* ---- multi-GPU from ONE process (SURVEY 8b "Threading", 8e): the form the R `.Call` boundary can use ------------ *
 * The reference's host is a single R process; it cannot be forked per GPU.  A gprc_mgpu drives G ranks -- one per
 * listed device, each with its own streams and buffers -- from the calling thread and runs the SAME sweep as the
 * one-process-per-GPU driver: panel p of the packed factor is owned by rank p mod G (1-D block-cyclic), the owner
 * factors it on a side stream beside the trailing update of the previous panel (look-ahead), every rank receives every
 * panel -- the ONE exchange step -- so L ends up replicated, alpha is solved on every rank, and the test points of a
 * predict are sliced over the ranks with no exchange.  Replaces GPR$initialize / GPR$predict (R/GPRclass.R:127-170)
 * exactly as gprc_gpr_fit / gprc_gpr_predict do, with bit-identical results.
 *   devices  n_ranks device indices.  A device may be listed SEVERAL times: "virtual ranks" that share a GPU and
 *            exchange panels by device-to-device copies -- how a one-GPU box exercises the G = 2, 3, 8 sweeps.
 *   flags    GPRC_MGPU_RCCL: the exchange is ncclBroadcast over xGMI (single-process ncclCommInitAll + group calls;
 *            distinct devices only; librccl.so.1 is resolved at run time).  0: peer copies (hipMemcpyPeerAsync).
 *            GPRC_MGPU_NO_LOOKAHEAD: factor panel p+1 only after the whole trailing update of panel p.
 * All data pointers of these calls are HOST memory (REAL(x) of the `.Call` case). */
#define GPRC_MGPU_RCCL 1
#define GPRC_MGPU_NO_LOOKAHEAD 2
/*            GPRC_MGPU_SCATTER_ALLGATHER: the large-message form of the exchange step (last row).  xGMI is
 *            point-to-point: a rooted broadcast leaves the owner G - 1 times at one link's rate each; here the owner hands
 *            piece r (1/G of the panel, 4 KiB granules) to rank r over all its links at once and every rank then collects the
 *            other pieces from their holders (RCCL: grouped ncclSend / ncclRecv; otherwise event-ordered pull copies).  Panels
 *            below 1 MiB and the 512 KiB of inverses still travel as one rooted broadcast.  Pure data movement: same bits.
 *            GPRC_MGPU_AUTO_EXCHANGE: gprc_mgpu_create runs gprc_mgpu_calibrate and keeps the faster form. */
#define GPRC_MGPU_SCATTER_ALLGATHER 4
#define GPRC_MGPU_AUTO_EXCHANGE 8
typedef struct gprc_mgpu gprc_mgpu;
typedef struct gprc_mgpu_model gprc_mgpu_model;
GPRC_API int gprc_mgpu_create(const int* devices, int n_ranks, int flags, gprc_mgpu** mgpu_out);
GPRC_API int gprc_mgpu_destroy(gprc_mgpu* mgpu);
GPRC_API int gprc_mgpu_ranks(const gprc_mgpu* mgpu, int* n_ranks_out);
/* Start-up calibration of the exchange step: both forms move a `doubles`-sized buffer from a rotating root to every rank
 * `reps` times (after one warm-up), must deliver identical data, and scatter + all-gather is adopted when it is at least 10 %
 * faster.  choice_out (may be NULL): 0 rooted broadcast, 1 scatter + all-gather; ms_out (may be NULL): the two times. */
GPRC_API int gprc_mgpu_calibrate(gprc_mgpu* mgpu, int64_t doubles, int reps, int* choice_out, double* ms_out);
/* 0 peer copies / rooted, 1 RCCL broadcast, 2 peer copies scatter + all-gather, 3 RCCL scatter + all-gather */
GPRC_API int gprc_mgpu_exchange_mode(const gprc_mgpu* mgpu, int* mode_out);
/* What the last fit (and the last predict) on this gprc_mgpu did -- a schedule-rehearsal record, not a benchmark.  out[0..n):
 * [0] ranks G, [1] panels P, [2] exchange mode, [3] exchange operations issued, [4] bytes received per rank, [5] event record /
 * wait pairs, [6] far-update passes, [7] look-ahead updates, [8] fit wall ms, [9] predict wall ms, then per rank r
 * [10 + 3r] fill + sweep ms, [11 + 3r] alpha / logp ms (HIP events on the rank's main stream), [12 + 3r] predict ms of its slice. */
GPRC_API int gprc_mgpu_stats(const gprc_mgpu* mgpu, double* out, int n);
/* GPR$initialize, one Cholesky attempt (as gprc_gpr_fit) / the ten-step jitter loop (as gprc_gpr_fit_retry) */
GPRC_API int gprc_mgpu_gpr_fit(gprc_mgpu* mgpu, int kernel, const double* params, int n_params, const double* X, int64_t d,
                      int64_t n, const double* y, double noise, gprc_mgpu_model** model_out);
GPRC_API int gprc_mgpu_gpr_fit_retry(gprc_mgpu* mgpu, int kernel, const double* params, int n_params, const double* X, int64_t d,
                            int64_t n, const double* y, double noise, gprc_mgpu_model** model_out, double* noise_used,
                            int* attempts);
/* GPR$predict(X_star, pointwise_var = TRUE): rank r predicts the r-th contiguous slice of the test points */
GPRC_API int gprc_mgpu_gpr_predict(gprc_mgpu_model* model, const double* X_star, int64_t n_star, double* mean_out,
                          double* var_out);
GPRC_API int gprc_mgpu_gpr_get_alpha(gprc_mgpu_model* model, double* alpha_out);
GPRC_API int gprc_mgpu_gpr_get_logp(gprc_mgpu_model* model, double* logp_out);
GPRC_API int gprc_mgpu_gpr_get_noise(gprc_mgpu_model* model, double* noise_out);
/* rank r's replica as an ordinary (borrowed) model handle: gprc_gpr_predict(pointwise = 0), gprc_model_get_L, ...
 * It belongs to the gprc_mgpu_model and dies with it.
 * Lifetime: a gprc_mgpu_model may be freed after its gprc_mgpu was destroyed (garbage collectors finalise in any order); its
 * predict then fails with GPRC_ERR_ARG instead of touching the destroyed ranks. */
GPRC_API int gprc_mgpu_model_rank(gprc_mgpu_model* model, int rank, gprc_model** model_out);
GPRC_API int gprc_mgpu_model_free(gprc_mgpu_model* model);

/* ---- sampling: multivariate_normal(n, mean, covariance, tol = 1e-6)  (R/GPRclass.R:360-370) --------------------------
 * L = t(chol(covariance)); if the Cholesky fails (the usual case for a posterior covariance K(X*,X*) - t(v) %*% v,
 * which is numerically rank deficient) L = eigen$vectors %*% diag(sqrt(pmax(eigen$values, 0))) after
 * stopifnot(all(eigen$values > -tol * abs(eigen$values[1]))) -> GPRC_ERR_NOT_PD.  The standard normal matrix Z
 * (m x n_draws, column-major) comes from the caller: R draws it with rnorm on the host and so does the binding, so
 * the generator stays the caller's.  out = drop(mean) + L %*% Z, m x n_draws.  *method_out: 1 Cholesky, 2 eigen.
 * Eigenvectors are defined up to sign (and basis within repeated eigenvalues); with the eigen branch the draws for a
 * given Z therefore differ between LAPACK builds, this library and R, while L %*% t(L) -- the distribution -- agrees. */
GPRC_API int gprc_mvn_factor(gprc_ctx* ctx, const double* cov, int64_t ld, int64_t m, double tol, double* L_out, int* method_out);
GPRC_API int gprc_mvn_sample(gprc_ctx* ctx, const double* cov, int64_t ld, int64_t m, const double* mean, double tol, const double* Z,
                    int64_t n_draws, double* out, int* method_out);
/* eigen(A, symmetric = TRUE): eigenvalues in decreasing order and orthonormal eigenvectors (columns, m x m, may be
 * NULL); only the lower triangle of A is read (LAPACK dsyevr 'L', as R calls it).  Cyclic two-sided Jacobi with a
 * round-robin pair order on the device, m <= 16384; *sweeps_out = sweeps used (at most 40).
 * Range: the sweeps run on 2^-e A, 2^e <= max|A| < 2^(e+1), and the values are scaled back, so any finite A is accepted and
 * 2^s A returns the vectors of A bit for bit and 2^s times its values, as long as those stay between 2^-1022 and 2^1024 in
 * magnitude: a value beyond the double range comes back as +-Inf, one below 2^-1022 loses its low bits, and entries below
 * 2^-1022 max|A| are read as less than they are.  A NaN or Inf in the lower triangle is GPRC_ERR_ARG. */
GPRC_API int gprc_sym_eigen(gprc_ctx* ctx, const double* A, int64_t lda, int64_t m, double* values_out, double* vectors_out,
                   int* sweeps_out);

/* combine_all(lst) (R/simulation.R:338-349), the test grid of the simulate_* harness (:101-102, :223-224): all
 * combinations of the axis values, one point per column (d x prod(lengths), column-major), the LAST axis varying
 * fastest.  axis_values: the axes concatenated (sum(lengths) doubles); lengths: d host integers; d <= 64. */
GPRC_API int gprc_combine_all(gprc_ctx* ctx, const double* axis_values, const int64_t* lengths, int d, double* out);
/* ---- measurement: per-kernel-kind HIP-event timing (bench.py's live roofline numbers) ------------ *
 * When enabled, every launch is bracketed by two hipEvents on the stream it is launched on.  Kinds:
 * 0 fill, 1 potf2_inv, 2 trsm_panel, 3 in-panel GEMM (K=128), 4 trailing update, 5 predict right
 * update (K=512), 6 trsv, 7 row reductions, 8 covariance SYRK, 9 derivative row sums, 10 Jacobi sweep, 11 predict
 * left-looking update, 12 trailing left-looking update, 13 fused panel factorisation, 14 fused in-panel solve of the predict, 15 inverse GEMM
 * (-L^-T L^-1, lower), 16 gradient contraction (gprc_gpr_logp_grad), 17 Laplace gradient contraction (gprc_gpc_logq_grad),
 * 18 factor reversal, 19 prediction-gradient contraction (gprc_gpr_predict_grad; the sample paths'
 * generated-operand products and their gradient products are counted here too).  gprc_gpr_loo_grad adds no kind: its n^3 product is
 * counted under 8, its contraction under 17 and the builder of its scaled full inverse under 18.  flops/bytes are the ALGORITHMIC
 * figures of DESIGN.md for the launches seen, not counter readings. */
GPRC_API int gprc_prof_enable(int on);
/* With the environment variable GPRC_PANEL_TRACE=<p> set, the factor role of the fused panel kernel of panel p leaves
 * s_memrealtime stamps (100 MHz ticks) of its stages: [0] start, then per 128-column sub-step j: [1+6j] diagonal block
 * factored, [2+6j] W_j published, [3+6j] E_{j+1} seen, [4+6j] L(j+1,j) solved, [5+6j] R_{j+1} published, [6+6j] block
 * (j+1,j+1) updated.  side != 0: the context's look-ahead stream's launches.  Measurement only. */
GPRC_API int gprc_prof_panel_trace(gprc_ctx* ctx, int side, int64_t* ticks_out, int n);
/* With GPRC_SERVICE_TRACE set, a factor-service sweep (gprc_dev_factor_all and every fit at n <= 24576) leaves 16 stamps per panel
 * p (100 MHz ticks; 0 = not reached): [14] factor role arrives, [0] its diagonal block is complete: chain starts, [1] chain done;
 * [2]/[3] look-ahead strips start / done; [4] next-diagonal-block tiles may start, [5] their last k-chunk starts, [6] block
 * complete; [7]/[8] first ordinary-strip workgroup starts / ends; trailing update: [9] first tile starts, [10] sees the
 * look-ahead rows, [11] has published, [12] first tile of the block after the next published, [13] last tile done.
 * panels <= 48.  Measurement only. */
GPRC_API int gprc_prof_service_trace(gprc_ctx* ctx, int64_t* ticks_out, int panels);
/* When a factorisation ends in a device-side wait timeout (info = -99: the factor service's persistent launch and the caller's kernels did
 * not run concurrently, or a dependency never arrived), every wait that was unsatisfied at that moment has left a record: out[0] = records
 * written, then 8 ints per record from out[8] on -- site (1 flag, 2 count, 3 field, 4 chain helper, 5 sweep kernel, 6 residency gate; +10: the
 * wait was a bystander that left because somebody else's bound had run out), workgroup, grid size, value needed, value seen, index of the
 * awaited word inside its panel's flags, threads per workgroup, low 32 bits of those flags' address.  ints: capacity of out (at most
 * 8 * 49 are written).  Reading clears the records.  The fit entry points put the same records, as text, into gprc_last_error.  Diagnostics only. */
GPRC_API int gprc_prof_wait_timeout(int* out, int ints);
GPRC_API int gprc_prof_reset(void);
GPRC_API int gprc_prof_kinds(void);
GPRC_API int gprc_prof_summary(int kind, int64_t* count_out, double* ms_out, double* flops_out, double* bytes_out);

#ifdef __cplusplus
}
#endif
#endif /* GPRC_NATIVE_H */
