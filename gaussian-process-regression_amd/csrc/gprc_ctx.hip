// gprc_ctx.hip -- errors, the event profiler, context lifetime, the block pool, the workspace slots, argument staging and the entry
// points that are nothing but staging around one launcher (kernel matrices, class probabilities, combine_all).
//
// Host side of the hot path (reference R/GPRclass.R:127-170, R/GPCclass.R:66-115): owns device
// memory through opaque handles, stages host arrays when the caller hands over host pointers (the
// `.Call` case) and uses device pointers in place (the resident-data case).  No CPU arithmetic on
// matrices happens here: without a gfx950 device every entry point fails with GPRC_ERR_NO_DEVICE /
// GPRC_ERR_HIP.
#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <new>

#include "gprc_host.h"

namespace gprc {

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }

int hip_fail(hipError_t e, const char* what, const char* file, int line) {
  g_last_error = std::string("HIP error '") + hipGetErrorString(e) + "' in " + what + " at " + file + ":" + std::to_string(line);
  (void)hipGetLastError();
  return e == hipErrorOutOfMemory ? GPRC_ERR_NOMEM : GPRC_ERR_HIP;
}

// ---- event profiler ------------------------------------------------------------------------------
namespace {
struct ProfRec { int kind; double flops, bytes; hipEvent_t e0, e1; };
bool g_prof_on = false;
std::vector<ProfRec> g_prof_recs;
std::vector<hipEvent_t> g_prof_pool;
std::vector<ProfRec> g_prof_open;  // begun, not ended (per kind nesting is not used)
hipEvent_t prof_event() {
  if (!g_prof_pool.empty()) { hipEvent_t e = g_prof_pool.back(); g_prof_pool.pop_back(); return e; }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}
}  // namespace
std::mutex g_prof_mu;  // gprc_mgpu_gpr_predict runs one host thread per rank
bool prof_enabled() { return g_prof_on; }
void prof_begin(hipStream_t s, int kind) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  ProfRec r{kind, 0.0, 0.0, prof_event(), nullptr};
  (void)hipEventRecord(r.e0, s);
  g_prof_open.push_back(r);
}
void prof_end(hipStream_t s, int kind, double flops, double bytes) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (size_t i = g_prof_open.size(); i-- > 0;) {
    if (g_prof_open[i].kind != kind) continue;
    ProfRec r = g_prof_open[i];
    g_prof_open.erase(g_prof_open.begin() + (long)i);
    r.flops = flops; r.bytes = bytes; r.e1 = prof_event();
    (void)hipEventRecord(r.e1, s);
    g_prof_recs.push_back(r);
    return;
  }
}

namespace {

thread_local gprc_ctx* g_cur_ctx = nullptr;  // set by use_device(): whose pool the scoped temporaries use

// Contexts that exist.  A model may outlive its context (a host language's garbage collector finalising objects in arbitrary order
// at exit: Python does): gprc_model_free then must not touch the context's stream or block pool.
std::mutex g_live_mu;
std::vector<const gprc_ctx*> g_live_ctx;
uint64_t g_next_ctx_id = 1;
void ctx_register(gprc_ctx* c) { std::lock_guard<std::mutex> lk(g_live_mu); c->id = g_next_ctx_id++; g_live_ctx.push_back(c); }
void ctx_unregister(const gprc_ctx* c) {
  std::lock_guard<std::mutex> lk(g_live_mu);
  g_live_ctx.erase(std::remove(g_live_ctx.begin(), g_live_ctx.end(), c), g_live_ctx.end());
}

}  // namespace

bool ctx_alive(const gprc_ctx* c, uint64_t id) {
  std::lock_guard<std::mutex> lk(g_live_mu);
  return std::find(g_live_ctx.begin(), g_live_ctx.end(), c) != g_live_ctx.end() && c->id == id;
}

int use_device(const gprc_ctx* ctx) {
  if (!ctx) { set_error("null context"); return GPRC_ERR_ARG; }
  GPRC_HIP(hipSetDevice(ctx->device));
  g_cur_ctx = const_cast<gprc_ctx*>(ctx);
  return 0;
}

int use_device_unless(const gprc_ctx* ctx, bool bad, const char* msg) {
  GPRC_TRY(use_device(ctx));
  if (bad) { set_error(msg); return GPRC_ERR_ARG; }
  return 0;
}

int pool_alloc(gprc_ctx* ctx, size_t bytes, void** out) {
  if (bytes == 0) bytes = 8;
  if (ctx) {
    for (size_t i = ctx->pool.size(); i-- > 0;)
      if (ctx->pool[i].bytes == bytes) {
        *out = ctx->pool[i].p;
        ctx->pool_bytes -= bytes;
        ctx->pool.erase(ctx->pool.begin() + (long)i);
        return 0;
      }
  }
  hipError_t e = hipMalloc(out, bytes);
  if (e != hipSuccess && ctx && !ctx->pool.empty()) {  // give the cached blocks back and retry once
    (void)hipGetLastError();
    pool_trim(ctx);
    e = hipMalloc(out, bytes);
  }
  if (e != hipSuccess) return hip_fail(e, "hipMalloc", __FILE__, __LINE__);
  return 0;
}
void pool_release(gprc_ctx* ctx, void* p, size_t bytes) {
  if (!p) return;
  if (bytes == 0) bytes = 8;
  if (!ctx || bytes > ctx->pool_cap) { (void)hipFree(p); return; }
  while (!ctx->pool.empty() && ctx->pool_bytes + bytes > ctx->pool_cap) {  // evict the oldest
    (void)hipFree(ctx->pool.front().p);
    ctx->pool_bytes -= ctx->pool.front().bytes;
    ctx->pool.erase(ctx->pool.begin());
  }
  ctx->pool.push_back({p, bytes});
  ctx->pool_bytes += bytes;
}
void pool_trim(gprc_ctx* ctx) {
  for (auto& b : ctx->pool) (void)hipFree(b.p);
  ctx->pool.clear();
  ctx->pool_bytes = 0;
}

bool is_device_ptr(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t attr;
  hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess) { (void)hipGetLastError(); return false; }
  return attr.type == hipMemoryTypeDevice;
}

int ws_get(gprc_ctx* ctx, int slot, int64_t count, double** out) {
  if (count <= 0) count = 1;
  if (ctx->ws_cap[slot] < count) {
    if (ctx->ws[slot]) {
      GPRC_HIP(hipStreamSynchronize(ctx->stream));
      GPRC_HIP(hipFree(ctx->ws[slot]));
      ctx->ws[slot] = nullptr;
      ctx->ws_cap[slot] = 0;
    }
    hipError_t e = hipMalloc(&ctx->ws[slot], sizeof(double) * (size_t)count);
    if (e != hipSuccess) { ctx->ws[slot] = nullptr; return hip_fail(e, "hipMalloc(workspace)", __FILE__, __LINE__); }
    ctx->ws_cap[slot] = count;
  }
  *out = ctx->ws[slot];
  return 0;
}

int DevMem::alloc(int64_t count) {
  if (count <= 0) count = 1;
  owner = {g_cur_ctx, g_cur_ctx ? g_cur_ctx->id : 0};
  bytes = sizeof(double) * (size_t)count;
  return pool_alloc(owner.ctx, bytes, (void**)&p);
}

int DevMem::copy_from(hipStream_t s, const double* src, int64_t count) {
  GPRC_TRY(alloc(count));
  GPRC_HIP(hipMemcpyAsync(p, src, sizeof(double) * (size_t)count, hipMemcpyDefault, s));
  return 0;
}

}  // namespace gprc

using namespace gprc;

extern "C" {

const char* gprc_last_error(void) { return g_last_error.c_str(); }

int gprc_ctx_create(int device, void* stream, gprc_ctx** ctx_out) {
  if (!ctx_out) { set_error("null argument"); return GPRC_ERR_ARG; }
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess || c <= 0) {
    (void)hipGetLastError();
    set_error("no HIP device visible: the gprc native path needs an MI355X (gfx950); there is no CPU fallback");
    return GPRC_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= c) { set_error("device index out of range"); return GPRC_ERR_ARG; }
  GPRC_HIP(hipSetDevice(device));
  gprc_ctx* ctx = new (std::nothrow) gprc_ctx();
  if (!ctx) { set_error("out of host memory"); return GPRC_ERR_NOMEM; }
  ctx->device = device;
  if (stream) { ctx->stream = (hipStream_t)stream; ctx->own_stream = false; }
  else {
    hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete ctx; return hip_fail(e, "hipStreamCreate", __FILE__, __LINE__); }
    ctx->own_stream = true;
  }
  hipError_t e = hipMalloc(&ctx->info_dev, 64);
  if (e == hipSuccess) e = hipMalloc(&ctx->scal_dev, 64);
  if (e == hipSuccess) e = hipMalloc(&ctx->sync_dev, 512);
  if (e == hipSuccess) e = hipMemset(ctx->sync_dev, 0, 512);
  if (e != hipSuccess) { gprc_ctx_destroy(ctx); return hip_fail(e, "hipMalloc(ctx)", __FILE__, __LINE__); }
  if (const char* vp = std::getenv("GPRC_VT_PAD")) {
    const long long v = std::atoll(vp);
    if (v >= 0 && v % 2 == 0) ctx->vt_pad = v;
  }
  if (const char* pb = std::getenv("GPRC_POOL_BYTES")) {
    const long long v = std::atoll(pb);
    if (v >= 0) ctx->pool_cap = (size_t)v;
  }
  if (const char* cb = std::getenv("GPRC_CHUNK_BYTES")) {
    const long long v = std::atoll(cb);
    if (v > 0) ctx->chunk_bytes = (size_t)v;
  }
  ctx_register(ctx);
  *ctx_out = ctx;
  return 0;
}

int gprc_ctx_destroy(gprc_ctx* ctx) {
  if (!ctx) return 0;
  ctx_unregister(ctx);
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  for (int i = 0; i < 4; ++i)
    if (ctx->ws[i]) (void)hipFree(ctx->ws[i]);
  pool_trim(ctx);
  if (g_cur_ctx == ctx) g_cur_ctx = nullptr;
  if (ctx->info_dev) (void)hipFree(ctx->info_dev);
  if (ctx->scal_dev) (void)hipFree(ctx->scal_dev);
  if (ctx->sync_dev) (void)hipFree(ctx->sync_dev);
  if (ctx->svc_trace) (void)hipFree(ctx->svc_trace);
  if (ctx->side_stream) { (void)hipStreamSynchronize(ctx->side_stream); (void)hipStreamDestroy(ctx->side_stream); }
  if (ctx->side_stream2) { (void)hipStreamSynchronize(ctx->side_stream2); (void)hipStreamDestroy(ctx->side_stream2); }
  for (hipEvent_t ev : ctx->ev_pool)
    if (ev) (void)hipEventDestroy(ev);
  if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return 0;
}

int gprc_ctx_trim(gprc_ctx* ctx) {
  GPRC_TRY(gprc_ctx_synchronize(ctx));
  pool_trim(ctx);
  for (int i = 0; i < 4; ++i)
    if (ctx->ws[i]) { (void)hipFree(ctx->ws[i]); ctx->ws[i] = nullptr; ctx->ws_cap[i] = 0; }
  return 0;
}
int gprc_ctx_synchronize(gprc_ctx* ctx) {
  GPRC_TRY(use_device(ctx));
  GPRC_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int gprc_prof_enable(int on) {
  g_prof_on = on != 0;
  return 0;
}
int gprc_prof_reset(void) {
  for (auto& r : g_prof_recs) { g_prof_pool.push_back(r.e0); g_prof_pool.push_back(r.e1); }
  g_prof_recs.clear();
  return 0;
}
int gprc_prof_kinds(void) { return PK_COUNT; }
int gprc_prof_summary(int kind, int64_t* count_out, double* ms_out, double* flops_out, double* bytes_out) {
  if (kind < 0 || kind >= PK_COUNT) { set_error("prof_summary: bad kind"); return GPRC_ERR_ARG; }
  int64_t cnt = 0;
  double ms = 0.0, fl = 0.0, by = 0.0;
  for (auto& r : g_prof_recs) {
    if (r.kind != kind) continue;
    GPRC_HIP(hipEventSynchronize(r.e1));
    float t = 0.f;
    GPRC_HIP(hipEventElapsedTime(&t, r.e0, r.e1));
    ms += t; fl += r.flops; by += r.bytes; ++cnt;
  }
  if (count_out) *count_out = cnt;
  if (ms_out) *ms_out = ms;
  if (flops_out) *flops_out = fl;
  if (bytes_out) *bytes_out = by;
  return 0;
}

// ---- entry points that are one launcher behind argument checks and staging ----------------------------
int gprc_abi_version(void) { return GPRC_ABI_VERSION; }

int gprc_device_count(int* count_out) {
  if (!count_out) { set_error("null argument"); return GPRC_ERR_ARG; }
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) { (void)hipGetLastError(); c = 0; }
  *count_out = c;
  return 0;
}

int gprc_kernel_matrix(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* A, int64_t d,
                       int64_t nA, const double* B, int64_t nB, double* out, int64_t ld_out) {
  GPRC_TRY(use_device_unless(ctx, d < 1 || nA < 0 || nB < 0 || ld_out < nA, "kernel_matrix: bad dimensions"));
  if (nA == 0 || nB == 0) return 0;
  KernelSpec ks;
  GPRC_TRY(make_spec(kernel, params, n_params, d, &ks));
  hipStream_t s = ctx->stream;
  In a, b;
  GPRC_TRY(a.set(s, A, d * nA));
  GPRC_TRY(b.set(s, B, d * nB));
  Out o;   // host output: rows nA..ld_out-1 of the caller's array are never touched
  GPRC_TRY(o.set(out, ld_out, nA, nB));
  for (int64_t c0 = 0; c0 < nB; c0 += 1 << 20) {  // grid.y limit
    const int64_t nc = (nB - c0 < (1 << 20)) ? nB - c0 : (1 << 20);
    GPRC_TRY(launch_fill(s, ks, a.dev, nA, b.dev, nB, d, o.dev + c0 * o.ld, o.ld, 0, nA, c0, nc, PAD_NONE, 0.0));
  }
  return finish_sync(s, o);
}

int gprc_kernel_colwise(gprc_ctx* ctx, int kernel, const double* params, int n_params, const double* x,
                        const double* y, int64_t d, int64_t m, double* out) {
  GPRC_TRY(use_device_unless(ctx, d < 1 || m < 0, "kernel_colwise: bad dimensions"));
  if (m == 0) return 0;
  KernelSpec ks;
  GPRC_TRY(make_spec(kernel, params, n_params, d, &ks));
  hipStream_t s = ctx->stream;
  In a, b;
  Out o;
  GPRC_TRY(a.set(s, x, d * m));
  GPRC_TRY(b.set(s, y, d * m));
  GPRC_TRY(o.set(out, m));
  GPRC_TRY(launch_colwise(s, ks, a.dev, b.dev, d, m, o.dev));
  return finish_sync(s, o);
}

int gprc_class_probability(gprc_ctx* ctx, const double* fs_bar, const double* Vfs, int64_t n, double* prob_out) {
  GPRC_TRY(use_device_unless(ctx, n < 0 || (n > 0 && (!fs_bar || !Vfs || !prob_out)), "class_probability: bad arguments"));
  if (n == 0) return 0;
  hipStream_t s = ctx->stream;
  In a, b;
  Out o;
  GPRC_TRY(a.set(s, fs_bar, n));
  GPRC_TRY(b.set(s, Vfs, n));
  GPRC_TRY(o.set(prob_out, n));
  GPRC_TRY(launch_gpc_class_prob(s, a.dev, b.dev, o.dev, n));
  return finish_sync(s, o);
}

// combine_all(lst)  --  R/simulation.R:338-349 (the test grid of the simulate_* harness, :101-102)
int gprc_combine_all(gprc_ctx* ctx, const double* axis_values, const int64_t* lengths, int d, double* out) {
  GPRC_TRY(use_device_unless(ctx, !axis_values || !lengths || !out || d < 1 || d > 64, "combine_all: bad arguments"));
  int64_t sum = 0, total = 1;
  for (int k = 0; k < d; ++k) {
    if (lengths[k] < 1) { set_error("combine_all: every axis needs at least one value"); return GPRC_ERR_ARG; }
    sum += lengths[k];
    if (total > ((int64_t)1 << 40) / lengths[k]) { set_error("combine_all: grid too large"); return GPRC_ERR_ARG; }
    total *= lengths[k];
  }
  hipStream_t s = ctx->stream;
  In v;
  Out o;
  GPRC_TRY(v.set(s, axis_values, sum));
  GPRC_TRY(o.set(out, total * d));
  GPRC_TRY(launch_combine_all(s, v.dev, lengths, d, o.dev));
  return finish_sync(s, o);
}

}  // extern "C"
