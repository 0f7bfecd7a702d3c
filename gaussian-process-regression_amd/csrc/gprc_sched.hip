// gprc_sched.hip -- the host-side schedules: which launchers run in which order for a factorisation (factor_subpanel .. factor_all)
// and a triangular solve of many rows (solve_rows), and how a pass over test points is chunked (chunk_workspace).  Every schedule
// knob of the host layer (GPRC_FACTOR, GPRC_SOLVE, GPRC_PANEL, GPRC_SERVICE, GPRC_SWEEP, GPRC_SOLVE_PANEL, GPRC_SERVICE_TRACE,
// GPRC_FITGRAD_DENSE, GPRC_IGNORE_MEMINFO) and of the factor's launchers (GPRC_CHAIN_SPLIT, GPRC_SERVICE_SHARE, GPRC_SWEEP_WGS,
// GPRC_HEAD_SLICES, GPRC_PANEL_TRACE, GPRC_POTF2_TRACE, GPRC_TEST_SERVICE_TIMEOUT: kernels_chol.hip takes what they decide as launch
// parameters) is read in this file and nowhere else.  Its C entry points: the layout helpers and the
// gprc_dev_* building blocks (the schedules themselves and the single launchers a caller composes with them), the two trace read-backs.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "gprc_host.h"

namespace gprc {

// GPRC_PANEL=steps: the launch-per-stage panel kernels instead of the fused one (and no factor service)
static bool panel_steps() {
  static const bool steps = [] { const char* e = std::getenv("GPRC_PANEL"); return e && std::strcmp(e, "steps") == 0; }();
  return steps;
}

// ---- factorisation of all panels of a packed matrix (single GPU) ------------------------------
// 128-column sub-step j of panel p, left-looking inside the panel: first the columns of block j receive the
// contributions of the blocks 0..j-1 of the same panel in one pass (K = 128 j, C tile in the accumulators: the same
// products in the same order as three K = 128 updates from the left, with half the C traffic and a third of the
// launches), then the diagonal block is factored + inverted and the rows below it are solved.  After it the columns
// [128 j, 128 (j+1)) of the panel are final (what the pipelined broadcast relies on).
// part: 1 = the whole sub-step, 2 = nothing (kept so that callers written for the right-looking form still work), 0 = 1.
int factor_subpanel(gprc_ctx* ctx, double* packed, int64_t n_pad, int64_t p, int j, int part, double* winv, int* info_dev) {
  if (part == 2) return 0;
  hipStream_t s = ctx->stream;
  const int64_t ld = panel_ld(n_pad, p);
  double* pan = packed + panel_offset(n_pad, p);
  const int64_t cj = (int64_t)j * NBI;
  double* wblk = winv + (p * (NB / NBI) + j) * NBI * NBI;
  if (cj > 0)  // rows cj.. of block j's columns -= (rows cj.. of the earlier columns) * (rows cj..cj+127 of the earlier columns)^T
    GPRC_TRY(launch_gemm_nt(s, pan + cj + cj * ld, ld, pan + cj, ld, pan + cj, ld, ld - cj, NBI, cj, 1, PK_GEMM_INNER));
  GPRC_TRY(launch_potf2_inv(s, pan + cj + cj * ld, ld, wblk, info_dev, (int)(p * NB + cj)));
  const int64_t below = ld - cj - NBI;
  if (below > 0) GPRC_TRY(launch_trsm_panel(s, pan + (cj + NBI) + cj * ld, ld, below, wblk));
  return 0;
}

// The whole panel: ONE launch (panel_fused_kernel: the four sub-steps overlap across row strips, dependencies carried by
// device-side flags), bit-identical to the twelve launches of the sub-step form.  GPRC_PANEL=steps selects the latter.
// GPRC_PANEL_TRACE=<p>: the factor role of panel p stamps its stages (read back with gprc_prof_panel_trace); with GPRC_POTF2_TRACE the
// stamps are those of the SECOND diagonal block's potf2 instead.  Measurement only.
int factor_panel(gprc_ctx* ctx, double* packed, int64_t n_pad, int64_t p, double* winv, int* info_dev) {
  static const long long trace_p = [] { const char* e = std::getenv("GPRC_PANEL_TRACE"); return e ? std::atoll(e) : -1LL; }();
  static const int trace_mode = std::getenv("GPRC_POTF2_TRACE") != nullptr ? 2 : 1;
  if (!panel_steps()) return launch_panel_fused(ctx->stream, packed, n_pad, p, winv, info_dev, ctx->sync_dev, trace_p == p ? trace_mode : 0);
  for (int j = 0; j < NB / NBI; ++j) GPRC_TRY(factor_subpanel(ctx, packed, n_pad, p, j, 0, winv, info_dev));
  return 0;
}

// `to` waits for everything enqueued on `from` so far (events recycled round-robin: a wait captures the record made here)
static int stream_after(gprc_ctx* ctx, hipStream_t to, hipStream_t from) {
  hipEvent_t& ev = ctx->ev_pool[ctx->ev_next++ % 8];
  if (!ev) GPRC_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  GPRC_HIP(hipEventRecord(ev, from));
  GPRC_HIP(hipStreamWaitEvent(to, ev, 0));
  return 0;
}

// Set when a factorisation under the factor service ended in a device-side wait timeout: the persistent launch and the caller's
// kernels did not run concurrently (a tool that serialises dispatches, e.g. rocprofv3 --pmc).  From then on this process factors with
// one fused launch per panel (what GPRC_SERVICE=0 selects).
std::atomic<bool> g_service_off{false};

// Lower tiles a group of the left-looking schedule should have at least (see factor_all_async)
static int64_t want_for(int64_t n_pad) {
  // below n_pad = 20480 one group -- the plain right-looking sweep under the factor service -- is fastest (measured,
  // profiles/r02_factor_schedules.txt: n = 16384 30.0 ms against 29.2..32.8 with groups of 1000..6000 tiles); from there on 8192
  return n_pad < 20480 ? INT64_MAX : 8192;
}

static bool service_carries_inverse(int64_t n_pad) {
  return n_pad < 20480;   // measured (profiles/r03_experiments.txt): no difference up to 20480 (+0.5 % there without)
}

// The split chain (four more resident CUs) where the panel chain weighs: below n_pad = 20480, i.e. wherever the whole matrix is ONE group
// of the service (measured, same box, profiles/r03_chain_split.txt; in the grouped schedule beyond it makes no difference and the four
// CUs stay with the update).  GPRC_CHAIN_SPLIT=0 / 1 forces it off / on at every size.
static bool chain_split(int64_t n_pad) {
  static const int v = [] { const char* e = std::getenv("GPRC_CHAIN_SPLIT"); return e ? std::atoi(e) : -1; }();
  return v >= 0 ? v != 0 : n_pad < 20480;
}

// The SHARED service.  A service workgroup asks for the factor role's 149 KB of LDS, so nothing else fits on its CU -- 21 to 25 CUs
// that, where the update is the bound, mostly sleep on their flags.  From n_pad = 13312 on, the 4-wave roles (all but the factor role and
// the chain helpers, whose 8 waves x 256 VGPRs fill a CU) are launched on their own, on a second side stream, with a GEMM team's LDS only
// (launch_panel_service, part 2): ONE sweep workgroup then fits beside each of them and has the CU's matrix cores while the role waits.
// Measured, same box (profiles/r03_chain_split.txt): n = 14336 19.45 -> 19.07 ms, 16384 27.3 -> 26.4, 18432 37.55 -> 35.97, 24576
// 79.7 -> 78.9, 32768 172.5 -> 170.4, 65536 unchanged; 12288 and below unchanged or slower (the chain's own tiles run at half rate
// beside a busy sweep workgroup), hence the threshold.  Raising the roles' wave priority (s_setprio 3) changes nothing measurable; it
// stays.  GPRC_SERVICE_SHARE=0 / 1 forces it off / on (from n_pad = 10752, where the sweep runs two workgroups per CU).
static bool service_shared(int64_t n_pad) {
  static const int v = [] { const char* e = std::getenv("GPRC_SERVICE_SHARE"); return e ? std::atoi(e) : -1; }();
  return n_pad >= 10752 && (v >= 0 ? v != 0 : n_pad >= 13312);
}

// workgroups the service keeps resident (a CU each)
static int service_workgroups(bool with_inverse, int64_t n_pad) {
  return SERVICE_CORE_WGS + (with_inverse ? TPP : 0) + (chain_split(n_pad) ? CHAIN_HELPERS : 0);
}

// The persistent sweep of a group (launch_trailing_sweep): its workgroups, its tile loop, and whether its head tiles go in slices.
static int launch_group_sweep(gprc_ctx* ctx, double* packed, int64_t n_pad, int64_t g0, int64_t g1, double* winv, int* info_dev, void* sync, void* trace,
                              int service_wgs) {
  int dev = 0, cus = 0;
  GPRC_HIP(hipGetDevice(&dev));
  GPRC_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  // Two workgroups per CU the service leaves free (all co-resident) -- except below n_pad = 10752, where the panel chain is the bound and
  // what counts is how quickly a tile the chain waits for is done: ONE workgroup per CU has the CU's MFMA pipes to itself
  // (measured, same box: n = 8192 6.28 -> 5.99 ms, 10240 9.44 -> 9.21; 12288 13.55 -> 14.60: profiles/r03_factor_schedules.txt).
  // GPRC_SWEEP_WGS=<n> overrides.
  static const int wgs_env = [] { const char* e = std::getenv("GPRC_SWEEP_WGS"); return e ? std::atoi(e) : 0; }();
  const int per_cu = n_pad < 10752 ? 1 : 2;
  // shared service: the resident 4-wave roles' CUs take ONE sweep workgroup each beside the role
  const int shared = service_shared(n_pad) ? service_wgs - 1 - (chain_split(n_pad) ? CHAIN_HELPERS : 0) : 0;
  const int wgs = wgs_env > 0 ? wgs_env : std::max(8, per_cu * (cus - service_wgs) + shared);
  // The tile loop: 2 (no VALU instruction in the loop) where ONE workgroup has the CU; 1 (the first interleaved loop) where two share it:
  // there the faster tile costs 5-8 % (chol_tile.h, trailing_sweep_kernel: profiles/r03_chain_split.txt).
  const int core = (per_cu == 1 && wgs_env <= 0) ? 2 : 1;
  static const int head_slices = [] { const char* e = std::getenv("GPRC_HEAD_SLICES"); return e ? std::atoi(e) : 1; }();   // 0: whole head tiles (A/B switch)
  return launch_trailing_sweep(ctx->stream, packed, n_pad, g0, g1, winv, info_dev, sync, trace, wgs, core, core == 2 ? head_slices : 0);
}

// One GROUP of panels [g0, g1) with the FACTOR SERVICE (kernels_chol.hip): the group's columns have received every earlier panel
// (left-looking pass, or g0 = 0); inside the group the sweep is right-looking with the whole dependent chain -- diagonal blocks, the
// strips around them, the rows of the next diagonal block and that block's update -- in ONE persistent 21-workgroup launch on a side
// stream; the caller's stream carries the ordinary strips and the rest of the within-group update, one launch per panel, tied to the
// service by counters.  Same tiles in the same k order: bit-identical.  sync: panel_service_sync_bytes(P), zeroed once per
// factorisation; launches: service launches on it so far (this one included).
static int factor_group_service(gprc_ctx* ctx, double* packed, int64_t n_pad, double* winv, int* info_dev, double* inv, int64_t g0, int64_t g1, void* sync,
                                void* trace, int launches) {
  hipStream_t s = ctx->stream, side = ctx->side_stream;
  GPRC_TRY(stream_after(ctx, side, s));                       // everything the group's first panel needs precedes the service
  // The explicit inverses ride in the service (four more resident workgroups, off the chain) below n_pad = 20480, where the whole
  // matrix is one group; in the grouped schedule beyond, one launch after the sweep computes them (factor_all_async) and the four
  // CUs go to the update.
  const bool shared = service_shared(n_pad), split = chain_split(n_pad);
  if (shared) {
    hipStream_t side2 = ctx->side_stream2;
    GPRC_TRY(stream_after(ctx, side2, s));
    GPRC_TRY(launch_panel_service(side, packed, n_pad, winv, info_dev, sync, trace, service_carries_inverse(n_pad) ? inv : nullptr, g0, g1, split, 1));
    GPRC_TRY(launch_panel_service(side2, packed, n_pad, winv, info_dev, sync, trace, service_carries_inverse(n_pad) ? inv : nullptr, g0, g1, split, 2));
  } else
  GPRC_TRY(launch_panel_service(side, packed, n_pad, winv, info_dev, sync, trace, service_carries_inverse(n_pad) ? inv : nullptr, g0, g1, split, 0));
  // GPRC_TEST_SERVICE_TIMEOUT=1 (test hook): the FIRST gate of the process waits for a residency count that cannot be reached and
  // gives up at once -- the timeout / refill / service-off path of the fit entry points without a profiler.
  static std::atomic<bool> fire{std::getenv("GPRC_TEST_SERVICE_TIMEOUT") != nullptr};
  GPRC_TRY(launch_service_gate(s, n_pad, info_dev, sync, launches, fire.exchange(false)));   // nothing that waits on the service starts before the service is resident
  GPRC_TRY(launch_panel_strips(s, packed, n_pad, g0, winv, info_dev, sync, trace));        // the later panels' strips ride in the update kernels
  // (Round 3 measured a batched form of this loop -- panel s applied at once only to the next B + 1 panels, the batch's B panels
  //  to everything further in ONE K = 512 B pass, bit-identical -- and it was SLOWER at every size: n = 16384 29.9 -> 31.6 / 30.9 /
  //  30.6 ms for B = 2 / 4 / 8, because the chain idles behind the long pass and the near launches are small and ragged.
  //  profiles/r03_experiments.txt; removed.)
  // ... in ONE persistent launch for the whole group (trailing_sweep_kernel: no partly filled last generation of tiles and no drained
  // GPU at every panel boundary; n = 8192 / 16384: see profiles/r03_factor_schedules.txt).  GPRC_SWEEP=0: one launch per panel.
  static const bool per_panel = [] { const char* e = std::getenv("GPRC_SWEEP"); return e && std::atoi(e) == 0; }();
  if (per_panel) {
    for (int64_t p = g0; p + 1 < g1; ++p) GPRC_TRY(launch_trailing_service(s, packed, n_pad, p, winv, info_dev, sync, trace, g1));
  } else {
    GPRC_TRY(launch_group_sweep(ctx, packed, n_pad, g0, g1, winv, info_dev, sync, trace, service_workgroups(service_carries_inverse(n_pad) && inv, n_pad)));
  }
  GPRC_TRY(stream_after(ctx, s, side));
  if (shared) GPRC_TRY(stream_after(ctx, s, ctx->side_stream2));
  return 0;
}

// All panels of a packed matrix on one GPU, asynchronously (info stays on the device).  Schedule: the panels are taken
// in GROUPS; before a group is factored its panels receive the contributions of every earlier panel in one
// left-looking pass (trailing_range_kernel, K = g0 NB, C tile held in the accumulators); inside the group the panels
// update each other right-looking.  Bit-identical to the plain right-looking sweep (same products, same order).  A
// group is the shortest run of panels whose lower tiles number >= 8192: a left-looking tile is long (K / 512 x 110 us),
// so a pass needs many generations of tiles per CU or the partially filled last one costs more than the saved
// prologues (measured at n = 32768 / 65536: 1024 tiles -6 %, 8192 tiles +3 % / +7 % on the fit against right-looking).
// GPRC_FACTOR=right: one group = right-looking; GPRC_FACTOR=<tiles> changes the threshold.
// inv (may be null): n_pad x NB doubles that receive, per panel, the explicit inverse of its diagonal block (transposed) -- what
// launch_trsv works with; the factor service produces it on the side, the other schedules in one launch after the sweep
int factor_all_async(gprc_ctx* ctx, double* packed, int64_t n_pad, double* winv, int* info_dev, double* inv, bool* used_service) {
  hipStream_t s = ctx->stream;
  const int64_t P = n_pad / NB;
  const char* mode = std::getenv("GPRC_FACTOR");
  int64_t want = want_for(n_pad);
  if (mode && std::strcmp(mode, "right") == 0) want = INT64_MAX;
  else if (mode && std::atoll(mode) > 0) want = std::atoll(mode);
  // GPRC_PANEL=steps: the launch-per-stage panel kernels; GPRC_SERVICE=0: one fused launch per panel inside the groups instead of
  // the factor service.  (A look-ahead sweep on two streams, with and without CU masks, was measured in round 2 and removed in
  // favour of the service: DESIGN.md section 3, profiles/r02_experiments.txt.)
  static const int sv_env = [] { const char* e = std::getenv("GPRC_SERVICE"); return e ? std::atoi(e) : -1; }();
  const bool service = !panel_steps() && sv_env != 0 && P >= 2 && !g_service_off.load();
  if (used_service) *used_service = service;
  DevMem sync;   // flags of every panel + the counters; goes back to the pool when every launch below has been ordered behind it
  void* trace = nullptr;
  if (service) {
    if (!ctx->side_stream) {
      int lo = 0, hi = 0;
      GPRC_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
      GPRC_HIP(hipStreamCreateWithPriority(&ctx->side_stream, hipStreamNonBlocking, hi));
      GPRC_HIP(hipStreamCreateWithPriority(&ctx->side_stream2, hipStreamNonBlocking, hi));
    }
    GPRC_TRY(sync.alloc((int64_t)(panel_service_sync_bytes(P) + 7) / 8));
    GPRC_HIP(hipMemsetAsync(sync.p, 0, panel_service_sync_bytes(P), s));
    static const bool want_trace = std::getenv("GPRC_SERVICE_TRACE") != nullptr;
    if (want_trace && P <= SVC_TRACE_PANELS) {
      if (!ctx->svc_trace) GPRC_HIP(hipMalloc(&ctx->svc_trace, SVC_TRACE_PANELS * 16 * sizeof(int64_t)));
      GPRC_HIP(hipMemsetAsync(ctx->svc_trace, 0, SVC_TRACE_PANELS * 16 * sizeof(int64_t), s));
      trace = ctx->svc_trace;
    }
  }
  int launches = 0;
  auto sweep = [&]() -> int {
    for (int64_t g0 = 0; g0 < P;) {
      int64_t g1 = g0, tiles = 0;
      while (g1 < P && tiles < want) { tiles += panel_tiles(P, g1); ++g1; }
      GPRC_TRY(launch_trailing_range(s, packed, n_pad, 0, g0, g0, g1, 1));   // left-looking: every panel before the group, into the group
      if (service) {
        GPRC_TRY(factor_group_service(ctx, packed, n_pad, winv, info_dev, inv, g0, g1, sync.p, trace, ++launches));
      } else {
        for (int64_t p = g0; p < g1; ++p) {
          GPRC_TRY(factor_panel(ctx, packed, n_pad, p, winv, info_dev));
          if (p + 1 < g1) GPRC_TRY(launch_trailing_update(s, packed, n_pad, p, p + 1, g1, 1));
        }
      }
      g0 = g1;
    }
    return (inv && !(service && service_carries_inverse(n_pad))) ? launch_inv512(s, packed, n_pad, winv, inv, 0, P) : 0;
  };
  const int rc = sweep();
  if (rc != 0 && service) {
    // a launch failed half way: the persistent service kernel may still be running on the side stream and spinning on the flags in
    // `sync` (its waits are bounded).  The block must not go back to the pool -- to be handed to somebody else -- before it has left.
    (void)hipStreamSynchronize(ctx->side_stream);
    if (ctx->side_stream2) (void)hipStreamSynchronize(ctx->side_stream2);
    (void)hipStreamSynchronize(s);
  }
  return rc;
}


int factor_all(gprc_ctx* ctx, double* packed, int64_t n_pad, double* winv, int* info_host, double* inv, bool* used_service) {
  hipStream_t s = ctx->stream;
  GPRC_HIP(hipMemsetAsync(ctx->info_dev, 0, sizeof(int), s));
  GPRC_TRY(factor_all_async(ctx, packed, n_pad, winv, ctx->info_dev, inv, used_service));
  GPRC_HIP(hipMemcpyAsync(info_host, ctx->info_dev, sizeof(int), hipMemcpyDeviceToHost, s));
  GPRC_HIP(hipStreamSynchronize(s));
  if (*info_host < 0) {
    set_error("factorisation: a device-side dependency wait timed out (info = " + std::to_string(*info_host) + ")" + wait_timeout_report() +
              "; the factor is not valid.  The factor service needs its persistent launch and the caller's kernels to run CONCURRENTLY: "
              "under a tool that serialises dispatches (e.g. rocprofv3 --pmc) set GPRC_SERVICE=0");
    return GPRC_ERR_HIP;
  }
  return 0;
}

// vt (m_pad x n_pad) := vt * L^-T.  Schedules with bit-identical results (same products, same order):
//   right-looking: after panel p is solved, subtract its contribution from every column to the right (K = NB per pass);
//   left-looking:  before a GROUP of G panels is solved, subtract the contributions of ALL earlier panels from the
//                  group's columns in one pass (K = p NB), the C tile staying in the accumulators -- one C load/store
//                  and one tile prologue instead of p; inside the group the panels update each other right-looking.
// G is the smallest group that gives a pass (m_pad / 128) * 4 G >= 4096 tiles (eight generations of two workgroups on
// each of 256 CUs: the partially filled last generation of long tiles stays cheap); G >= P degenerates to plain right-looking.  GPRC_SOLVE=right forces that, =left forces G = 1, =<n> G = n.
// sspart != nullptr: the panel solve that finalises a 128-column block also leaves that block's per-row sum of squares in
// sspart[block * m_pad + row] (n_pad / 128 blocks): colSums(v * v) without another pass over the chunk.
// tri_row0 >= 0 (fit()'s gradient, diag(K^-1)): the m_pad rows of vt are rows tri_row0, tri_row0 + 1, ... of the IDENTITY.  Row i of
// the result, (L^-1 e_{tri_row0 + i})^T, is zero left of column tri_row0 + i, so (a) a panel touches only the rows that start at or
// left of its last column and (b) a row tile's left-looking pass starts at the tile's first column: n^3 / 3 flops for the whole
// inverse instead of n^3.  Everything skipped is a product with an exact zero: the same bits as the dense solve
// (test_fit_gradient_triangular_solve_is_bit_identical); sspart must have been zeroed (rows never reached keep their zeros).
// p_end >= 0: only panels [0, p_end) are solved (columns [0, p_end NB) of the result; later columns never feed back into them).
int solve_rows(gprc_ctx* ctx, const double* packed, const double* winv, int64_t n_pad, double* vt, int64_t ldv, int64_t m_pad,
               double* sspart, int64_t tri_row0, int64_t p_end) {
  hipStream_t s = ctx->stream;
  const int64_t P = p_end >= 0 ? std::min(p_end, n_pad / NB) : n_pad / NB;
  const char* mode = std::getenv("GPRC_SOLVE");
  int64_t G = (4096 + (m_pad / 128) * (NB / NBI) - 1) / ((m_pad / 128) * (NB / NBI));
  if (mode && std::strcmp(mode, "left") == 0) G = 1;
  else if (mode && std::atoi(mode) > 0) G = std::atoi(mode);  // an explicit group size
  if ((mode && std::strcmp(mode, "right") == 0) || G > P) G = P;
  auto rows_of = [&](int64_t col_end) {   // rows of the chunk that are not identically zero left of column col_end
    if (tri_row0 < 0) return m_pad;
    return std::max<int64_t>(0, std::min<int64_t>(m_pad, pad_up(col_end - tri_row0, 128)));
  };
  for (int64_t g0 = 0; g0 < P; g0 += G) {
    const int64_t g1 = std::min(P, g0 + G);  // panels [g0, g1)
    const int64_t mg = rows_of(g1 * NB);
    if (mg == 0) continue;
    GPRC_TRY(launch_solve_left(s, vt, ldv, mg, packed, n_pad, g0, g1 - g0, tri_row0));
    static const bool solve_panel_steps = [] { const char* e = std::getenv("GPRC_SOLVE_PANEL"); return e && std::strcmp(e, "steps") == 0; }();
    for (int64_t p = g0; p < g1; ++p) {
      const int64_t ld = panel_ld(n_pad, p);
      const double* pan = packed + panel_offset(n_pad, p);
      const int64_t mp = rows_of((p + 1) * NB);
      if (mp == 0) continue;
      if (!solve_panel_steps) {                   // the four sub-steps of the panel in one launch (GPRC_SOLVE_PANEL=steps: seven launches, same bits)
        GPRC_TRY(launch_solve_panel_fused(s, vt, ldv, mp, packed, n_pad, p, winv, sspart, m_pad));
      } else
      for (int j = 0; j < NB / NBI; ++j) {  // inside the panel, left-looking by 128-column blocks (K = 128 j, as factor_subpanel)
        const int64_t cj = p * NB + (int64_t)j * NBI;  // global column
        const double* wblk = winv + (p * (NB / NBI) + j) * NBI * NBI;
        if (j > 0)
          GPRC_TRY(launch_gemm_nt(s, vt + cj * ldv, ldv, vt + p * NB * ldv, ldv, pan + (int64_t)j * NBI, ld, mp, NBI, (int64_t)j * NBI, 0,
                                  PK_GEMM_INNER));
        GPRC_TRY(launch_trsm_panel(s, vt + cj * ldv, ldv, mp, wblk, sspart ? sspart + (cj / NBI) * m_pad : nullptr));
      }
      const int64_t right = (g1 - (p + 1)) * NB;  // the rest of the group
      if (right > 0)
        GPRC_TRY(launch_gemm_nt(s, vt + (p + 1) * NB * ldv, ldv, vt + p * NB * ldv, ldv, pan + NB, ld, mp, right, NB, 0, PK_SOLVE_UPDATE));
    }
  }
  return 0;
}

// GPRC_FITGRAD_DENSE=1: gprc_fit_gradient sends the identity through solve_rows in the dense n^3 form (tri_row0 = -1)
bool identity_solve_dense() {
  static const bool dense = std::getenv("GPRC_FITGRAD_DENSE") != nullptr;
  return dense;
}

// doubles of partial-sum workspace per chunk row: the fill's K*^T w partials (one per 64 columns) + the solve's
// sums of squares (one per 128 columns)
int64_t predict_partials(int64_t n_pad) { return fill_mean_tiles(n_pad) + n_pad / NBI; }

static int chunk_rows(const gprc_ctx* ctx, int64_t n_pad, int64_t ns) {
  int64_t rows = ((int64_t)(ctx->chunk_bytes / (sizeof(double) * (size_t)n_pad)) - ctx->vt_pad) / 256 * 256;
  if (rows < 256) rows = 256;
  const int64_t need = pad_up(ns, 128);
  return (int)(rows < need ? rows : need);
}

// The workspaces of a chunked pass over test points (K*^T chunk, its partial sums, k(x*, x*)): `rows` rows per chunk.
// The budget (GPRC_CHUNK_BYTES, 40 GiB) is only a wish: the chunk is sized to what the device can actually give --
// hipMemGetInfo's free figure plus what the context's slots already hold, less a reserve -- and if an allocation still fails
// (another process took the memory in between; a fragmented heap) the chunk is HALVED and tried again, down to 256 rows, before
// the call fails with GPRC_ERR_NOMEM.  Results do not depend on the chunking, bit for bit (a row's arithmetic depends on columns
// only: test_chunked_predict_is_bitwise_chunk_invariant), so shrinking is free.  want_tmp: also slot 2 (`rows` doubles).
int chunk_workspace(gprc_ctx* ctx, int64_t n_pad, int64_t ns, bool want_tmp, int64_t* rows_out, double** vt, double** part, double** tmp) {
  int64_t rows = chunk_rows(ctx, n_pad, ns);
  const int64_t per_row = (n_pad + predict_partials(n_pad) + 1) * (int64_t)sizeof(double);
  static const bool ignore_meminfo = std::getenv("GPRC_IGNORE_MEMINFO") != nullptr;   // test hook: exercise the retry path itself
  size_t free_b = 0, total_b = 0;
  if (!ignore_meminfo && hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
    int64_t have = 0;
    for (int i = 0; i < 3; ++i) have += ctx->ws_cap[i] * (int64_t)sizeof(double);
    const int64_t avail = (int64_t)free_b + have - ((int64_t)256 << 20);   // 256 MiB stay free: the pool's small blocks, the runtime
    const int64_t fit = (avail / per_row - ctx->vt_pad) / 256 * 256;
    if (fit < rows) rows = fit < 256 ? 256 : fit;
  } else {
    (void)hipGetLastError();
  }
  for (;;) {
    const int64_t ldv = rows + ctx->vt_pad;
    int rc = ws_get(ctx, 0, ldv * n_pad, vt);
    if (rc == 0) rc = ws_get(ctx, 1, rows * predict_partials(n_pad), part);
    if (rc == 0 && want_tmp) rc = ws_get(ctx, 2, rows, tmp);
    if (rc == 0) break;
    if (rc != GPRC_ERR_NOMEM || rows <= 256) return rc;
    pool_trim(ctx);                                    // cached blocks of earlier calls go back first
    rows = std::max<int64_t>(256, rows / 2 / 256 * 256);
  }
  *rows_out = rows;
  return 0;
}

}  // namespace gprc

using namespace gprc;

extern "C" {

int gprc_dev_factor_panel(gprc_ctx* ctx, double* packed, int64_t n_pad, int64_t p, double* winv, int* info_dev) {
  GPRC_TRY(use_device_unless(ctx, n_pad % NB || p < 0 || p >= n_pad / NB || !info_dev, "factor_panel: bad arguments"));
  return factor_panel(ctx, packed, n_pad, p, winv, info_dev);
}

int gprc_dev_factor_subpanel(gprc_ctx* ctx, double* packed, int64_t n_pad, int64_t p, int j, int part, double* winv, int* info_dev) {
  GPRC_TRY(use_device_unless(ctx, n_pad % NB || p < 0 || p >= n_pad / NB || j < 0 || j >= NB / NBI || part < 0 || part > 2 || !info_dev,
                             "factor_subpanel: bad arguments"));
  return factor_subpanel(ctx, packed, n_pad, p, j, part, winv, info_dev);
}
int gprc_dev_factor_all(gprc_ctx* ctx, double* packed, int64_t n_pad, double* winv, int* info_dev, double* inv) {
  GPRC_TRY(use_device_unless(ctx, !packed || !winv || !info_dev || n_pad <= 0 || n_pad % NB, "dev_factor_all: bad arguments"));
  return factor_all_async(ctx, packed, n_pad, winv, info_dev, inv);
}
int gprc_factor_service(int on) {
  const int was = g_service_off.load() ? 0 : 1;
  if (on == 0) g_service_off.store(true);
  else if (on > 0) g_service_off.store(false);
  return was;
}

int gprc_dev_solve_rows(gprc_ctx* ctx, const double* packed, const double* winv, int64_t n_pad, double* vt,
                        int64_t ld, int64_t m_pad) {
  GPRC_TRY(use_device_unless(ctx, m_pad % 128 || n_pad % NB || ld < m_pad || ld % 2, "solve_rows: bad padding"));
  return solve_rows(ctx, packed, winv, n_pad, vt, ld, m_pad);
}

int gprc_dev_reverse_factor(gprc_ctx* ctx, const double* packed, const double* winv, int64_t n_pad, double* packed_rev, double* winv_rev) {
  GPRC_TRY(use_device_unless(ctx, !packed || !winv || !packed_rev || !winv_rev || n_pad <= 0 || n_pad % NB, "dev_reverse_factor: bad arguments"));
  return launch_reverse_factor(ctx->stream, packed, winv, n_pad, packed_rev, winv_rev);
}

int gprc_prof_panel_trace(gprc_ctx* ctx, int side, int64_t* ticks_out, int n) {
  GPRC_TRY(use_device_unless(ctx, !ticks_out || n < 1 || n > 24, "prof_panel_trace: 1..24 stamps"));
  GPRC_HIP(hipDeviceSynchronize());
  GPRC_HIP(hipMemcpy(ticks_out, static_cast<char*>(ctx->sync_dev) + (side ? 256 : 0) + 64, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost));
  return 0;
}

int gprc_prof_service_trace(gprc_ctx* ctx, int64_t* ticks_out, int panels) {
  GPRC_TRY(use_device_unless(ctx, !ticks_out || panels < 1 || panels > SVC_TRACE_PANELS, "prof_service_trace: 1..48 panels"));
  if (!ctx->svc_trace) { set_error("prof_service_trace: no traced sweep on this context (set GPRC_SERVICE_TRACE before the first call)"); return GPRC_ERR_ARG; }
  GPRC_HIP(hipDeviceSynchronize());
  GPRC_HIP(hipMemcpy(ticks_out, ctx->svc_trace, sizeof(int64_t) * 16 * (size_t)panels, hipMemcpyDeviceToHost));
  return 0;
}

// ---- layout helpers + device-level building blocks ------------------------------------------------
int64_t gprc_panel_width(void) { return NB; }
int64_t gprc_pad(int64_t n) { return pad_up(n, NB); }
int64_t gprc_panel_count(int64_t n_pad) { return n_pad / NB; }
int64_t gprc_panel_offset(int64_t n_pad, int64_t p) { return panel_offset(n_pad, p); }
int64_t gprc_panel_elems(int64_t n_pad, int64_t p) { return panel_ld(n_pad, p) * NB; }
int64_t gprc_packed_size(int64_t n_pad) { return panel_offset(n_pad, n_pad / NB); }
int64_t gprc_winv_size(int64_t n_pad) { return n_pad * NBI; }
int64_t gprc_trsv_work_size(int64_t n_pad) { return n_pad + n_pad / NB + 8; }   // x_p staging + one gate (8 bytes) per panel
int64_t gprc_solve_inv_size(int64_t n_pad) { return n_pad * NB; }
int64_t gprc_rowreduce_splits(int64_t cols) { return rowreduce_splits(cols); }

int gprc_dev_fill_panel(gprc_ctx* ctx, int kernel, const double* params_host, int n_params, const double* X,
                        int64_t d, int64_t n, int64_t n_pad, double noise, double* packed, int64_t p) {
  GPRC_TRY(use_device_unless(ctx, n_pad != pad_up(n, NB) || p < 0 || p >= n_pad / NB, "fill_panel: bad layout arguments"));
  KernelSpec ks;
  GPRC_TRY(make_spec(kernel, params_host, n_params, d, &ks));
  return launch_fill(ctx->stream, ks, X, n, X, n, d, packed + panel_offset(n_pad, p), panel_ld(n_pad, p), p * NB, n_pad - p * NB,
                     p * NB, NB, PAD_IDENTITY, noise);
}

int gprc_dev_solve_prepare(gprc_ctx* ctx, const double* packed, const double* winv, int64_t n_pad, double* inv, int64_t p_begin, int64_t p_end) {
  GPRC_TRY(use_device_unless(ctx, !packed || !winv || !inv || n_pad <= 0 || n_pad % NB || p_begin < 0 || p_end > n_pad / NB, "dev_solve_prepare: bad arguments"));
  return launch_inv512(ctx->stream, packed, n_pad, winv, inv, p_begin, p_end);
}
int gprc_dev_update_range(gprc_ctx* ctx, double* packed, int64_t n_pad, int64_t p_begin, int64_t p_end, int64_t q_begin, int64_t q_end,
                          int64_t q_stride) {
  GPRC_TRY(use_device_unless(ctx, !packed || n_pad <= 0 || n_pad % NB || p_begin < 0 || p_end > n_pad / NB, "dev_update_range: bad arguments"));
  if (p_end - p_begin == 1) return launch_trailing_update(ctx->stream, packed, n_pad, p_begin, q_begin, q_end, q_stride);  // the K = 512 kernel
  return launch_trailing_range(ctx->stream, packed, n_pad, p_begin, p_end, q_begin, q_end, q_stride);
}
int gprc_dev_update_trailing(gprc_ctx* ctx, double* packed, int64_t n_pad, int64_t p, int64_t q_begin,
                             int64_t q_end, int64_t q_stride) {
  GPRC_TRY(use_device_unless(ctx, n_pad % NB, "update_trailing: bad n_pad"));
  if (q_begin >= q_end) return 0;
  return launch_trailing_update(ctx->stream, packed, n_pad, p, q_begin, q_end, q_stride);
}

int gprc_dev_trsv(gprc_ctx* ctx, const double* packed, const double* inv, int64_t n_pad, double* b, int transpose,
                  double* work) {
  GPRC_TRY(use_device_unless(ctx, !packed || !inv || !b || !work || n_pad <= 0 || n_pad % NB, "dev_trsv: bad arguments"));
  return launch_trsv(ctx->stream, packed, inv, n_pad, b, transpose, work);
}

int gprc_dev_trsv_step(gprc_ctx* ctx, const double* packed, const double* inv, int64_t n_pad, double* b, int transpose, int64_t p, double* work) {
  GPRC_TRY(use_device_unless(ctx, !packed || !inv || !b || !work || n_pad <= 0 || n_pad % NB, "dev_trsv_step: bad arguments"));
  return launch_trsv_step(ctx->stream, packed, inv, n_pad, b, transpose, (int)p, work);
}

int gprc_dev_fill_cross(gprc_ctx* ctx, int kernel, const double* params_host, int n_params, const double* X_star,
                        int64_t d, int64_t m, int64_t m_pad, const double* X, int64_t n, int64_t n_pad, double* vt,
                        int64_t ld) {
  GPRC_TRY(use_device_unless(ctx, m_pad % 128 || m_pad < m || n_pad < n || ld < m_pad || ld % 2, "fill_cross: bad padding"));
  KernelSpec ks;
  GPRC_TRY(make_spec(kernel, params_host, n_params, d, &ks));
  return launch_fill(ctx->stream, ks, X_star, m, X, n, d, vt, ld, 0, m_pad, 0, n_pad, PAD_ZERO, 0.0);
}

int gprc_dev_row_reduce(gprc_ctx* ctx, const double* vt, int64_t ld, int64_t rows, int64_t cols, const double* w,
                        double* out, double* work) {
  GPRC_TRY(use_device(ctx));
  return launch_row_reduce(ctx->stream, vt, ld, rows, cols, w, out, work);
}

int gprc_dev_gemm_nt(gprc_ctx* ctx, double* Cm, int64_t ldc, const double* A, int64_t lda, const double* B, int64_t ldb, int64_t M, int64_t N,
                     int64_t K, int lower) {
  GPRC_TRY(use_device_unless(ctx, !Cm || !A || !B || ldc < M || lda < M || ldb < N, "dev_gemm_nt: bad arguments"));
  return launch_gemm_nt(ctx->stream, Cm, ldc, A, lda, B, ldb, M, N, K, lower ? 1 : 0, PK_COV_SYRK);
}

int gprc_dev_gram_rows(gprc_ctx* ctx, const double* vt, int64_t ld, int64_t rows, int64_t n_pad, double* packed) {
  GPRC_TRY(use_device(ctx));
  return launch_gram_rows(ctx->stream, vt, ld, rows, n_pad, packed);
}

int gprc_dev_col_reduce(gprc_ctx* ctx, const double* vt, int64_t ld, int64_t rows, int64_t cols, const double* w, double* out) {
  GPRC_TRY(use_device(ctx));
  return launch_col_reduce(ctx->stream, vt, ld, rows, cols, w, out);
}

int gprc_dev_logp(gprc_ctx* ctx, const double* packed, int64_t n_pad, int64_t n, const double* y, const double* alpha,
                  double* out_dev) {
  GPRC_TRY(use_device(ctx));
  return launch_logp(ctx->stream, packed, n_pad, n, y, alpha, out_dev);
}

}  // extern "C"
