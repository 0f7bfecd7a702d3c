// kernels_chol.hip -- the fp64 Cholesky's kernels that hand work over BETWEEN workgroups through agent-scope flags and counters
// (PanelSync), each with its launcher, and the records their bounded waits leave when one gives up (g_wait_diag: one home, the library
// is built without relocatable device code -- every kernel that can record a wait sits in this unit beside the host functions that
// read the records).  panel_fused_kernel: a whole panel's dependent chain in one launch; panel_service_kernel: every panel's in one
// persistent launch (the factor service), with the caller's-stream kernels that go with it (service gate, strips, trailing update per
// panel or as one persistent sweep); the explicit inverse of a panel's diagonal block, a role of the service and a kernel of its own.
// Tile core and diagonal-block factorisation: chol_tile.h.  Which of these run, and with which parameters: gprc_sched.hip.
#include <algorithm>
#include <mutex>

#include "chol_tile.h"

namespace gprc {
namespace {

__global__ __launch_bounds__(1024) void potf2_inv_blocked_kernel(double* A, int64_t lda, double* winv, int* info, int col0) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  potf2_blocked_body<16>(sm, A, lda, winv, info, col0);
}

// ------------------------------------------------------------------------------------------------
// One launch per 512-column panel: diagonal blocks, panel solves and in-panel updates of all four 128-column sub-steps.
//
// The launch-per-stage form (factor_subpanel: update K = 128 j -> diagonal block -> panel solve, 4 x 3 dependent launches
// per panel) leaves the GPU almost empty while each stage drains: ~570 us per panel, which is most of the fit at
// n = 8192..16384 and most of one rank's share of an 8-rank sweep.  Here the stages of different 128-row strips overlap
// and only the true dependencies remain, carried by agent-scope flags inside one grid of 512-thread workgroups:
//   factor workgroup (ticket 0, 8 waves)   the whole critical chain, with no hand-off on it:
//                                           for j = 0..3: factor + invert block (j, j) in LDS (potf2_blocked_body<8>),
//                                           publish W_j; then, itself, the two tiles the NEXT diagonal block waits for:
//                                           L(j+1, j) = C'(j+1, j) Winv_j^T (publish R_{j+1}) and
//                                           C(j+1, j+1) -= L(j+1, j) L(j+1, j)^T
//   diagonal strips s = 1..3 (tickets 2..4, one 4-wave team): blocks (s, 0..s-2) like any strip; then everything of
//                                           blocks (s, s-1) and (s, s) that does not need L(s-1, s-1) yet -- the updates
//                                           with the columns left of block s-1 -- and publish E_s
//   other strips, two per workgroup (two 4-wave teams with their own LDS halves, in lockstep: the same flags, the same
//                                           barrier count): for j = 0..3: wait R_j (j > 0), C(s,j) -= L(s,<j) L(j,<j)^T,
//                                           wait W_j, C(s,j) := C(s,j) Winv_j^T
// Every tile is a gemm_tile_128 call with the same operands and the same K order as in the launch-per-stage form (an update
// split in two calls continues the same accumulator chain from the stored value), and the diagonal block goes through the
// same 16x16-block arithmetic: the results are bit-identical.
// No deadlock, whatever the dispatch order, the number of resident workgroups (149 KB of LDS: one per CU) or what else runs
// on the GPU: roles are dealt by a ticket counter in START order; every flag is published by one of the first five tickets
// (factor role and diagonal strips); those five wait only on each other, in an order without cycles (the factor role
// publishes W_0, R_1, W_1, R_2 ... before it waits for the E_s that needs them); and a workgroup with a later ticket can
// only be running -- and spinning -- when all five earlier ones have started.
// Hand-off protocol: MI355X_MICROARCH.md "inter-workgroup visibility" (plain stores, every wave's vmcnt(0), workgroup
// barrier, one lane's agent release fence + vmcnt(0), relaxed agent store of the flag; one lane polls with relaxed agent
// loads, agent acquire fence + vmcnt(0), workgroup barrier, plain / LDS-DMA loads).
// ------------------------------------------------------------------------------------------------
struct PanelSync { int ticket; int failed; int W[4]; int E[4]; int R[4]; int LA; int SU; };   // 16 ints, zeroed before the launch
static_assert(TPP <= 4, "PanelSync holds four flags of each kind and LA four 8-bit fields: the factor service is written for NB = 4 x 128");
// Bound of every device-side dependency wait: WALL time (s_memrealtime, 100 MHz), not a poll count -- a busy, shared GPU slows the
// polls down but must not shorten the patience.  Legitimate waits are below 10 ms (one trailing update at n <= 24576).
constexpr unsigned long long WAIT_LIMIT_TICKS = 400000000ULL;   // 4 s
// (factor service only -- LA: the look-ahead strips' finished blocks, one 8-bit count per 128-column sub-step j (a strip adds
//  1 << 8 j after block (s, j)): field j = TPP when all four strips have finished sub-step j.  A single sum over the sub-steps --
//  the round-2 form -- reads "4 (j + 1)" also when one strip is a sub-step ahead and another one behind, which happens as soon as
//  the service's workgroups do not start together (another context's kernels on the GPU): profiles/r03_la_counter_race.txt.
//  A strip goes through its blocks in order, so field TPP - 1 = TPP -- LA >= TPP << 24 -- means rows [NB, 2 NB) are final;
//  E[0], E[1]: blocks (s, j <= s-2) the diagonal strips s = 2, 3 have finished;
//  SU: the split chain's counters, eight 4-bit fields with 3-bit counts -- field j: 32-row slices of L(j, j-1) that are final (the chain
//  helpers' solve phase), field 4 + j: slices of block (j, j) that have received L(j, j-1) (their update phase); each reaches
//  CHAIN_HELPERS.  j = 0 stands for the step BEHIND the panel: slices of L(4, 3), and of tile (0, 0) of the next diagonal block; bit 3 of
//  field 0: that tile has received the k-chunks 0..2 (role SERVICE_D0).  R[0]: block (4, 3) is ready for its solve (look-ahead strip 4))

// Who gave up, and on what: every wait of a factorisation that runs out its bound -- and every wait that was still unsatisfied when it
// saw that somebody else had (site + 10) -- leaves a record for the host (wait_timeout_report, gprc_prof_wait_timeout): up to
// WAIT_DIAG_RECORDS records of 8 ints behind a counter -- [0] site (1 flag, 2 count, 3 field, 4 chain, 5 sweep, 6 gate), [1] blockIdx.x,
// [2] gridDim.x, [3] the value needed, [4] the value seen, [5] the awaited word's index inside its panel's PanelSync (or its distance
// from it), [6] threads per workgroup, [7] low 32 bits of the PanelSync's address (which panel)
constexpr int WAIT_DIAG_RECORDS = 48;
__device__ int g_wait_diag[8 * (WAIT_DIAG_RECORDS + 1)];
__device__ __attribute__((noinline)) void wait_diag(int site, int need, int seen, const int* word, const void* sy) {
  const int k = atomicAdd(&g_wait_diag[0], 1);
  if (k >= WAIT_DIAG_RECORDS) return;
  int* r = g_wait_diag + 8 * (k + 1);
  r[0] = site; r[1] = (int)blockIdx.x; r[2] = (int)gridDim.x; r[3] = need; r[4] = seen;
  r[5] = sy ? (int)(word - static_cast<const int*>(sy)) : -1; r[6] = (int)blockDim.x; r[7] = (int)(uintptr_t)sy;
}

// relaxed: the caller is throughput work (a strip riding in the sweep kernel), not a role of the chain: it looks at the flag once per
// microsecond instead of every ~50 ns.  Hundreds of workgroups polling flags and counters at full rate slow every device-scope access
// down -- the chain's own publishes and polls included (measured with the round-3 tile core, whose faster tiles left the sweep's
// workgroups waiting longer: ticket atomics 6 -> 16 us, n = 8192 factorisation 6.27 -> 6.71 ms; tools/sweep_prof.py).
__device__ __forceinline__ void relaxed_pause() { __builtin_amdgcn_s_sleep(32); }   // 32 x 64 clocks ~ 0.9 us

// THE bounded wait; the whole workgroup calls it.  One lane polls -- satisfied() loads the awaited word(s) with relaxed agent-scope loads and
// compares -- and pauses between two looks (s_sleep SLEEP; relaxed: relaxed_pause instead); at every 256th miss it checks the two ways out every
// wave reaches.  record(site) leaves the wait_diag record of what was still missing.  Then the acquire side of the hand-off protocol.
template <int SITE, int SLEEP, typename Satisfied, typename Record>
__device__ __forceinline__ void bounded_wait(PanelSync* sy, int* info, bool relaxed, Satisfied satisfied, Record record) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's own stores: its team-mates re-read them after the barrier
  if (threadIdx.x == 0) {
    int spins = 0;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (!satisfied()) {
      if (relaxed) relaxed_pause();
      else __builtin_amdgcn_s_sleep(SLEEP);
      if ((++spins & 255) != 0) continue;
      // somebody has already given up (e.g. a profiler that serialises dispatches keeps producer and consumer kernels apart): every
      // later wait of the factorisation returns at once instead of running out its own bound
      if (__hip_atomic_load(info, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == GPRC_INFO_WAIT_TIMEOUT) { record(SITE + 10); break; }
      // exit condition every wave reaches (a producer that never publishes must not leave this workgroup spinning on the GPU
      // for ever): after WAIT_LIMIT_TICKS of wall time give up, let the grid drain, and tell the host through the ONE word it
      // always reads after a factorisation -- info = GPRC_INFO_WAIT_TIMEOUT (< 0; LAPACK infos are > 0)
      if (__builtin_amdgcn_s_memrealtime() - t0 > WAIT_LIMIT_TICKS) {
        record(SITE);
        __hip_atomic_store(&sy->failed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        atomicExch(info, GPRC_INFO_WAIT_TIMEOUT);
        break;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
}
#define GPRC_PEEK(word) __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

__device__ __forceinline__ void panel_flag_wait(int* flag, PanelSync* sy, int* info, bool relaxed = false) {
  bounded_wait<1, 2>(sy, info, relaxed, [&] { return GPRC_PEEK(flag) != 0; }, [&](int site) { wait_diag(site, 1, 0, flag, sy); });
}

__device__ __forceinline__ void panel_flag_publish(int* flag) {               // the whole workgroup calls it
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__device__ __forceinline__ void panel_ready_wait(int* ctr, int need, PanelSync* sy, int* info, bool relaxed = false) {
  bounded_wait<2, 2>(sy, info, relaxed, [&] { return GPRC_PEEK(ctr) >= need; }, [&](int site) { wait_diag(site, need, GPRC_PEEK(ctr), ctr, sy); });
}

// waits until the 8-bit field at `shift` of *ctr has reached `need` (the look-ahead strips' per-sub-step counts in LA)
__device__ __forceinline__ void panel_field_wait(int* ctr, int shift, int need, PanelSync* sy, int* info) {
  bounded_wait<3, 2>(sy, info, false, [&] { return ((GPRC_PEEK(ctr) >> shift) & 0xff) >= need; },
                     [&](int site) { wait_diag(site, need << shift, GPRC_PEEK(ctr), ctr, sy); });
}

__device__ __forceinline__ void panel_count_publish(int* ctr, int add) {      // the whole workgroup calls it
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_fetch_add(ctr, add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Workgroup barriers gemm_tile_128 executes for a K-deep tile WITHOUT the SSQ epilogue: one after the first DMA and one
// per further k-tile.  Waves of a workgroup that sit a tile out call this so that the barrier counts match.
__device__ __forceinline__ void gemm_tile_shadow_barriers(int K) {
  const int KT = K / G_KB;
  for (int b = 0; b < KT; ++b) __builtin_amdgcn_s_barrier();
}

// ------------------------------------------------------------------------------------------------
// The SPLIT chain (factor service only).  Between two diagonal blocks of a panel the chain runs two 128 x 128 x 128 tiles -- the solve
// L(j+1, j) = C'(j+1, j) Winv_j^T and the update C(j+1, j+1) -= L(j+1, j) L(j+1, j)^T -- and on ONE CU each is bound by that CU's MFMA
// rate (13.7 us of MFMAs + 3.5 us of prologue: 17.4 and 20.5-24 us measured, profiles/r03_chain_traces_after_diag16.txt; a second team
// on the same CU changes nothing).  Here CHAIN_HELPERS = 4 resident workgroups (8 waves each, a CU each) take 32 ROWS of both tiles
// each: a quarter of the MFMAs (3.4 us), operands loaded in one go (the slice's 32 x 128 A rows through LDS, every wave's 16 B rows
// straight into registers), results stored write-through (sc1) and handed on by counters -- solve slices to each other (the update
// needs all of L(j+1, j)), update slices to the factor role, which then loads the block itself (potf2_blocked_body, not preloaded).
// Every output element is still acc = C (or 0), then for the k-steps 0..31 ascending acc = v_mfma_f64_16x16x4(B strip value, A strip
// value, acc) with the update's negate-A bit: the same operand roles, k order and accumulator start as gemm_tile_128 -- identical bits.
// ------------------------------------------------------------------------------------------------
#ifdef GPRC_CHAIN_PROF
constexpr int GPRC_CHAIN_PROF_PANEL = GPRC_CHAIN_PROF;
#else
constexpr int GPRC_CHAIN_PROF_PANEL = -1;
#endif
constexpr int PANEL_LA_TILES = TPP * TPP;             // tiles of a panel's rows [NB, 2 NB)
constexpr int AUX_STRIDE = 2 * TPP + PANEL_LA_TILES;  // ints per panel in the sync block's last array: 2 TPP early-chunk flags, then the slice counts of the sweep's head tiles
constexpr int CHAIN_LDS_LD = 48;                  // doubles per k-slice of the A image: 32 rows + 16 pad (consecutive k-slices 32 banks apart)
static_assert(CHAIN_HELPERS * 32 == 128 && CHAIN_HELPERS < 8, "SU holds 3-bit counts of 32-row slices (bit 3 of field 0 is a flag)");

#ifdef GPRC_CHAIN_PROF
// measurement build: s_memrealtime stamps (100 MHz) of panel GPRC_CHAIN_PROF's chain -- [0..31] helper 0 (8 per sub-step: W seen,
// operands in, MFMAs done, stored + counted, S seen, operands in, MFMAs done, stored + counted), [32 + 4 j ..] the factor role
// (U seen, potf2 done, W published)
__device__ unsigned long long g_chain_prof[64];
#define CHAIN_STAMP(on, k) do { if ((on) && threadIdx.x == 0) g_chain_prof[k] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define CHAIN_STAMP(on, k)
#endif

// waits until ((*a >> sa) & ma) >= va and (b == null or ((*b >> sb) & mb) >= vb); the whole workgroup calls it; the polls fly together
__device__ __forceinline__ void chain_wait2(int* a, int sa, int ma, int va, int* b, int sb, int mb, int vb, PanelSync* sy, int* info) {
  int xa, xb;
  bounded_wait<4, 1>(sy, info, false,
                     [&] {
                       xa = (GPRC_PEEK(a) >> sa) & ma;
                       xb = b ? (GPRC_PEEK(b) >> sb) & mb : vb;
                       return xa >= va && xb >= vb;
                     },
                     [&](int site) {
                       if (xa < va) wait_diag(site, va << sa, GPRC_PEEK(a), a, sy);
                       else wait_diag(site, vb << sb, GPRC_PEEK(b), b, sy);
                     });
}

// C (32 rows x 128 columns, column-major) = (SET ? 0 : C) -/+ A (32 x 128) B (128 x 128)^T on 512 threads: wave w the columns
// [16 w, 16 w + 16).  lds: 128 x CHAIN_LDS_LD doubles.  C may be A (the solve in place: every A element is in LDS before the first
// store).  Stores are write-through; the caller publishes (every wave's vmcnt(0), barrier, counter).
template <bool SET>
__device__ __forceinline__ void chain_slice_32(double* C_, int64_t ldc, const double* A_, int64_t lda, const double* B_, int64_t ldb, double* lds_,
                                               bool prof = false, int stamp0 = 0) {
  // explicit address spaces: inside a non-inlined role the pointers are generic, and FLAT loads would tie the LDS waits to the
  // outstanding global loads (a flat instruction counts in vmcnt and lgkmcnt)
  typedef __attribute__((address_space(1))) double gdouble;
  typedef __attribute__((address_space(3))) double ldouble;
  gdouble* C = (gdouble*)C_;
  const gdouble* A = (const gdouble*)A_;
  const gdouble* B = (const gdouble*)B_;
  ldouble* lds = (ldouble*)lds_;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int fk = lane >> 4, fr = lane & 15;
  constexpr int NEG = SET ? 0 : 1;
  // the A slice: thread t brings rows [8 (t & 3), +8) of k-slice t >> 2
  const gdouble* asrc = A + 8 * (t & 3) + (int64_t)(t >> 2) * lda;
  double av[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) av[i] = asrc[i];
  double4_t acc[2];
  gdouble* Cw = C + fr + (int64_t)(16 * wave + fk) * ldc;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[m][r] = SET ? 0.0 : Cw[16 * m + (int64_t)(4 * r) * ldc];
  // this wave's 16 B rows, all 32 k-steps: one double per lane and step
  const gdouble* bsrc = B + (16 * wave + fr) + (int64_t)fk * ldb;
  double b[32];
#pragma unroll
  for (int s = 0; s < 32; ++s) b[s] = bsrc[(int64_t)(4 * s) * ldb];
  ldouble* adst = lds + (t >> 2) * CHAIN_LDS_LD + 8 * (t & 3);
#pragma unroll
  for (int i = 0; i < 8; ++i) adst[i] = av[i];
  __syncthreads();
  const ldouble* ap = lds + fk * CHAIN_LDS_LD + fr;
  double a0[2], a1[2];   // operand reads two k-steps ahead
  a0[0] = ap[0]; a1[0] = ap[16];
  a0[1] = ap[4 * CHAIN_LDS_LD]; a1[1] = ap[4 * CHAIN_LDS_LD + 16];
#pragma unroll
  for (int s = 0; s < 32; ++s) {
    const double x0 = a0[s & 1], x1 = a1[s & 1];
    if (s + 2 < 32) { a0[s & 1] = ap[4 * (s + 2) * CHAIN_LDS_LD]; a1[s & 1] = ap[4 * (s + 2) * CHAIN_LDS_LD + 16]; }
    acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(b[s], x0, acc[0], 0, 0, NEG);
    acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(b[s], x1, acc[1], 0, 0, NEG);
#ifdef GPRC_CHAIN_PROF
    if (s == 0) CHAIN_STAMP(prof, stamp0);       // the first MFMAs are issued: A image and b[0] are in
#endif
  }
#ifdef GPRC_CHAIN_PROF
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
  if (prof && threadIdx.x == 0) { double sink = acc[0][0] + acc[1][3]; asm volatile("" :: "v"(sink)); g_chain_prof[stamp0 + 1] = __builtin_amdgcn_s_memrealtime(); }
#endif
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) __hip_atomic_store(&Cw[16 * m + (int64_t)(4 * r) * ldc], acc[m][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the slice is stored: every wave's vmcnt(0), barrier, then one lane adds `add` to *ctr (write-through payload: no write-back).
// Returns (to thread 0 only) the counter's previous value.
__device__ __forceinline__ int chain_publish(int* ctr, int add) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  return threadIdx.x == 0 ? __hip_atomic_fetch_add(ctr, add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
}

// Chain helper q of one panel (512 threads): rows [32 q, 32 q + 32) of the solve tile of every sub-step and of EVERY update of the
// diagonal blocks (1,1), (2,2), (3,3) -- the one the next potf2 waits for, and, in the 35 us that potf2 then runs, the updates of the
// later diagonal blocks with the column just finished (the diagonal strips' own share in the unsplit form: with the two chain tiles
// down from 38 to 17 us the chain waited 29 us for strip 3's K = 256 tiles, tools/chain_prof.py).  A helper touches only its own 32
// rows of those blocks, k-chunk after k-chunk in order: no flag between them, and the same accumulator chain through memory.
// strip_progress: E[0] / E[1], the finished blocks (s, j <= s-2) of the diagonal strips s = 2, 3.
// dnext (null: no next panel in the launch's group): tile (0, 0) of the NEXT panel's diagonal block, leading dimension ldn.  The path from
// W_3 to the next chain is the same pattern once more -- L(4, 3) = C'(4, 3) Winv_3^T, D(0, 0) -= L(4, 3) L(4, 3)^T, potf2 -- and was a
// 17-us solve on the look-ahead strip's CU plus a 20-us tile on a next-diagonal-block role's; the helpers do both in slices: the
// look-ahead strip TPP hands block (4, 3) over when it has received the panel's earlier columns (R[0]), role SERVICE_D0 hands tile
// (0, 0) over when it has received the k-chunks 0..2 (bit 3 of SU), the last solve slice counts the
// block into LA for that strip, the last update slice counts the tile into ready_next, and the next factor role starts on the
// update slices' count (field 4 of SU) instead of waiting for the other nine tiles, which it does not read.
// ready_mine (null: first panel of the launch): the count of finished tiles of THIS panel's diagonal block -- the helpers' first solve
// reads tile (1, 0), which the factor role no longer waits for.
__device__ __attribute__((noinline)) void panel_chain_helper_role(double* sm, double* pan, int64_t ld, double* wp, int* info, PanelSync* sy, int q,
                                                                  bool prof, double* dnext, int64_t ldn, int* ready_next, int* ready_mine) {
  for (int j = 0; j + 1 < TPP; ++j) {
    double* Cn = pan + (int64_t)(j + 1) * NBI + (int64_t)j * NBI * ld;            // block (j+1, j)
    double* Dn = pan + (int64_t)(j + 1) * NBI + (int64_t)(j + 1) * NBI * ld;      // block (j+1, j+1)
    const int fs = 4 * (j + 1), fu = 16 + 4 * (j + 1);
    // solve: W_j published; j > 0: block (j+1, j) has received the columns left of block j (E = 1, the diagonal strip j+1)
    chain_wait2(&sy->W[j], 0, 1, 1, j > 0 ? &sy->E[j + 1] : ready_mine, 0, 0xffff, j > 0 ? 1 : PANEL_DIAG_TILES, sy, info);
    CHAIN_STAMP(prof, 8 * j);
    chain_slice_32<true>(Cn + 32 * q, ld, Cn + 32 * q, ld, wp + (int64_t)j * NBI * NBI, 128, sm, prof, 8 * j + 1);
    const int before = chain_publish(&sy->SU, 1 << fs);
    CHAIN_STAMP(prof, 8 * j + 3);
    // the last slice completes L(j+1, j): R_{j+1} for the strips (every slice was written through and had landed before its count)
    if (threadIdx.x == 0 && ((before >> fs) & 7) == CHAIN_HELPERS - 1) __hip_atomic_store(&sy->R[j + 1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // update: all four slices of L(j+1, j)
    chain_wait2(&sy->SU, fs, 7, CHAIN_HELPERS, nullptr, 0, 0, 0, sy, info);
    CHAIN_STAMP(prof, 8 * j + 4);
    chain_slice_32<false>(Dn + 32 * q, ld, Cn + 32 * q, ld, Cn, ld, sm, prof, 8 * j + 5);
    (void)chain_publish(&sy->SU, 1 << fu);
    CHAIN_STAMP(prof, 8 * j + 7);
    // while the factor role is busy with block (j+1, j+1): column j into the later diagonal blocks
    for (int s = j + 2; s < TPP; ++s) {
      double* Ls = pan + (int64_t)s * NBI + (int64_t)j * NBI * ld;                // L(s, j), solved by diagonal strip s
      chain_wait2(&sy->E[s - 2], 0, 0xffff, j + 1, nullptr, 0, 0, 0, sy, info);
      chain_slice_32<false>(pan + (int64_t)s * NBI + (int64_t)s * NBI * ld + 32 * q, ld, Ls + 32 * q, ld, Ls, ld, sm);
    }
  }
  if (dnext) {
    double* Cn = pan + (int64_t)TPP * NBI + (int64_t)(TPP - 1) * NBI * ld;       // block (4, 3)
    chain_wait2(&sy->W[TPP - 1], 0, 1, 1, &sy->R[0], 0, 1, 1, sy, info);
    CHAIN_STAMP(prof, 24);
    chain_slice_32<true>(Cn + 32 * q, ld, Cn + 32 * q, ld, wp + (int64_t)(TPP - 1) * NBI * NBI, 128, sm, prof, 25);
    const int b0 = chain_publish(&sy->SU, 1);
    CHAIN_STAMP(prof, 27);
    if (threadIdx.x == 0 && (b0 & 7) == CHAIN_HELPERS - 1) __hip_atomic_fetch_add(&sy->LA, 1 << (8 * (TPP - 1)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    chain_wait2(&sy->SU, 0, 7, CHAIN_HELPERS, &sy->SU, 3, 1, 1, sy, info);   // all slices of L(4, 3); tile (0, 0) has its k-chunks 0..2 (bit 3)
    CHAIN_STAMP(prof, 28);
    chain_slice_32<false>(dnext + 32 * q, ldn, Cn + 32 * q, ld, Cn, ld, sm, prof, 29);
    const int b1 = chain_publish(&sy->SU, 1 << 16);
    CHAIN_STAMP(prof, 31);
    if (threadIdx.x == 0 && ((b1 >> 16) & 7) == CHAIN_HELPERS - 1) __hip_atomic_fetch_add(ready_next, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The factor role beside the chain helpers: the four diagonal blocks, each loaded when its update slices are complete.
__device__ __forceinline__ void panel_factor_role_split(double* sm, double* pan, int64_t ld, double* wp, int* info, int p, PanelSync* sy) {
  for (int j = 0; j < TPP; ++j) {
    if (j > 0) chain_wait2(&sy->SU, 16 + 4 * j, 7, CHAIN_HELPERS, nullptr, 0, 0, 0, sy, info);
    CHAIN_STAMP(p == GPRC_CHAIN_PROF_PANEL, 32 + 4 * j);
    potf2_blocked_body<8>(sm, pan + (int64_t)j * NBI + (int64_t)j * NBI * ld, ld, wp + (int64_t)j * NBI * NBI, info, p * NB + j * NBI, nullptr, false);
    CHAIN_STAMP(p == GPRC_CHAIN_PROF_PANEL, 33 + 4 * j);
    panel_flag_publish(&sy->W[j]);
    CHAIN_STAMP(p == GPRC_CHAIN_PROF_PANEL, 34 + 4 * j);
  }
}

// trace (may be null): the factor role's lane 0 leaves s_memrealtime stamps (100 MHz) of its stages there -- measurement only
#define PANEL_STAMP(k) do { if (trace && t == 0) trace[k] = __builtin_amdgcn_s_memrealtime(); } while (0)

// The factor role of one panel: 512 threads (8 waves), sm = PB_SMEM_DOUBLES doubles of LDS.
__device__ __forceinline__ void panel_factor_role(double* sm, double* pan, int64_t ld, double* wp, int* info, int p, PanelSync* sy,
                                                  unsigned long long* trace, unsigned long long* ptrace = nullptr) {
  const int t = threadIdx.x, team = t >> 8, tid = t & 255;
  PANEL_STAMP(0);
  for (int j = 0; j < TPP; ++j) {
    potf2_blocked_body<8>(sm, pan + (int64_t)j * NBI + (int64_t)j * NBI * ld, ld, wp + (int64_t)j * NBI * NBI, info, p * NB + j * NBI,
                          (ptrace && j == 1) ? ptrace : nullptr, j > 0);   // blocks 1..3 arrive in LDS from the update tile below
    PANEL_STAMP(1 + 6 * j);
    panel_flag_publish(&sy->W[j]);               // (its vmcnt(0) + barrier also make L(j,j) / Winv_j visible to this workgroup's own DMA)
    PANEL_STAMP(2 + 6 * j);
    if (j + 1 == TPP) break;
    // the two tiles the next diagonal block is waiting for, by team 0 (team 1 shadows the barriers)
    double* Cn = pan + (int64_t)(j + 1) * NBI + (int64_t)j * NBI * ld;            // block (j+1, j)
    double* Dn = pan + (int64_t)(j + 1) * NBI + (int64_t)(j + 1) * NBI * ld;      // block (j+1, j+1)
    if (j > 0) panel_ready_wait(&sy->E[j + 1], 1, sy, info);                      // block (j+1, j): its update with the columns left of block j
    PANEL_STAMP(3 + 6 * j);
    if (team == 0) gemm_tile_128<true, false, false, false, false, false>(Cn, ld, Cn, ld, wp + (int64_t)j * NBI * NBI, 128, 128, sm, 0, 0, 0, nullptr, tid);
    else gemm_tile_shadow_barriers(128);
    PANEL_STAMP(4 + 6 * j);
    panel_flag_publish(&sy->R[j + 1]);           // rows of strip j+1 left of its diagonal block are final
    PANEL_STAMP(5 + 6 * j);
    if (j > 0) panel_ready_wait(&sy->E[j + 1], 2, sy, info);                      // block (j+1, j+1): likewise
    // the updated block goes to memory (its upper triangle is part of the packed matrix's bits) AND, as potf2's LDS image, straight
    // to the factorisation: no wait for the stores, no reload (5 + 1.5 us per diagonal block)
    if (team == 0) gemm_tile_128<false, false, false, false, true, false>(Dn, ld, Cn, ld, Cn, ld, 128, sm, 0, 0, 0, nullptr, tid, sm);
    else { gemm_tile_shadow_barriers(128); __builtin_amdgcn_s_barrier(); }
    __syncthreads();                             // the image is complete for all 8 waves
    PANEL_STAMP(6 + 6 * j);
  }
}

// The role of strip s (128 rows of the panel) for ONE 4-wave team: tid = thread within the team, smem = the team's
// G_SMEM_DOUBLES of LDS.  s >= TPP: an ordinary strip; s = 2, 3: a diagonal strip (blocks (s, 0..s-2), then the early part of
// blocks (s, s-1) and (s, s), then E_s); s = 0, 1 have nothing to do.  Its workgroup barriers and flag waits are workgroup-wide:
// teams sharing a workgroup must run strips of the same kind.
// progress (may be null; factor service): after every finished block (s, j) of the j loop the workgroup adds `teams` to it behind a
// release.  early (may be null; factor service: the progress counters of the diagonal strips 2 and 3, early[0] / early[1]): an
// ordinary strip then applies the k-chunks 0..j-2 of the update of block (s, j) as soon as L(j, 0..j-2) is final -- long before R_j --
// and only the last chunk (columns of block j-1) after R_j: the same products in the same order, continued through memory.
// progress_shift: the count of block (s, j) goes to the 8-bit field j of *progress (teams << progress_shift j; 0: one plain sum).
__device__ __forceinline__ void panel_strip_role(double* smem, double* pan, int64_t ld, double* wp, int* info, PanelSync* sy, int s, int tid,
                                                 int* progress = nullptr, int teams = 1, int* early = nullptr, int progress_shift = 0, bool relaxed = false,
                                                 bool skip_diag = false, bool hand_last = false, int* early_done = nullptr) {
  if (s < 2) return;
  const double* Arow = pan + (int64_t)s * 128;     // my 128 rows of the panel
  const int jlast = s < TPP ? s - 2 : TPP - 1;     // a diagonal strip solves blocks (s, 0..s-2) itself
  for (int j = 0; j <= jlast; ++j) {
    const int64_t cj = (int64_t)j * NBI;
    double* C = pan + (int64_t)s * 128 + cj * ld;
    __syncthreads();                               // the previous tile's LDS reads are over before this one's first DMA lands
    if (j > 0) {
      if (early && j >= 2) {
        const int64_t ke = (int64_t)(j - 1) * NBI;
        if (early_done) {                                   // split chain: a next-diagonal-block role has applied the early chunks (panel_next_diag_role)
          panel_flag_wait(&early_done[(j - 2) * TPP], sy, info, relaxed);
        } else {
          panel_ready_wait(&early[j - 2], j - 1, sy, info, relaxed);   // L(j, 0..j-2) final
          gemm_tile_128<false, false, false, false, false, false>(C, ld, Arow, ld, pan + cj, ld, (int)ke, smem, 0, 0, 0, nullptr, tid);
        }
        panel_flag_wait(&sy->R[j], sy, info, relaxed);      // (its vmcnt(0) + barrier: the block is reloaded as the next call's C)
        gemm_tile_128<false, false, false, false, false, false>(C, ld, Arow + ke * ld, ld, pan + cj + ke * ld, ld, 128, smem, 0, 0, 0, nullptr, tid);
      } else {
        panel_flag_wait(&sy->R[j], sy, info, relaxed);      // rows of strip j left of its diagonal block are final
        gemm_tile_128<false, false, false, false, false, false>(C, ld, Arow, ld, pan + cj, ld, (int)cj, smem, 0, 0, 0, nullptr, tid);
      }
    }
    if (hand_last && j == TPP - 1) {               // split chain, look-ahead strip TPP: the chain helpers solve this block (R[0]: it is ready for them)
      panel_flag_publish(&sy->R[0]);
      break;
    }
    panel_flag_wait(&sy->W[j], sy, info, relaxed);
    gemm_tile_128<true, false, false, false, false, false>(C, ld, C, ld, wp + (int64_t)j * NBI * NBI, 128, 128, smem, 0, 0, 0, nullptr, tid);
    if (progress) panel_count_publish(progress, teams << (progress_shift * j));
  }
  if (s < TPP) {                                   // diagonal strip: the early part of blocks (s, s-1) and (s, s): K = 128 (s-1)
    const int64_t K = (int64_t)(s - 1) * NBI;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // my own L(s, 0..s-2): every wave's stores, then the barrier
    __syncthreads();
    // block (s, s-1) first: the factor role's solve tile is the next thing on the chain that needs this strip (E_s = 1); block (s, s),
    // which its update tile preloads one tile later, second (E_s = 2).  (The other order -- (s, s) needs my own rows only and can run
    // before R_{s-1} -- left the factor role waiting 13 us for E_3 in every panel.)
    panel_flag_wait(&sy->R[s - 1], sy, info, relaxed);
    gemm_tile_128<false, false, false, false, false, false>(pan + (int64_t)s * 128 + K * ld, ld, Arow, ld, pan + K, ld, (int)K, smem, 0, 0, 0, nullptr, tid);
    panel_count_publish(&sy->E[s], 1);
    if (skip_diag) return;                         // split chain: the chain helpers apply every update of the diagonal blocks themselves
    gemm_tile_128<false, false, false, false, false, false>(pan + (int64_t)s * 128 + (int64_t)s * NBI * ld, ld, Arow, ld, Arow, ld, (int)K, smem, 0, 0, 0, nullptr, tid);
    panel_count_publish(&sy->E[s], 1);
  }
}

__global__ __launch_bounds__(512) void panel_fused_kernel(double* packed, int64_t n_pad, int p, double* winv, int* info, PanelSync* sy,
                                                          unsigned long long* trace, int potf2_trace) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ int sh_id;
  const int t = threadIdx.x;
  if (t == 0) sh_id = atomicAdd(&sy->ticket, 1);
  __syncthreads();
  const int id = sh_id;
  const int64_t ld = panel_ld(n_pad, p);
  double* pan = packed + panel_offset(n_pad, p);
  double* wp = winv + (int64_t)p * TPP * NBI * NBI;
  const int S = (int)(ld / 128);
  const int team = t >> 8, tid = t & 255;
  if (id == 0) {                                   // ---- factor role: the critical chain
    panel_factor_role(sm, pan, ld, wp, info, p, sy, potf2_trace ? nullptr : trace, potf2_trace ? trace : nullptr);
    return;
  }
  int s;
  if (id <= TPP) {                                 // a diagonal strip: one team
    if (team == 1) return;
    s = id - 1;
  } else {
    s = TPP + 2 * (id - TPP - 1) + team;
    if (s >= S) return;                            // odd strip count: the last workgroup runs one team
  }
  panel_strip_role(sm + team * G_SMEM_DOUBLES, pan, ld, wp, info, sy, s, tid);
}

// ------------------------------------------------------------------------------------------------
// The explicit inverse of a panel's NB x NB diagonal block, for the triangular solves with vectors (kernels_vec.hip).
//
// x_p = L_pp^-1 b_p through the four 128-block inverses is a chain of eight dependent small products -- 35 us in one workgroup,
// half of every panel step of a solve.  With inv(L_pp) explicit it is ONE 512 x 512 product, spread over 16 workgroups.
// Stored TRANSPOSED: T = inv(L_pp)^T, column-major with ld = NB, so that row r of the inverse is the NB contiguous doubles at
// T + r NB.  Block row j of T (128-blocks) from the W_i the factorisation leaves in winv:
//   T(j, j) = W_j^T
//   T(j, i) = -( sum_{k = j}^{i-1} T(j, k) L(i, k)^T ) W_i^T        i > j      [inv(i, j) = -W_i sum_k L(i, k) inv(k, j), transposed]
// i.e. per block one accumulating gemm_tile_128 call from a zeroed tile (K = 128 (i - j): the blocks T(j, j..i-1) and L(i, j..i-1)
// are contiguous strips) and one X := X W^T call.  Blocks below the diagonal of T are never written and never read.
// One 4-wave team per block row.  sy != null (factor service): block (j, i) waits for W_i of the panel being factored.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void inv512_row_role(double* smem, const double* pan, int64_t ld, const double* wp, double* T, int j, int tid,
                                                PanelSync* sy, int* info) {
  if (sy) panel_flag_wait(&sy->W[j], sy, info);
  {
    const double* W = wp + (int64_t)j * NBI * NBI;
    double* Tjj = T + (int64_t)j * 128 + (int64_t)j * 128 * NB;
    for (int e = tid; e < 128 * 128; e += 256) Tjj[(e & 127) + (int64_t)(e >> 7) * NB] = W[(e >> 7) + (e & 127) * 128];   // T[c, r] = W[r, c]
  }
  for (int i = j + 1; i < TPP; ++i) {
    double* C = T + (int64_t)j * 128 + (int64_t)i * 128 * NB;
    for (int e = tid; e < 128 * 128; e += 256) C[(e & 127) + (int64_t)(e >> 7) * NB] = 0.0;
    if (sy) panel_flag_wait(&sy->W[i], sy, info);        // (its vmcnt(0) + barrier also settle the stores above for the team's loads)
    else { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __syncthreads(); }
    gemm_tile_128<false, false, false, false, false, false>(C, NB, T + (int64_t)j * 128 + (int64_t)j * 128 * NB, NB, pan + (int64_t)i * 128 + (int64_t)j * 128 * ld, ld, 128 * (i - j), smem,
                         0, 0, 0, nullptr, tid);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    gemm_tile_128<true, false, false, false, false, false>(C, NB, C, NB, wp + (int64_t)i * NBI * NBI, 128, 128, smem, 0, 0, 0, nullptr, tid);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
}

// panels [p0, p0 + gridDim.x / TPP): one workgroup per block row
__global__ __launch_bounds__(256, 2) void inv512_kernel(const double* packed, int64_t n_pad, const double* winv, double* inv, int p0) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int p = p0 + (int)blockIdx.x / TPP, j = (int)blockIdx.x % TPP;
  inv512_row_role(smem, packed + panel_offset(n_pad, p), panel_ld(n_pad, p), winv + (int64_t)p * TPP * NBI * NBI, inv + (int64_t)p * NB * NB, j,
                  (int)threadIdx.x, nullptr, nullptr);
}

// ------------------------------------------------------------------------------------------------
// The factor SERVICE: the whole dependent chain of a factorisation in one persistent launch (one-GPU right-looking sweep,
// n <= 24576).
//
// With one fused launch per panel the chain of panel p + 1 (330 us) starts only when the trailing update of panel p has drained,
// and run beside that update on a second stream its workgroups queue for whole CUs behind the update's GEMM tiles.  Here 21
// workgroups are launched ONCE per factorisation on a side stream and stay resident (21 of 256 CUs); they walk through the panels:
//   role 0        the factor role of the fused kernel (diagonal blocks + the two tiles each next one waits for)
//   roles 1, 2    the diagonal strips 2 and 3 (they also count their finished blocks (s, j <= s-2) into E[0] / E[1])
//   roles 3..6    LOOK-AHEAD strips 4..7: the rows of panel p that are the rows of the NEXT diagonal block; after every finished
//                 block (s, j) they count themselves into LA
//   roles 7..16   the ten lower tiles of the next diagonal block: as soon as the look-ahead strips have finished sub-step j
//                 (field j of LA = 4), D(a, b) -= L(4+a, j) L(4+b, j)^T -- the K = 512 update of that tile in its four k-chunks, in
//                 order, continuing one accumulator chain through memory -- and after chunk 3 they count themselves into
//                 ready[p + 1], on which roles 0..2 start panel p + 1.
//   roles 17..20  (when the caller wants it) the explicit inverse of the panel's diagonal block for the vector solves, one block
//                 row each, paced by the W flags (inv512_row_role) -- off the chain
// (One 4-wave team per CU: two teams sharing a CU ran a K = 128 tile in ~39 us instead of ~20, and those tiles are the path
// between two panels' chains.)  So the distance between two chains is one 128-column solve + one K = 128 tile, with no kernel
// launch, no drained GPU and no contended CU on it.  The caller's stream carries only throughput work, one launch per panel
// (trailing_service_kernel): the trailing update of panel p WITHOUT the next diagonal block, and the ordinary strips (>= 8) of panel
// p + 1, which wait on the service's W / R flags.  That kernel is tied in by counters: its tiles of the next panel's rows 4..7 count
// into ready_la[p + 1] (the look-ahead strips of panel p + 1 wait for 16), its tiles of the diagonal block after the next count into
// ready_d2[p + 2] (roles 7..16 wait for 10 before they add panel p + 1's part: k ascending, as in the launch-per-panel form), and its
// tiles of the next panel's column wait for the last field of LA of panel p (their B operand is the look-ahead strips' result).  Same tiles, same
// k order: bit-identical.
// No deadlock: main-stream kernels of panel p wait only on service flags of panel p; the service waits, for panel p, only on the
// update of panel p - 1, which waits only on service flags of panel p - 1; and nothing that waits on the service is launched before
// the service is resident (service_gate_kernel, the first kernel on the caller's stream).
// ------------------------------------------------------------------------------------------------
constexpr int SERVICE_LA0 = 3;                                   // first look-ahead strip role (one 4-wave team per workgroup)
constexpr int SERVICE_D0 = SERVICE_LA0 + TPP;                    // first next-diagonal-block role (one tile per workgroup)
constexpr int SERVICE_INV0 = SERVICE_D0 + PANEL_DIAG_TILES;     // first explicit-inverse role (one block row of inv(L_pp)^T each)
constexpr int SERVICE_H0 = SERVICE_INV0 + TPP;                   // first chain helper (split chain only; 8 waves each)
constexpr int SERVICE_WGS = SERVICE_H0 + CHAIN_HELPERS;

// One team's share of the next diagonal block: lower tile `idx` (0..9: (0,0) (1,0) (1,1) (2,0) ...) of the block, in four k-chunks.
__device__ __forceinline__ void panel_next_diag_role(double* smem, const double* pan, int64_t ld, double* Dn, int64_t ldn, int* info,
                                                     PanelSync* sy, int idx, int tid, unsigned long long* stamp, bool hand_last = false,
                                                     int* aux = nullptr) {
  int tr, tc;
  diag_tile(idx, tr, tc);
  double* C = Dn + (int64_t)tr * 128 + (int64_t)tc * 128 * ldn;
  // aux (split chain; null otherwise): this role also applies, between its own k-chunks, the EARLY k-chunks of one look-ahead strip's
  // block -- with the chain down to ~200 us a look-ahead strip's ten tiles (~220 us on its one CU) had become the bound
  // (tools/chain_prof.py), while these roles are busy 80 us per panel.  idx 1..4: block (s, 2), s = 3 + idx, chunk 0 after the role's own
  // chunk 0; idx 5..8: block (s, 3), s = idx - 1, chunk 0 there and chunk 1 after the role's chunk 1.  aux[s - TPP] / aux[TPP + s - TPP]
  // = 1: the block has its early chunks (the strip applies the last one).  Same products in the same order, continued through memory.
  const int es = !aux ? -1 : (idx >= 1 && idx <= TPP) ? TPP - 1 + idx : (idx > TPP && idx <= 2 * TPP) ? idx - 1 : -1;   // my look-ahead strip
  const int eb = idx <= TPP ? 2 : 3;                                                                                    // ... and its block
  for (int j = 0; j < TPP; ++j) {
    if (hand_last && j == TPP - 1) {                   // split chain, tile (0, 0): the chain helpers apply the last k-chunk (bit 3 of SU: the tile is ready for them)
      panel_count_publish(&sy->SU, 8);
      break;
    }
    panel_field_wait(&sy->LA, 8 * j, TPP, sy, info);   // all four look-ahead strips have finished sub-step j
    if (stamp && j == TPP - 1 && threadIdx.x == 0) *stamp = __builtin_amdgcn_s_memrealtime();
    gemm_tile_128<false, false, false, false, false, false>(C, ldn, pan + (int64_t)(TPP + tr) * 128 + (int64_t)j * NBI * ld, ld, pan + (int64_t)(TPP + tc) * 128 + (int64_t)j * NBI * ld, ld,
                         128, smem, 0, 0, 0, nullptr, tid);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the tile is reloaded as the next chunk's C
    __syncthreads();
    if (es >= 0 && j <= eb - 2) {                      // L(es, j) is final (LA field j); L(eb, j): the diagonal strip eb's progress
      panel_ready_wait(&sy->E[eb - 2], j + 1, sy, info);
      double* Ce = const_cast<double*>(pan) + (int64_t)es * 128 + (int64_t)eb * NBI * ld;
      gemm_tile_128<false, false, false, false, false, false>(Ce, ld, pan + (int64_t)es * 128 + (int64_t)j * NBI * ld, ld, pan + (int64_t)eb * NBI + (int64_t)j * NBI * ld, ld,
                           128, smem, 0, 0, 0, nullptr, tid);
      if (j == eb - 2) panel_flag_publish(&aux[(eb - 2) * TPP + es - TPP]);
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
  }
}

// ready: three counters per panel -- ready[p]: lower tiles of diagonal block p complete (10); ready[P + p]: tiles of panel p's rows
// [NB, 2 NB) that have received panel p - 1 (16); ready[2 P + p]: lower tiles of diagonal block p that have received panel p - 2 (10)
// trace (may be null; GPRC_SERVICE_TRACE): 16 s_memrealtime stamps per panel, see gprc_prof_service_trace -- measurement only
#define SERVICE_STAMP(p, k) do { if (trace && (threadIdx.x & 255) == 0) trace[16 * (p) + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)

// The launch serves the panels [p_begin, p_end) -- a group of the grouped left-looking schedule, or all of them: its first panel is
// complete when the launch starts; the next diagonal block is updated only inside the group (the panel behind the group receives
// everything in its left-looking pass, k ascending), the look-ahead strips are solved for every panel that has rows below it.
__global__ __launch_bounds__(512) void panel_service_kernel(double* packed, int64_t n_pad, double* winv, int* info, PanelSync* sy_base,
                                                            int* ready, int P, unsigned long long* trace, double* inv, int p_begin, int p_end,
                                                            int split, int part) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int t = threadIdx.x, team = t >> 8, tid = t & 255;
  if (t == 0) __hip_atomic_fetch_add(&ready[3 * P], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // resident: see service_gate_kernel
  // (Putting the factor role and its four helpers behind ONE L2 -- a grid of 8 x 5 with the five of them on workgroups 0, 8, 16, 24, 32,
  //  the dealing to XCDs being round robin -- was measured and is SLOWER: n = 8192 5.43 -> 5.67 ms, 16384 27.3 -> 27.5; the other twenty
  //  roles then crowd four XCDs and the look-ahead strips fall 70 us behind.  profiles/r03_chain_split.txt.)
  // part 0: the whole service in one launch (role = workgroup).  SHARED service (service_shared): two launches -- part 1 the factor role and
  // the chain helpers (8 waves each: a CU of their own), part 2 the twenty 4-wave roles with only a GEMM team's LDS, so that ONE workgroup of
  // the sweep kernel fits beside each of them and has the CU's matrix cores while the role waits for its flags.
  const int role = part == 0 ? (int)blockIdx.x : part == 1 ? (blockIdx.x == 0 ? 0 : SERVICE_H0 + (int)blockIdx.x - 1) : 1 + (int)blockIdx.x;
  if (part == 2) __builtin_amdgcn_s_setprio(3);   // beside throughput work on the same SIMDs: the role's instructions go first
#ifdef GPRC_CHAIN_PROF
  if (t == 0 && (role == 0 || role >= SERVICE_H0)) g_chain_prof[56 + (role == 0 ? 0 : 1 + role - SERVICE_H0)] = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 15;
#endif
  if (role >= SERVICE_H0) { if (!split) return; }    // the chain helpers: all 8 waves
  else if (role >= 1 && team == 1) return;           // every other role but the factor role is one 4-wave team
  if (role >= SERVICE_INV0 && role < SERVICE_H0 && !inv) return;
  for (int p = p_begin; p < p_end; ++p) {
    PanelSync* sy = sy_base + p;
    const int64_t ld = panel_ld(n_pad, p);
    double* pan = packed + panel_offset(n_pad, p);
    double* wp = winv + (int64_t)p * TPP * NBI * NBI;
    const bool hand = split && p + 1 < p_end;        // the path W_3 -> next chain goes through the chain helpers
    // aux[p][2 TPP]: flags "block (TPP + i, 2) / (TPP + i, 3) of panel p has its early k-chunks", behind the sweep kernel's flags in the sync block
    int* aux = ready + 3 * P + 16 + 2 * P * TPP * P + 8 * P + P * TPP * P * TPP + (int64_t)p * AUX_STRIDE;
    if (role <= 2) {
      if (role == 0) SERVICE_STAMP(p, 14);
      if (p > p_begin) {
        if (role == 0 && split) chain_wait2(&sy_base[p - 1].SU, 16, 7, CHAIN_HELPERS, nullptr, 0, 0, 0, sy, info);   // tile (0, 0) is all the first potf2 reads
        else panel_ready_wait(&ready[p], PANEL_DIAG_TILES, sy, info);
      }
      if (role == 0) SERVICE_STAMP(p, 0);
      if (role == 0) {
        if (split) panel_factor_role_split(sm, pan, ld, wp, info, p, sy);
        else panel_factor_role(sm, pan, ld, wp, info, p, sy, nullptr);
      } else panel_strip_role(sm, pan, ld, wp, info, sy, role + 1, tid, &sy->E[role - 1], 1, nullptr, 0, false, split != 0);
      if (role == 0) SERVICE_STAMP(p, 1);
    } else if (role >= SERVICE_H0) {
      panel_chain_helper_role(sm, pan, ld, wp, info, sy, role - SERVICE_H0, role == SERVICE_H0 && p == GPRC_CHAIN_PROF_PANEL,   // paced by this panel's W flags
                              hand ? packed + panel_offset(n_pad, p + 1) : nullptr, hand ? panel_ld(n_pad, p + 1) : 0, &ready[p + 1],
                              p > p_begin ? &ready[p] : nullptr);
    } else if (role >= SERVICE_INV0) {
      inv512_row_role(sm, pan, ld, wp, inv + (int64_t)p * NB * NB, role - SERVICE_INV0, tid, sy, info);
    } else if (role < SERVICE_D0 ? p + 1 < P : p + 1 < p_end) {
      if (role < SERVICE_D0) {
        if (p > p_begin) panel_ready_wait(&ready[P + p], PANEL_LA_TILES, sy, info);
        if (role == SERVICE_LA0) SERVICE_STAMP(p, 2);
        panel_strip_role(sm, pan, ld, wp, info, sy, TPP + (role - SERVICE_LA0), tid, &sy->LA, 1, sy->E, 8, false, false, hand && role == SERVICE_LA0,
                         hand ? aux + (role - SERVICE_LA0) : nullptr);
        if (role == SERVICE_LA0) SERVICE_STAMP(p, 3);
      } else {
        if (p > p_begin) panel_ready_wait(&ready[2 * P + p + 1], PANEL_DIAG_TILES, sy, info);
        if (role == SERVICE_D0) SERVICE_STAMP(p, 4);
        panel_next_diag_role(sm, pan, ld, packed + panel_offset(n_pad, p + 1), panel_ld(n_pad, p + 1), info, sy, role - SERVICE_D0, tid,
                             (role == SERVICE_D0 && trace) ? trace + 16 * p + 5 : nullptr, hand && role == SERVICE_D0, hand ? aux : nullptr);
        if (!(hand && role == SERVICE_D0)) panel_count_publish(&ready[p + 1], 1);
        if (role == SERVICE_INV0 - 1) SERVICE_STAMP(p, 6);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                               // LDS and this panel's stores are settled before the next panel's first DMA
  }
}

// First kernel of the caller's stream: one wave that returns once every service workgroup is resident.  Whatever waits on the
// service is ordered behind it, so a GPU full of waiting workgroups can never keep the service out.
// (Not a bounded_wait either: one wave, nobody to hand over to -- no fence, no barrier, no PanelSync.)
// limit_ticks: patience in s_memrealtime ticks (WAIT_LIMIT_TICKS; the test hook GPRC_TEST_SERVICE_TIMEOUT, launch_service_gate's `forced`, passes 0 with an
// unreachable `need`: the gate gives up at its first look, every wait behind it returns at once, info = GPRC_INFO_WAIT_TIMEOUT).
__global__ void service_gate_kernel(int* alive, int need, int* info, unsigned long long limit_ticks) {
  if (threadIdx.x == 0) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__hip_atomic_load(alive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < need) {
      if (__builtin_amdgcn_s_memrealtime() - t0 >= limit_ticks) {
        wait_diag(6, need, __hip_atomic_load(alive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), alive, nullptr);
        atomicExch(info, GPRC_INFO_WAIT_TIMEOUT);
        break;
      }
      __builtin_amdgcn_s_sleep(8);
    }
  }
}

// the ordinary strips (s >= 8) of panel p, one 4-wave workgroup each, waiting on the service's flags
__global__ __launch_bounds__(256, 2) void panel_strips_kernel(double* packed, int64_t n_pad, int p, double* winv, int* info, PanelSync* sy,
                                                              unsigned long long* trace) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int64_t ld = panel_ld(n_pad, p);
  if (blockIdx.x == 0) SERVICE_STAMP(p, 7);
  panel_strip_role(smem, packed + panel_offset(n_pad, p), ld, winv + (int64_t)p * TPP * NBI * NBI, info, sy, 2 * TPP + (int)blockIdx.x, (int)threadIdx.x,
                   nullptr, 1, sy->E);
  if (blockIdx.x == 0) SERVICE_STAMP(p, 8);
}

// The caller's-stream kernel of panel p under the factor service: the trailing update of panel p -- every lower tile of the panels
// behind p EXCEPT the next diagonal block (the service's roles 5..9 own it) -- AND the ordinary strips of panel p + 1, which so run
// beside the bulk of the update instead of as a phase of their own (190 us per panel with the GPU two thirds empty).
// Roles are dealt by a ticket counter in START order:
//   tickets [0, n_first)                    the tiles of panel p + 1's own column, rows [NB, 2 NB) first: those 16 count into
//                                           ready_la (the service's look-ahead strips of panel p + 1 wait for them), the others into
//                                           rowcnt[their 128-row strip]; all of them first wait until the look-ahead strips of
//                                           panel p are final (sy->LA >= TPP << 24: their B operand)
//   tickets [n_first, n_first + nstrips)    strip 8 + i of panel p + 1: waits for its four tiles (rowcnt = 4), then the strip role on
//                                           the service's W / R flags of panel p + 1
//   the rest                                all other tiles (XCD-contiguous ranges), the diagonal block of panel p + 2 first (-> ready_d2)
// A strip workgroup can only be running when every ticket before it has started, so the tiles it waits for are running or done,
// and those wait only on the service: no deadlock whatever the dispatch order.
// q_end: the targets are the panels (p, q_end) -- the rest of the group.
__global__ __launch_bounds__(256, 2) void trailing_service_kernel(double* packed, int64_t n_pad, int p, int ntiles, int nstrips, PanelSync* sy_base,
                                                                  int* ready, int* rowcnt, double* winv, int* info, unsigned long long* trace, int q_end) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ int sh_ticket;
  const int P = (int)(n_pad / NB);
  constexpr int DIAG = PANEL_DIAG_TILES;
  PanelSync* sy = sy_base + p;
  const int T0 = panel_tiles(P, p + 1);   // tiles of panel p + 1 (>= DIAG + LAT: there are >= 2 targets)
  const int n_first = T0 - DIAG;
  // Only the first `base` workgroups (the waiting roles and what they wait for) take tickets; the rest map block id -> tile directly,
  // so that block id mod 8 -- the XCD -- still selects a contiguous range of tiles (ticket order would scatter an XCD's tiles and
  // with them the operand strips its L2 serves: measured -12 % on the update).
  const int base = (n_first + nstrips + 7) & ~7;
  int t;
  if ((int)blockIdx.x < base) {
    if (threadIdx.x == 0) sh_ticket = atomicAdd(&sy->ticket, 1);
    __syncthreads();
    t = sh_ticket;
    if (t >= n_first + nstrips) return;
  } else {
    t = n_first + nstrips + ((int)blockIdx.x - base);
  }
  if (t == 0) SERVICE_STAMP(p, 9);
  int s, local;                                                     // target index behind p + 1, tile index in that panel's list
  bool sig_d2 = false;
  if (t < n_first) { s = 0; local = DIAG + t; }
  else if (t < n_first + nstrips) {                                 // ---- an ordinary strip of panel p + 1
    const int q = p + 1, strip = 2 * TPP + (t - n_first);
    if (strip == 2 * TPP) SERVICE_STAMP(q, 7);
    panel_ready_wait(&rowcnt[(int64_t)q * TPP * P + strip], TPP, sy_base + q, info);
    panel_strip_role(smem, packed + panel_offset(n_pad, q), panel_ld(n_pad, q), winv + (int64_t)q * TPP * NBI * NBI, info, sy_base + q, strip, (int)threadIdx.x,
                     nullptr, 1, sy_base[q].E);
    if (strip == 2 * TPP) SERVICE_STAMP(q, 8);
    return;
  } else {
    const int nrest = ntiles - n_first;
    int id = (int)xcd_remap((unsigned)(t - n_first - nstrips), (unsigned)nrest);
    if (id == nrest - 1) SERVICE_STAMP(p, 13);
    const int T1 = T0 - TPP * TPP;
    if (id < DIAG) { s = 1; local = id; sig_d2 = true; }
    else if (id < T1) { s = 1; local = id; }
    else {
      id -= T1;
      s = 2;
      for (;; ++s) {
        if (p + 1 + s >= q_end) return;
        const int tq = panel_tiles(P, p + 1 + s);
        if (id < tq) break;
        id -= tq;
      }
      local = id;
    }
  }
  const int q = p + 1 + s;
  int tr, tc;
  panel_tile(local, tr, tc);
  if (s == 0) panel_ready_wait(&sy->LA, TPP << (8 * (TPP - 1)), sy, info);
  if (t == 0) SERVICE_STAMP(p, 10);
  const int64_t ldp = panel_ld(n_pad, p), ldq = panel_ld(n_pad, q);
  const double* Lp = packed + panel_offset(n_pad, p) + (int64_t)(q - p) * NB;  // row q*NB of panel p
  double* Cq = packed + panel_offset(n_pad, q);
  gemm_tile_128<false, false, false, false, false, true, 1>(Cq + (int64_t)tr * 128 + (int64_t)tc * 128 * ldq, ldq, Lp + (int64_t)tr * 128, ldp, Lp + (int64_t)tc * 128, ldp, NB, smem);
  if (s == 0) panel_count_publish(tr < 2 * TPP ? &ready[P + q] : &rowcnt[(int64_t)q * TPP * P + tr], 1);
  else if (sig_d2) panel_count_publish(&ready[2 * P + q], 1);
  if (t == 0) SERVICE_STAMP(p, 11);
  if (sig_d2 && local == 0) SERVICE_STAMP(p, 12);
}


// ------------------------------------------------------------------------------------------------
// The caller's-stream work of a whole GROUP of panels under the factor service in ONE persistent launch (round 3).
//
// One trailing_service_kernel per panel leaves the GPU partly empty at every launch boundary: the last generation of a launch's
// tiles is only partly filled (at n = 8192 the updates have 3.9, 3.4, 2.9 ... generations of ~470 co-resident tiles: 25 generations
// are paid for 20.6), the next launch cannot start one tile before the last one of this launch has finished, and an in-order stream
// has no way to let them overlap (hipExtAnyOrderLaunch is not honoured on gfx950: tools/microbench/anyorder.hip).  Here the same
// work items -- panel p's tiles of panel p + 1's column, the ordinary strips of panel p + 1, every other tile of panel p's update,
// p = p_begin .. p_last - 1 -- are dealt to 2 x (CUs - service workgroups) persistent workgroups by ticket counters, and what the
// kernel boundary used to order is carried by three kinds of flags:
//   ver[q][tr][tc]        number of the group's panels tile (tr, tc) of panel q has received: the update with panel p waits for
//                         p - p_begin and leaves p - p_begin + 1 (the same k order as the launch-per-panel form: identical bits);
//   stripdone[p][strip]   the ordinary strip (>= 2 TPP) of panel p is final -- an operand of panel p's update (the strips of the
//                         group's first panel ran in a launch of their own in front of this kernel);
//   the service's counters and flags as before (LA of panel p for the tiles of panel p + 1's column, rowcnt / ready_la / ready_d2).
// Order of the tickets: panel by panel; inside a panel the `head` (the column of panel p + 1, then that panel's strips: one counter,
// sy[p].ticket) before the `rest`, which is split into eight contiguous ranges with a counter each -- a workgroup takes from the
// range of ITS XCD (HW_REG_XCC_ID) so that an XCD's L2 keeps serving neighbouring tiles' operand strips, and from the other ranges
// only when its own is used up.  A workgroup looks at panel p + 1 only when every ticket of panel p has been taken.
// No deadlock: a workgroup holding a ticket waits only for tickets that come earlier in this order -- all of them taken by
// workgroups that are running -- or for the service, which is resident (service_gate_kernel) and itself waits only for such tickets.
// Every wait is bounded in wall time; after a timeout (info = GPRC_INFO_WAIT_TIMEOUT) every workgroup leaves at its next look.
// ------------------------------------------------------------------------------------------------
#ifdef GPRC_SWEEP_PROF
__device__ unsigned long long g_sweep_prof[8];   // ticks (100 MHz) summed over workgroups: take, wait, gemm, publish, strip; [5] tiles, [6] strips, [7] kernel
#define SWEEP_T(var) const unsigned long long var = __builtin_amdgcn_s_memrealtime()
#define SWEEP_ADD(k, a, b) do { if (threadIdx.x == 0) atomicAdd(&g_sweep_prof[k], (b) - (a)); } while (0)
#else
#define SWEEP_T(var)
#define SWEEP_ADD(k, a, b)
#endif
struct SweepSync {          // views into the sync block behind PanelSync[P], ready[3 P + 16] and rowcnt[P TPP P]
  int* stripdone;           // [P][TPP P]
  int* rest_ticket;         // [P][8]
  int* ver;                 // [P][TPP P][TPP]
  int* aux;                 // [P][AUX_STRIDE]: from 2 TPP on, the finished 32-row slices of the head tiles of the update INTO panel q (sweep_slice_32)
};

// The sync block of a factorisation under the service (zeroed by the caller, stream-ordered before the first launch), carved in ONE place:
//   sy[P]                   the flags of every panel
//   ready[3 P]              ready, ready_la, ready_d2 (P ints each)
//   resident[16]            the service's "resident" counter (and padding)
//   rowcnt[P][TPP P]        per panel, per 128-row strip, the tiles of that strip which have received the previous panel
//   sw                      the persistent sweep's flags (trailing_sweep_kernel): stripdone[P][TPP P], rest_ticket[P][8], ver[P][TPP P][TPP],
//                           aux[P][AUX_STRIDE]  (panel_service_kernel reaches aux from `ready`: the same sums)
struct SyncView {
  PanelSync* sy;
  int *ready, *resident, *rowcnt;
  SweepSync sw;
  size_t bytes;
  SyncView(void* sync, int64_t P) : sy(static_cast<PanelSync*>(sync)), bytes((size_t)P * sizeof(PanelSync)) {
    auto carve = [&](int64_t ints) {
      int* at = reinterpret_cast<int*>(reinterpret_cast<uintptr_t>(sync) + bytes);
      bytes += (size_t)ints * sizeof(int);
      return at;
    };
    ready = carve(3 * P);
    resident = carve(16);
    rowcnt = carve(P * TPP * P);
    sw.stripdone = carve(P * TPP * P);
    sw.rest_ticket = carve(8 * P);
    sw.ver = carve(P * TPP * P * TPP);
    sw.aux = carve(P * AUX_STRIDE);
  }
};

// a ticket of counter ctr, or `limit` when it is used up (one lane; one device-scope round trip -- a counter past its limit is harmless)
__device__ __forceinline__ int sweep_take(int* ctr, int limit) {
  const int t = __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return t < limit ? t : limit;
}

// waits until *a >= va, *b >= vb, *c >= vc (null pointers are skipped; the three polls fly together), then one acquire for all.
// false: somebody's wait has timed out (info = GPRC_INFO_WAIT_TIMEOUT) -- the caller leaves.
// (Not a bounded_wait: its checks come at the first miss and every 64th, and it hands a result to the whole workgroup through sh_dead.)
__device__ __forceinline__ bool sweep_wait3(int* a, int va, int* b, int vb, int* c, int vc, int* failed, int* info, int* sh_dead) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (threadIdx.x == 0) {
    int spins = 0;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    for (;;) {
      const int xa = a ? __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : va;
      const int xb = b ? __hip_atomic_load(b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : vb;
      const int xc = c ? __hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : vc;
      if (xa >= va && xb >= vb && xc >= vc) break;
      relaxed_pause();
      if ((++spins & 63) != 1) continue;              // at the first miss and every 64th from there
      if (__hip_atomic_load(info, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == GPRC_INFO_WAIT_TIMEOUT) {
        if (xa < va) wait_diag(15, va, xa, a, failed - 1); else if (xb < vb) wait_diag(15, vb, xb, b, failed - 1); else wait_diag(15, vc, xc, c, failed - 1);
        *sh_dead = 1;
        break;
      }
      if (__builtin_amdgcn_s_memrealtime() - t0 > WAIT_LIMIT_TICKS) {   // bounded in wall time (see bounded_wait)
        if (xa < va) wait_diag(5, va, xa, a, failed - 1); else if (xb < vb) wait_diag(5, vb, xb, b, failed - 1); else wait_diag(5, vc, xc, c, failed - 1);
        __hip_atomic_store(failed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        atomicExch(info, GPRC_INFO_WAIT_TIMEOUT);
        *sh_dead = 1;
        break;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  return *sh_dead == 0;
}

// the item is complete: its flag (a version or a strip's "done"), and (may be null) one count for the service / the strips
// written_through: every byte of the item was stored sc1 (gemm_tile_128<.., WT>): nothing of it is dirty in L2, no write-back needed
// (the microarchitecture guide's form "sc1 payload -> every wave's vmcnt(0) -> barrier -> sc1 flag"; the consumers acquire as always)
__device__ __forceinline__ void sweep_publish(int* flag, int value, int* ctr, bool written_through = false) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    if (!written_through) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ctr) __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// 32 rows x 128 columns of C -= A B^T over K columns (a multiple of 128) on ONE 4-wave workgroup: chain_slice_32's scheme (the A rows of a
// 128-column chunk through LDS, each wave's B rows straight into registers, write-through stores), wave w the columns [32 w, 32 w + 32).
// Every element: acc = C, then the k-steps ascending with the negate-A bit -- gemm_tile_128's arithmetic, identical bits.
__device__ __forceinline__ void sweep_slice_32(double* C_, int64_t ldc, const double* A_, int64_t lda, const double* B_, int64_t ldb, int K, double* lds_) {
  typedef __attribute__((address_space(1))) double gdouble;
  typedef __attribute__((address_space(3))) double ldouble;
  gdouble* C = (gdouble*)C_;
  const gdouble* A = (const gdouble*)A_;
  const gdouble* B = (const gdouble*)B_;
  ldouble* lds = (ldouble*)lds_;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int fk = lane >> 4, fr = lane & 15;
  double4_t acc[2][2];
  gdouble* Cw = C + fr + (int64_t)(32 * wave + fk) * ldc;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[m][n][r] = Cw[16 * m + (int64_t)(16 * n + 4 * r) * ldc];
  for (int k0 = 0; k0 < K; k0 += 128) {
    const gdouble* asrc = A + 16 * (t & 1) + (int64_t)(k0 + (t >> 1)) * lda;   // thread t: rows [16 (t & 1), +16) of k-slice t >> 1
    double av[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) av[i] = asrc[i];
    const gdouble* bsrc = B + (32 * wave + fr) + (int64_t)(k0 + fk) * ldb;
    double b0[32], b1[32];
#pragma unroll
    for (int s = 0; s < 32; ++s) { b0[s] = bsrc[(int64_t)(4 * s) * ldb]; b1[s] = bsrc[16 + (int64_t)(4 * s) * ldb]; }
    __syncthreads();                                   // the previous chunk's LDS reads are over
    ldouble* adst = lds + (t >> 1) * CHAIN_LDS_LD + 16 * (t & 1);
#pragma unroll
    for (int i = 0; i < 16; ++i) adst[i] = av[i];
    __syncthreads();
    const ldouble* ap = lds + fk * CHAIN_LDS_LD + fr;
#pragma unroll
    for (int s = 0; s < 32; ++s) {
      const double a0 = ap[4 * s * CHAIN_LDS_LD], a1 = ap[4 * s * CHAIN_LDS_LD + 16];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(b0[s], a0, acc[0][0], 0, 0, 1);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(b0[s], a1, acc[1][0], 0, 0, 1);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(b1[s], a0, acc[0][1], 0, 0, 1);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(b1[s], a1, acc[1][1], 0, 0, 1);
    }
  }
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) __hip_atomic_store(&Cw[16 * m + (int64_t)(16 * n + 4 * r) * ldc], acc[m][n][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct SweepItem { int kind, p, s, local, strip, flags; };   // kind 0: tile (s, local) of panel p's update; 1: strip of panel p + 1; 2: rows [32 strip, +32) of head tile `local`; -1: nothing left
constexpr int SWEEP_SIG_D2 = 1, SWEEP_FIRST = 2, SWEEP_LAST = 4;

// One lane's view of the ticket order (see the kernel): which panel it is at, which counter, and that panel's item counts.
struct SweepCursor {
  int p, phase;                                    // phase 0: head; 1 + k: the rest range of XCD (xcc + k) & 7
  int n_first, nstrips, nrest, T1;
  __device__ void enter(int p_, int P, int64_t n_pad, int q_end) {
    p = p_; phase = 0;
    constexpr int DIAG = PANEL_DIAG_TILES;
    const int T0 = panel_tiles(P, p + 1);                           // lower tiles of panel p + 1
    n_first = T0 - DIAG;                                            // ... without its diagonal block (the service's)
    const int ld1 = (int)(panel_ld(n_pad, p + 1) / 128);
    nstrips = ld1 > 2 * TPP ? ld1 - 2 * TPP : 0;
    int ntiles = -DIAG;
    for (int q = p + 1; q < q_end; ++q) ntiles += panel_tiles(P, q);
    nrest = ntiles - n_first;
    T1 = T0 - TPP * TPP;                                            // lower tiles of panel p + 2
  }
};

// panels p in [p_begin, p_last): the update of panel p over the targets (p, q_end) (without the next diagonal block) and the
// ordinary strips of panel p + 1.  The caller makes sure p_last - 1 still has something to do (p_last + 1 < P, p_last < q_end).
// CORE: the tile loop of gemm_tile_128 -- 1 (first interleaved loop) where two sweep workgroups share a CU, 2 (no VALU instruction in the
// loop) where ONE workgroup has the CU (n_pad < 10752): there the faster tile pays (n = 8192 5.47 -> 5.27 ms); beside a second workgroup
// it costs 5-8 % (12288 13.4 -> 14.3, 16384 26.6 -> 27.5, 32768 171.6 -> 173.7; same box, profiles/r03_chain_split.txt).
template <int CORE>
__global__ __launch_bounds__(256, 2) void trailing_sweep_kernel(double* packed, int64_t n_pad, int p_begin, int p_last, int q_end, PanelSync* sy_base,
                                                                int* ready, int* rowcnt, SweepSync sw, double* winv, int* info,
                                                                unsigned long long* trace, int head_slices) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ SweepItem sh_item;
  __shared__ int sh_dead;
  if (threadIdx.x == 0) sh_dead = 0;
  const int P = (int)(n_pad / NB);
  constexpr int DIAG = PANEL_DIAG_TILES;
  const int xcc = (int)(__builtin_amdgcn_s_getreg((3 << 11) | 20) & 7);   // HW_REG_XCC_ID[3:0]: speed only (which L2 this CU sits behind)
  SWEEP_T(tkern0);

  // The next item in ticket order (lane 0; one device-scope atomic in the steady state).  Taking it AHEAD of time -- while the
  // current tile's stores drain -- was measured slower at every size (n = 8192 6.66 against 6.36 ms, 16384 27.75 against 27.52):
  // a ticket then sits behind its holder's publish while somebody may already be waiting for it.
  SweepCursor cur;
  cur.enter(p_begin, P, n_pad, q_end);
  auto find_next = [&](SweepItem& it) {
    it.kind = -1; it.flags = 0; it.s = 0; it.local = 0; it.strip = 0;
    while (cur.p < p_last) {
      it.p = cur.p;
      if (cur.phase == 0) {
        // (CORE == 2, one workgroup per CU: the chain is the bound, and the first 16 head tiles -- the next panel's rows [NB, 2 NB), which
        //  release that panel's look-ahead strips -- are dealt in four 32-row slices each: 64 items of ~25 us instead of 16 tiles of ~100)
        const int extra = (CORE == 2 && head_slices && cur.n_first >= PANEL_LA_TILES) ? 3 * PANEL_LA_TILES : 0;
        const int lim = cur.n_first + cur.nstrips + extra;
        int t = sweep_take(&sy_base[cur.p].ticket, lim);
        if (t >= lim) { cur.phase = 1; continue; }
        if (t == 0) it.flags |= SWEEP_FIRST;
        if (extra && t < 4 * PANEL_LA_TILES) { it.kind = 2; it.local = DIAG + (t >> 2); it.strip = t & 3; return; }
        t -= extra;
        if (t < cur.n_first) { it.kind = 0; it.local = DIAG + t; }
        else { it.kind = 1; it.strip = 2 * TPP + (t - cur.n_first); }
        return;
      }
      if (cur.phase <= 8) {
        const int x = (xcc + cur.phase - 1) & 7;
        const int rq = cur.nrest >> 3, rr = cur.nrest & 7;
        const int cnt = rq + (x < rr ? 1 : 0);
        const int start = x < rr ? x * (rq + 1) : rr * (rq + 1) + (x - rr) * rq;
        const int i = cnt > 0 ? sweep_take(sw.rest_ticket + (int64_t)cur.p * 8 + x, cnt) : cnt;
        if (i >= cnt) { ++cur.phase; continue; }
        int id = start + i;
        if (id == cur.nrest - 1) it.flags |= SWEEP_LAST;
        if (id < cur.T1) { it.kind = 0; it.s = 1; it.local = id; if (id < DIAG) it.flags |= SWEEP_SIG_D2; return; }
        id -= cur.T1;
        int s = 2;
        for (; cur.p + 1 + s < q_end; ++s) {
          const int tq = panel_tiles(P, cur.p + 1 + s);
          if (id < tq) break;
          id -= tq;
        }
        if (cur.p + 1 + s < q_end) { it.kind = 0; it.s = s; it.local = id; return; }
        continue;
      }
      if (cur.p + 1 < p_last) cur.enter(cur.p + 1, P, n_pad, q_end);   // every ticket of this panel has been taken
      else cur.p = p_last;
    }
  };

  SweepItem nxt;
  for (;;) {
    SWEEP_T(tk0);
    if (threadIdx.x == 0) find_next(nxt);
    __syncthreads();                                  // every wave has left the previous item (its LDS, its view of sh_item)
    if (threadIdx.x == 0) sh_item = nxt;
    __syncthreads();
    const SweepItem it = sh_item;
    SWEEP_T(tk1);
    SWEEP_ADD(0, tk0, tk1);
    if (it.kind < 0) break;
    const int p = it.p;
    PanelSync* sy = sy_base + p;
    if (it.flags & SWEEP_FIRST) SERVICE_STAMP(p, 9);
    if (it.flags & SWEEP_LAST) SERVICE_STAMP(p, 13);
    if (it.kind == 0 || it.kind == 2) {
      // ---- one tile of the update with panel p: target q = p + 1 + s, tile (tr, tc) of that panel (kind 2: 32 rows of it)
      const int q = p + 1 + it.s, local = it.local;
      int tr, tc;
      panel_tile(local, tr, tc);
      const int stage = p - p_begin;                                // versions the tiles of this panel's update wait for
      const int ra = (q - p) * TPP + tr, rb = (q - p) * TPP + tc;   // the operands' 128-row strips of panel p
      int* verp = sw.ver + ((int64_t)q * TPP * P + tr) * TPP + tc;
      // strips TPP .. 2 TPP - 1 are the service's look-ahead strips (LA >= TPP << 24 when all four are final); the others ride in this
      // kernel, except those of the group's first panel, which ran in a launch of their own in front of it
      int* sd_p = sw.stripdone + (int64_t)p * TPP * P;
      int* wa = ra >= 2 * TPP ? (stage > 0 ? sd_p + ra : nullptr) : &sy->LA;
      int* wb = rb >= 2 * TPP ? (stage > 0 ? sd_p + rb : nullptr) : &sy->LA;
      if (wb == wa) wb = nullptr;
      SWEEP_T(tw0);
      constexpr int LA_FINAL = TPP << (8 * (TPP - 1));
      if (!sweep_wait3(stage > 0 ? verp : nullptr, stage, wa, wa == &sy->LA ? LA_FINAL : 1, wb, wb == &sy->LA ? LA_FINAL : 1, &sy->failed, info, &sh_dead)) break;
      SWEEP_T(tw1);
      const int64_t ldp = panel_ld(n_pad, p), ldq = panel_ld(n_pad, q);
      const double* Lp = packed + panel_offset(n_pad, p) + (int64_t)(q - p) * NB;   // row q NB of panel p
      double* Cq = packed + panel_offset(n_pad, q);
      // (CORE = 1: see the loops' comments.  WT: the tile is stored write-through, so that its publication needs no write-back of the XCD's
      //  L2 -- a release fence per tile, by ~60 workgroups per XCD, each flushing what all of them have dirtied since the last one, was
      //  2 % of the mid-size factorisation: n = 16384 27.42 -> 26.84 ms, 8192 5.98 -> 5.81, same box)
      if constexpr (CORE == 2) if (it.kind == 2) {
        sweep_slice_32(Cq + (int64_t)tr * 128 + (int64_t)tc * 128 * ldq + 32 * it.strip, ldq, Lp + (int64_t)tr * 128 + 32 * it.strip, ldp, Lp + (int64_t)tc * 128, ldp, NB, smem);
        // the slice is stored (write-through): count it; the fourth one publishes the tile as a whole tile's holder would
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0 &&
            (__hip_atomic_fetch_add(sw.aux + (int64_t)q * AUX_STRIDE + 2 * TPP + (local - DIAG), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 3) == 3) {
          __hip_atomic_store(verp, stage + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_fetch_add(&ready[P + q], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        SWEEP_ADD(5, 0ull, 1ull);
        if (it.flags & SWEEP_FIRST) SERVICE_STAMP(p, 11);
        continue;
      }
      gemm_tile_128<false, false, false, false, false, true, CORE, true>(Cq + (int64_t)tr * 128 + (int64_t)tc * 128 * ldq, ldq, Lp + (int64_t)tr * 128, ldp, Lp + (int64_t)tc * 128, ldp, NB, smem);
      SWEEP_T(tw2);
      int* ctr = nullptr;
      if (it.s == 0) ctr = tr < 2 * TPP ? &ready[P + q] : &rowcnt[(int64_t)q * TPP * P + tr];
      else if (it.flags & SWEEP_SIG_D2) ctr = &ready[2 * P + q];
      sweep_publish(verp, stage + 1, ctr, true);
      SWEEP_T(tw3);
      SWEEP_ADD(1, tw0, tw1); SWEEP_ADD(2, tw1, tw2); SWEEP_ADD(3, tw2, tw3); SWEEP_ADD(5, 0ull, 1ull);
      if (it.flags & SWEEP_FIRST) SERVICE_STAMP(p, 11);
    } else {
      // ---- an ordinary strip of panel p + 1: its four tiles of this update first, then the strip role on the service's flags
      const int q = p + 1, strip = it.strip;
      if (strip == 2 * TPP) SERVICE_STAMP(q, 7);
      if (!sweep_wait3(&rowcnt[(int64_t)q * TPP * P + strip], TPP, nullptr, 0, nullptr, 0, &sy_base[q].failed, info, &sh_dead)) break;
      panel_strip_role(smem, packed + panel_offset(n_pad, q), panel_ld(n_pad, q), winv + (int64_t)q * TPP * NBI * NBI, info, sy_base + q, strip, (int)threadIdx.x,
                       nullptr, 1, sy_base[q].E, 0, true);
      sweep_publish(sw.stripdone + (int64_t)q * TPP * P + strip, 1, nullptr);
      SWEEP_T(ts1);
      SWEEP_ADD(4, tk1, ts1); SWEEP_ADD(6, 0ull, 1ull);
      if (strip == 2 * TPP) SERVICE_STAMP(q, 8);
    }
  }
  SWEEP_T(tkern1);
  SWEEP_ADD(7, tkern0, tkern1);
}

}  // namespace

int launch_potf2_inv(hipStream_t s, double* A, int64_t lda, double* winv, int* info_dev, int col0) {
  ProfScope ps(s, PK_POTF2, 128.0 * 128 * 128 / 3 * 2, 8.0 * 3 * 128 * 128);
  GPRC_TRY(ensure_dynamic_lds<potf2_inv_blocked_kernel>(PB_SMEM_BYTES));
  hipLaunchKernelGGL(potf2_inv_blocked_kernel, dim3(1), dim3(1024), PB_SMEM_BYTES, s, A, lda, winv, info_dev, col0);
  GPRC_LAUNCH_CHECK();
  return 0;
}

// trace: 0 none; 1 the factor role stamps its stages (24 x 8 bytes at sync16 + 64 .. sync16 + 256; read back with gprc_prof_panel_trace);
// 2 the stamps are those of the SECOND diagonal block's potf2 instead.  Measurement only.
int launch_panel_fused(hipStream_t s, double* packed, int64_t n_pad, int64_t p, double* winv, int* info_dev, void* sync16, int trace) {
  static_assert(PB_SMEM_DOUBLES >= 2 * G_SMEM_DOUBLES, "two GEMM teams must fit beside each other in the factor role's LDS");
  GPRC_TRY(ensure_dynamic_lds<panel_fused_kernel>(PB_SMEM_BYTES));
  const int64_t ld = panel_ld(n_pad, p), S = ld / 128;
  const unsigned grid = (unsigned)(1 + TPP + (S - TPP + 1) / 2);
  GPRC_HIP(hipMemsetAsync(sync16, 0, sizeof(PanelSync), s));
  // algorithmic work of a whole panel factorisation: in-panel updates + panel solves + the four diagonal blocks
  double fl = 0.0;
  for (int j = 0; j < TPP; ++j) fl += 2.0 * (double)(ld - j * NBI) * NBI * (j * NBI) + (double)(ld - (j + 1) * NBI) * NBI * NBI + 2.0 * NBI * NBI * NBI / 3.0;
  ProfScope ps(s, PK_PANEL_FUSED, fl, 8.0 * 2.0 * (double)ld * NB);
  unsigned long long* stamps = trace ? reinterpret_cast<unsigned long long*>(static_cast<char*>(sync16) + 64) : nullptr;
  hipLaunchKernelGGL(panel_fused_kernel, dim3(grid), dim3(512), PB_SMEM_BYTES, s, packed, n_pad, (int)p, winv, info_dev, reinterpret_cast<PanelSync*>(sync16), stamps,
                     trace == 2 ? 1 : 0);
  GPRC_LAUNCH_CHECK();
  return 0;
}

size_t panel_service_sync_bytes(int64_t P) { return SyncView(nullptr, P).bytes; }

int launch_inv512(hipStream_t s, const double* packed, int64_t n_pad, const double* winv, double* inv, int64_t p_begin, int64_t p_end) {
  if (p_end <= p_begin) return 0;
  GPRC_TRY(ensure_dynamic_lds<inv512_kernel>(G_SMEM_BYTES));
  hipLaunchKernelGGL(inv512_kernel, dim3((unsigned)((p_end - p_begin) * TPP)), dim3(256), G_SMEM_BYTES, s, packed, n_pad, winv, inv, (int)p_begin);
  GPRC_LAUNCH_CHECK();
  return 0;
}

// two contexts may time out together: the records' copy-and-clear is one step (here and in gprc_prof_wait_timeout)
static std::mutex g_wait_diag_host;
static const int g_wait_diag_zero[8 * (WAIT_DIAG_RECORDS + 1)] = {};

// the records the timed-out waits left (wait_diag), as text for the host's error message; clears them
std::string wait_timeout_report() {
  int v[8 * (WAIT_DIAG_RECORDS + 1)];
  {
    std::lock_guard<std::mutex> lock(g_wait_diag_host);
    if (hipMemcpyFromSymbol(v, HIP_SYMBOL(g_wait_diag), sizeof(v)) != hipSuccess || v[0] == 0) return "";
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_wait_diag), g_wait_diag_zero, sizeof(g_wait_diag_zero));
  }
  static const char* const site[] = {"?", "flag", "count", "field", "chain", "sweep", "gate"};
  std::string out = " [waits that gave up (+10: still waiting when somebody else had):";
  const int n = v[0] < WAIT_DIAG_RECORDS ? v[0] : WAIT_DIAG_RECORDS;
  for (int k = 0; k < n && k < 8; ++k) {
    const int* r = v + 8 * (k + 1);
    const int st = r[0] % 10;
    out += std::string(k ? ";" : "") + " " + site[st >= 0 && st <= 6 ? st : 0] + (r[0] >= 10 ? "+10" : "") + " wait of workgroup " + std::to_string(r[1]) + "/" +
           std::to_string(r[2]) + "x" + std::to_string(r[6]) + " needed " + std::to_string(r[3]) + " saw " + std::to_string(r[4]) + " word " + std::to_string(r[5]);
  }
  return out + (v[0] > 8 ? "; ... " + std::to_string(v[0]) + " in all]" : "]");
}

// split: with the chain helpers (four more resident workgroups); part: 0 the whole service; 1 / 2 the two launches of the shared service
// (on two streams: they run side by side)
int launch_panel_service(hipStream_t s, double* packed, int64_t n_pad, double* winv, int* info_dev, void* sync, void* trace, double* inv,
                         int64_t p_begin, int64_t p_end, bool split, int part) {
  GPRC_TRY(ensure_dynamic_lds<panel_service_kernel>(PB_SMEM_BYTES));
  const int64_t P = n_pad / NB;
  const SyncView v(sync, P);
  ProfScope ps(s, PK_PANEL_FUSED, 0.0, 0.0);
  const unsigned grid = part == 0 ? SERVICE_WGS : part == 1 ? 1 + CHAIN_HELPERS : SERVICE_H0 - 1;
  hipLaunchKernelGGL(panel_service_kernel, dim3(grid), dim3(512), part == 2 ? G_SMEM_BYTES : PB_SMEM_BYTES, s, packed, n_pad, winv, info_dev, v.sy,
                     v.ready, (int)P, static_cast<unsigned long long*>(trace), inv, (int)p_begin, (int)p_end, split ? 1 : 0, part);
  GPRC_LAUNCH_CHECK();
  return 0;
}

// launches: service launches so far on this sync buffer, this one included (the "resident" counter is cumulative)
// forced (the test hook GPRC_TEST_SERVICE_TIMEOUT): the gate waits for a residency count that cannot be reached and gives up at once
int launch_service_gate(hipStream_t s, int64_t n_pad, int* info_dev, void* sync, int launches, bool forced) {
  hipLaunchKernelGGL(service_gate_kernel, dim3(1), dim3(64), 0, s, SyncView(sync, n_pad / NB).resident, forced ? (1 << 30) : SERVICE_WGS * launches, info_dev,
                     forced ? 0ULL : WAIT_LIMIT_TICKS);
  GPRC_LAUNCH_CHECK();
  return 0;
}

// the ordinary strips of panel p (rows from 2 NB below the panel's top)
int launch_panel_strips(hipStream_t s, double* packed, int64_t n_pad, int64_t p, double* winv, int* info_dev, void* sync, void* trace) {
  const int64_t ld = panel_ld(n_pad, p), S = ld / 128;
  if (S <= 2 * TPP) return 0;
  GPRC_TRY(ensure_dynamic_lds<panel_strips_kernel>(G_SMEM_BYTES));
  double fl = 0.0;
  for (int j = 0; j < TPP; ++j) fl += 2.0 * (double)(ld - 2 * NB) * NBI * (j * NBI) + (double)(ld - 2 * NB) * NBI * NBI;
  ProfScope ps(s, PK_GEMM_INNER, fl, 8.0 * 2.0 * (double)(ld - 2 * NB) * NB);
  hipLaunchKernelGGL(panel_strips_kernel, dim3((unsigned)(S - 2 * TPP)), dim3(256), G_SMEM_BYTES, s, packed, n_pad, (int)p, winv,
                     info_dev, SyncView(sync, n_pad / NB).sy + p, static_cast<unsigned long long*>(trace));
  GPRC_LAUNCH_CHECK();
  return 0;
}

// ordinary strips (rows from 2 NB below the top) of panel q, and the flops of their strip roles riding in an update kernel
static int64_t ordinary_strips(int64_t n_pad, int64_t q) { return std::max<int64_t>(0, panel_ld(n_pad, q) / 128 - 2 * TPP); }
static void add_strip_flops(int64_t nstrips, double& fl) {
  for (int j = 0; j < TPP; ++j) fl += nstrips * (2.0 * 128 * NBI * (j * NBI) + 128.0 * NBI * NBI);
}

// the caller's-stream kernel of panel p under the service: the trailing update of panel p over the targets (p, q_end) (everything
// except the next diagonal block) + the ordinary strips of panel p + 1
int launch_trailing_service(hipStream_t s, double* packed, int64_t n_pad, int64_t p, double* winv, int* info_dev, void* sync, void* trace, int64_t q_end) {
  const int64_t P = n_pad / NB;
  if (q_end > P) q_end = P;
  if (q_end - p - 1 < 1 || p + 2 >= P) return 0;   // no target, or the only target is the last panel: its diagonal block is all there is
  GPRC_TRY(ensure_dynamic_lds<trailing_service_kernel>(G_SMEM_BYTES));
  int64_t tiles = -(int64_t)PANEL_DIAG_TILES;
  for (int64_t q = p + 1; q < q_end; ++q) tiles += panel_tiles(P, q);
  double fl = 0.0, by = 0.0;
  trailing_work(n_pad, p + 1, q_end, 1, NB, true, fl, by);
  const int64_t nstrips = ordinary_strips(n_pad, p + 1);
  add_strip_flops(nstrips, fl);
  ProfScope ps(s, PK_TRAILING, fl, by);
  const SyncView v(sync, P);
  const int64_t n_first = panel_tiles(P, p + 1) - PANEL_DIAG_TILES;
  const int64_t base = (n_first + nstrips + 7) & ~(int64_t)7;     // ticketed workgroups, padded to a multiple of the XCD count
  hipLaunchKernelGGL(trailing_service_kernel, dim3((unsigned)(base + (tiles - n_first))), dim3(256), G_SMEM_BYTES, s, packed, n_pad, (int)p,
                     (int)tiles, (int)nstrips, v.sy, v.ready, v.rowcnt, winv, info_dev, static_cast<unsigned long long*>(trace), (int)q_end);
  GPRC_LAUNCH_CHECK();
  return 0;
}

// the caller's-stream work of the panels [g0, g1) of a group under the service in ONE persistent launch (trailing_sweep_kernel) of wgs
// workgroups; core: the kernel's tile loop (1 or 2, see the kernel); head_slices (core 2 only): the head tiles in 32-row slices
int launch_trailing_sweep(hipStream_t s, double* packed, int64_t n_pad, int64_t g0, int64_t g1, double* winv, int* info_dev, void* sync, void* trace,
                          int wgs, int core, int head_slices) {
  const int64_t P = n_pad / NB;
  const int64_t q_end = std::min(g1, P);
  int64_t p_last = g0;                                              // one past the last panel with something to do (launch_trailing_service's rule)
  for (int64_t p = g0; p + 1 < g1; ++p)
    if (!(q_end - p - 1 < 1 || p + 2 >= P)) p_last = p + 1;
  if (p_last == g0) return 0;
  GPRC_TRY(core == 2 ? ensure_dynamic_lds<trailing_sweep_kernel<2>>(G_SMEM_BYTES) : ensure_dynamic_lds<trailing_sweep_kernel<1>>(G_SMEM_BYTES));
  double fl = 0.0, by = 0.0;
  for (int64_t p = g0; p < p_last; ++p) {
    trailing_work(n_pad, p + 1, q_end, 1, NB, true, fl, by);
    add_strip_flops(ordinary_strips(n_pad, p + 1), fl);
  }
  ProfScope ps(s, PK_TRAILING, fl, by);
  const SyncView v(sync, P);
  if (core == 2)
    hipLaunchKernelGGL(trailing_sweep_kernel<2>, dim3((unsigned)wgs), dim3(256), G_SMEM_BYTES, s, packed, n_pad, (int)g0, (int)p_last,
                       (int)q_end, v.sy, v.ready, v.rowcnt, v.sw, winv, info_dev, static_cast<unsigned long long*>(trace), head_slices);
  else
    hipLaunchKernelGGL(trailing_sweep_kernel<1>, dim3((unsigned)wgs), dim3(256), G_SMEM_BYTES, s, packed, n_pad, (int)g0, (int)p_last,
                       (int)q_end, v.sy, v.ready, v.rowcnt, v.sw, winv, info_dev, static_cast<unsigned long long*>(trace), 0);
  GPRC_LAUNCH_CHECK();
  return 0;
}

}  // namespace gprc

// include/gprc_native.h: the raw records of the timed-out waits, see wait_diag; clears them
extern "C" __attribute__((visibility("default"))) int gprc_prof_wait_timeout(int* out, int ints) {   // out[0]: records written; 8 ints per record from out[8]
  if (!out || ints < 8) return -1;
  const size_t bytes = sizeof(int) * (size_t)std::min(ints, 8 * (gprc::WAIT_DIAG_RECORDS + 1));
  std::lock_guard<std::mutex> lock(gprc::g_wait_diag_host);
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(gprc::g_wait_diag), bytes) != hipSuccess) return -1;
  return hipMemcpyToSymbol(HIP_SYMBOL(gprc::g_wait_diag), gprc::g_wait_diag_zero, sizeof(gprc::g_wait_diag_zero)) == hipSuccess ? 0 : -1;
}
#ifdef GPRC_CHAIN_PROF
extern "C" __attribute__((visibility("default"))) int gprc_debug_chain_prof(unsigned long long* out64) {
  return hipMemcpyFromSymbol(out64, HIP_SYMBOL(gprc::g_chain_prof), 512) == hipSuccess ? 0 : -1;
}
#endif
#ifdef GPRC_SWEEP_PROF
extern "C" __attribute__((visibility("default"))) int gprc_debug_sweep_prof(unsigned long long* out8, int reset) {
  if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(gprc::g_sweep_prof), 64) != hipSuccess) return -1;
  if (reset) { unsigned long long z[8] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(gprc::g_sweep_prof), z, 64) != hipSuccess) return -1; }
  return 0;
}
#endif
