// kernels_knn.hip -- exact brute-force k-nearest-neighbours in float64 ("Local GPR"): for every query point the m
// candidates with the smallest key (dist2, index), lexicographic, in ascending key order, and the gather that turns the indices into the
// strided slabs of the batched small-model fit.
//
//   dist2(j, i) = sum_c ((xs_jc - x_ic) s_c)^2,   c ascending, acc = fma(t, t, acc) from 0,   t = (xs_jc - x_ic) * s_c   (s_c = 1: t = the difference)
//
// The difference is taken first: a query that coincides with a candidate has distance exactly 0.  The sum of one pair is one chain of
// fused multiply-adds in one order wherever the pair is evaluated, and the selection compares whole keys exactly, so indices and
// distance bits are a function of (X, Xs, scale, m) alone: not of the number of queries, the tile or the split a pair falls into.
//
// Layout.  A workgroup of KNN_WAVES waves owns KNN_WG_Q queries, KNN_Q per wave, and walks its range of candidates in tiles of KNN_TC,
// staged once in LDS (coordinate-major, KNN_DC coordinates at a time; a wider point takes several chunks, the partial sums stay in
// registers) and read by every wave.  A lane evaluates KNN_A candidates of the tile against the wave's KNN_Q queries.  Each query's
// result is a sorted list of 128 (dist2, index) pairs in registers, two per lane: rank r lives in lane r % 64 of slot r / 64.  The
// wave-uniform threshold, the list's entry of rank m - 1, rejects almost every candidate with one compare; the survivors of a step are
// found with a ballot and inserted one at a time: the insertion point is the number of smaller entries (two ballots), the tail moves up
// by one lane.  About m ln(n / m) insertions a query, beside n / (64 KNN_A) steps.
//
// For few queries the candidates are split over blockIdx.y; every part writes its sorted list to a workspace and knn_merge_kernel runs
// the same insertion over the parts' entries, on the same key.  No atomics, no waiting between workgroups.
// A candidate whose distance is not finite-or-smaller (NaN) is never selected; a rank that stays empty (fewer than m comparable
// candidates) reports index -1 and distance +inf, which the gather turns into NaN points.
#include <algorithm>
#include <limits>

#include "gprc_internal.h"

namespace gprc {
namespace {

constexpr int KNN_WAVES = 8;
constexpr int KNN_Q = 4;                        // queries per wave
constexpr int KNN_WG_Q = KNN_WAVES * KNN_Q;     // queries per workgroup
constexpr int KNN_A = 2;                        // candidates per lane and tile
constexpr int KNN_TC = 64 * KNN_A;              // candidates per tile
constexpr int KNN_DC = 16;                      // coordinates per staged chunk
constexpr int KNN_LDC = KNN_TC + 2;             // pitch of a coordinate's row of the tile (doubles)
constexpr int KNN_THREADS = 64 * KNN_WAVES;
static_assert(KNN_THREADS % KNN_TC == 0 && KNN_THREADS / KNN_WG_Q >= KNN_DC, "the staging of a chunk: whole candidates per pass, every query coordinate in one");

__device__ __forceinline__ bool key_less(double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); }

// one query's sorted list, two ranks per lane, and its threshold
struct KnnList {
  double d0, d1, thr_d;
  int i0, i1, thr_i;
};

__device__ __forceinline__ void list_init(KnnList& L) {
  L.d0 = L.d1 = L.thr_d = __builtin_huge_val();
  L.i0 = L.i1 = L.thr_i = -1;        // (+inf, -1): no candidate's key is equal, every finite distance is smaller
}

template <bool BIG>   // BIG: m > 64, the second slot is in use
__device__ __forceinline__ void list_insert(KnnList& L, int lane, int m, double nd, int ni) {
  int pos = __popcll(__ballot(key_less(L.d0, L.i0, nd, ni)));
  if (BIG) pos += __popcll(__ballot(key_less(L.d1, L.i1, nd, ni)));
  const double up_d = __shfl_up(L.d0, 1);
  const int up_i = __shfl_up(L.i0, 1);
  if (BIG) {
    const double carry_d = __shfl(L.d0, 63);
    const int carry_i = __shfl(L.i0, 63);
    double u_d = __shfl_up(L.d1, 1);
    int u_i = __shfl_up(L.i1, 1);
    if (lane == 0) { u_d = carry_d; u_i = carry_i; }
    const int p1 = pos - 64;
    if (lane > p1) { L.d1 = u_d; L.i1 = u_i; }
    else if (lane == p1) { L.d1 = nd; L.i1 = ni; }
  }
  if (lane > pos) { L.d0 = up_d; L.i0 = up_i; }
  else if (lane == pos) { L.d0 = nd; L.i0 = ni; }
  const int last = m - 1;
  if (BIG && last >= 64) { L.thr_d = __shfl(L.d1, last - 64); L.thr_i = __shfl(L.i1, last - 64); }
  else { L.thr_d = __shfl(L.d0, last); L.thr_i = __shfl(L.i0, last); }
}

// one candidate per lane (dist, idx; a lane without one passes +inf): whatever beats the threshold goes into the list.  The first test is
// one compare and one branch for the whole wave; the full key is looked at only when some lane's distance reaches the threshold's.
template <bool BIG>
__device__ __forceinline__ void list_consider(KnnList& L, int lane, int m, double dist, int idx) {
  if (__ballot(dist <= L.thr_d) == 0) return;
  unsigned long long mask = __ballot(key_less(dist, idx, L.thr_d, L.thr_i));
  while (mask) {
    const int src = __ffsll((long long)mask) - 1;
    list_insert<BIG>(L, lane, m, __shfl(dist, src), __shfl(idx, src));
    mask &= mask - 1;
    mask &= __ballot(key_less(dist, idx, L.thr_d, L.thr_i));   // the threshold has moved
  }
}

// rank r < m of the list to dist[r], idx[r] (dist may be null)
__device__ __forceinline__ void list_store(const KnnList& L, int lane, int m, int* idx, double* dist) {
  if (lane < m) { idx[lane] = L.i0; if (dist) dist[lane] = L.d0; }
  if (64 + lane < m) { idx[64 + lane] = L.i1; if (dist) dist[64 + lane] = L.d1; }
}

struct KnnArgs {
  const double* X;        // d x n, point-major
  const double* Xs;       // d x ns, point-major
  const double* scale;    // d doubles (SCALED only)
  int* idx;               // parts == 1: query j's at idx + j ld;  else the workspace: part p's at idx + (p ns + j) m
  double* dist;           // likewise; may be null when parts == 1
  int64_t d, n, ns, ld, part_len;   // part p takes the candidates [p part_len, min(n, (p + 1) part_len)), part_len a multiple of KNN_TC
  int m, parts;
  int64_t q_first;        // BEFORE only: query j is column q_first + j of X itself (Xs = X + q_first d)
};

// BEFORE (gprc_dev_knn_before, the conditioning sets of the Vecchia likelihood): the queries are columns of X and a candidate is eligible
// iff its index is below its query's.  An ineligible lane passes +inf, like a lane without a candidate, and a workgroup's tile loop ends
// at its largest query index: about half the pair work.  Ranks that no candidate fills keep the list's initial (+inf, -1).
template <bool SCALED, bool BIG, bool BEFORE = false>
__global__ __launch_bounds__(KNN_THREADS) void knn_kernel(const KnnArgs a) {
  __shared__ double cand[KNN_DC * KNN_LDC];
  __shared__ double qry[KNN_DC * KNN_WG_Q];     // [c][query of the workgroup]
  __shared__ double scl[KNN_DC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q0 = (int64_t)blockIdx.x * KNN_WG_Q;
  const int part = blockIdx.y;
  const int64_t i_begin = (int64_t)part * a.part_len;
  const int64_t i_end = i_begin + a.part_len < a.n ? i_begin + a.part_len : a.n;
  const int64_t d = a.d;
  KnnList L[KNN_Q];
#pragma unroll
  for (int q = 0; q < KNN_Q; ++q) list_init(L[q]);
  int64_t t_end = i_end;
  if constexpr (BEFORE) {   // the largest query index of the workgroup: no candidate from there on is eligible for any of its queries
    const int64_t q_last = a.q_first + (q0 + KNN_WG_Q < a.ns ? q0 + KNN_WG_Q : a.ns) - 1;
    if (q_last < t_end) t_end = q_last;
  }

  for (int64_t t0 = i_begin; t0 < t_end; t0 += KNN_TC) {
    double acc[KNN_A][KNN_Q];
#pragma unroll
    for (int s = 0; s < KNN_A; ++s)
#pragma unroll
      for (int q = 0; q < KNN_Q; ++q) acc[s][q] = 0.0;
    for (int64_t c0 = 0; c0 < d; c0 += KNN_DC) {
      const int dc = (int)(d - c0 < KNN_DC ? d - c0 : KNN_DC);
      __syncthreads();   // the previous chunk has been read
      {   // a thread stages one candidate's coordinates c = tid / KNN_TC, + KNN_THREADS / KNN_TC, ... and one coordinate of one query
        const int i = tid % KNN_TC;
        const int64_t gi = t0 + i;
        for (int c = tid / KNN_TC; c < dc; c += KNN_THREADS / KNN_TC) cand[c * KNN_LDC + i] = gi < i_end ? a.X[gi * d + c0 + c] : 0.0;
        const int q = tid % KNN_WG_Q, cq = tid / KNN_WG_Q;
        const int64_t gq = q0 + q;
        if (cq < dc) qry[cq * KNN_WG_Q + q] = gq < a.ns ? a.Xs[gq * d + c0 + cq] : 0.0;
      }
      if (SCALED && tid < dc) scl[tid] = a.scale[c0 + tid];
      __syncthreads();
#pragma unroll 4
      for (int c = 0; c < dc; ++c) {
        double xq[KNN_Q];
#pragma unroll
        for (int q = 0; q < KNN_Q; ++q) xq[q] = qry[c * KNN_WG_Q + wave * KNN_Q + q];
        const double sc = SCALED ? scl[c] : 1.0;
#pragma unroll
        for (int s = 0; s < KNN_A; ++s) {
          const double xc = cand[c * KNN_LDC + s * 64 + lane];
#pragma unroll
          for (int q = 0; q < KNN_Q; ++q) {
            double t = xq[q] - xc;
            if (SCALED) t *= sc;
            acc[s][q] = __builtin_fma(t, t, acc[s][q]);
          }
        }
      }
    }
#pragma unroll
    for (int s = 0; s < KNN_A; ++s) {
      const int64_t gi = t0 + s * 64 + lane;
      const bool in = gi < i_end;
#pragma unroll
      for (int q = 0; q < KNN_Q; ++q) {
        bool eligible = in;
        if constexpr (BEFORE) eligible = in && gi < a.q_first + q0 + wave * KNN_Q + q;
        list_consider<BIG>(L[q], lane, a.m, eligible ? acc[s][q] : __builtin_huge_val(), (int)gi);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < KNN_Q; ++q) {
    const int64_t gq = q0 + wave * KNN_Q + q;
    if (gq < a.ns) {
      const int64_t off = a.parts == 1 ? gq * a.ld : ((int64_t)part * a.ns + gq) * a.m;
      list_store(L[q], lane, a.m, a.idx + off, a.dist ? a.dist + off : nullptr);
    }
  }
}

struct KnnMergeArgs {
  const int* pidx;        // the parts' lists: part p's of query j at (p ns + j) m
  const double* pdist;
  int* idx;               // query j's at idx + j ld
  double* dist;           // may be null
  int64_t ns, ld;
  int m, parts;
};

// one wave a query: the parts' entries, 64 at a time, through the same insertion
template <bool BIG>
__global__ __launch_bounds__(256) void knn_merge_kernel(const KnnMergeArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= a.ns) return;   // a whole wave leaves: no barrier follows
  KnnList L;
  list_init(L);
  for (int p = 0; p < a.parts; ++p) {
    const int64_t off = ((int64_t)p * a.ns + j) * a.m;
    for (int r0 = 0; r0 < a.m; r0 += 64) {
      const bool in = r0 + lane < a.m;
      const int ci = in ? a.pidx[off + r0 + lane] : -1;
      const double cd = in ? a.pdist[off + r0 + lane] : __builtin_huge_val();
      list_consider<BIG>(L, lane, a.m, ci >= 0 ? cd : __builtin_huge_val(), ci);
    }
  }
  list_store(L, lane, a.m, a.idx + j * a.ld, a.dist ? a.dist + j * a.ld : nullptr);
}

struct GatherArgs {
  const int* idx;     // query j's m neighbours at idx + j ld
  const double* X;    // d x n
  const double* y;    // n
  double* Xg;         // model j's points at Xg + j d m, point-major
  double* yg;         // model j's targets at yg + j m
  int64_t d, ns, ld, m;
};

__global__ __launch_bounds__(256) void knn_gather_kernel(const GatherArgs a) {
  const int64_t total = a.ns * a.m;
  const double qnan = __builtin_nan("");
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = e / a.m, r = e - j * a.m;
    const int i = a.idx[j * a.ld + r];
    double* dst = a.Xg + e * a.d;
    if (i >= 0) {
      const double* src = a.X + (int64_t)i * a.d;
      for (int64_t c = 0; c < a.d; ++c) dst[c] = src[c];
      a.yg[e] = a.y[i];
    } else {
      for (int64_t c = 0; c < a.d; ++c) dst[c] = qnan;
      a.yg[e] = qnan;
    }
  }
}

}  // namespace

void knn_split(int64_t n, int64_t ns, int cus, int* parts, int64_t* part_len) {
  const int64_t groups = (ns + KNN_WG_Q - 1) / KNN_WG_Q;
  const int64_t tiles = (n + KNN_TC - 1) / KNN_TC;
  int64_t p = 1;
  if (groups < 2 * (int64_t)cus) {
    p = (2 * (int64_t)cus + groups - 1) / groups;
    const int64_t most = (tiles + 15) / 16;            // a part is at least 16 tiles: 2048 candidates
    if (p > most) p = most;
    if (p > 1024) p = 1024;
    if (p < 1) p = 1;
  }
  const int64_t tiles_each = (tiles + p - 1) / p;
  *part_len = tiles_each * KNN_TC;
  *parts = (int)((tiles + tiles_each - 1) / tiles_each);
}

size_t knn_workspace_doubles(int64_t ns, int m, int parts) {
  if (parts <= 1) return 0;
  const size_t entries = (size_t)parts * (size_t)ns * (size_t)m;
  return entries + (entries + 1) / 2;   // the distances, then the indices
}

namespace {

template <bool BEFORE>
int launch_knn_any(hipStream_t s, const double* X, int64_t d, int64_t n, const double* Xs, int64_t ns, int64_t q_first, const double* scale, int m, int* idx,
                   double* dist, int64_t ld, int parts, int64_t part_len, double* work) {
  if (ns <= 0) return 0;
  const int64_t groups = (ns + KNN_WG_Q - 1) / KNN_WG_Q;
  const bool split = parts > 1;
  const size_t entries = (size_t)parts * (size_t)ns * (size_t)m;
  double* wdist = split ? work : dist;
  int* widx = split ? reinterpret_cast<int*>(work + entries) : idx;
  KnnArgs a{X, Xs, scale, widx, wdist, d, n, ns, ld, part_len, m, parts, q_first};
  const dim3 grid((unsigned)groups, (unsigned)parts), block(KNN_THREADS);
  const bool big = m > 64;
  if (scale) {
    if (big) hipLaunchKernelGGL((knn_kernel<true, true, BEFORE>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((knn_kernel<true, false, BEFORE>), grid, block, 0, s, a);
  } else {
    if (big) hipLaunchKernelGGL((knn_kernel<false, true, BEFORE>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((knn_kernel<false, false, BEFORE>), grid, block, 0, s, a);
  }
  GPRC_LAUNCH_CHECK();
  if (split) {
    KnnMergeArgs g{widx, wdist, idx, dist, ns, ld, m, parts};
    const dim3 mgrid((unsigned)((ns + 3) / 4)), mblock(256);
    if (big) hipLaunchKernelGGL((knn_merge_kernel<true>), mgrid, mblock, 0, s, g);
    else hipLaunchKernelGGL((knn_merge_kernel<false>), mgrid, mblock, 0, s, g);
    GPRC_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace

int launch_knn(hipStream_t s, const double* X, int64_t d, int64_t n, const double* Xs, int64_t ns, const double* scale, int m, int* idx, double* dist,
               int64_t ld, int parts, int64_t part_len, double* work) {
  return launch_knn_any<false>(s, X, d, n, Xs, ns, 0, scale, m, idx, dist, ld, parts, part_len, work);
}

int launch_knn_before(hipStream_t s, const double* X, int64_t d, int64_t first, int64_t count, const double* scale, int m, int* idx, double* dist, int64_t ld,
                      int parts, int64_t part_len, double* work) {
  return launch_knn_any<true>(s, X, d, first + count, X + first * d, count, first, scale, m, idx, dist, ld, parts, part_len, work);
}

int launch_knn_gather(hipStream_t s, const int* idx, int64_t ld, const double* X, const double* y, int64_t d, int64_t ns, int64_t m, double* Xg, double* yg) {
  if (ns <= 0) return 0;
  GatherArgs a{idx, X, y, Xg, yg, d, ns, ld, m};
  const int64_t blocks = std::min<int64_t>((ns * m + 255) / 256, 8192);
  hipLaunchKernelGGL(knn_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
  GPRC_LAUNCH_CHECK();
  return 0;
}

}  // namespace gprc
