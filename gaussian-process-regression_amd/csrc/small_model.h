// small_model.h -- the core of the small-model family for gfx950 (MI355X): the kernels that run ONE MODEL OF AT MOST 128 POINTS PER
// WORKGROUP, in LDS ("Small models in batches").  Shared by kernels_batch.hip (evidence and gradient),
// kernels_batch_gpc.hip (the Laplace mode search), kernels_batch_predict.hip (the spec load alone: its arithmetic is its own),
// and kernels_vecchia.hip (the conditionals; its factorisation and solves are its own).
//
// What is here, each piece once, with the order of summation the kernels' head comments promise:
//   sqdist         the squared distance of two points: coordinates ascending, one fma chain, ARD through bt_scaled_diff;
//   load_spec      a model's parameter record into the KernelSpec the workgroup keeps in LDS, and SPEC_DOUBLES, the room it takes;
//   image_entry    the per-entry rule of the image handed to the factorisation: zero above the diagonal, the identity from n on, the
//                  pair's kernel value plus the noise on the diagonal;
//   winv_forward, winv_transposed    the two triangular solves as products with the explicit inverse potf2_blocked_body leaves above
//                  the diagonal of its image (chol_tile.h: pb_wdiag, pb_w): thread (row, q), q < 4, a stride-4 fma chain, the four
//                  parts as (q0 + q1) + (q2 + q3), last fma(W_rr, rhs_r, .); the q == 0 thread of a row hands the finished value to the
//                  caller's epilogue (batch stores alpha, the classifier forms b - sw o v);
//   sum128         entry t to thread t < 128; each of the two waves by wave_sum; the caller adds wave 0 + wave 1 behind its barrier;
//   LOG_2PI.
// What a pair adds to the theta sums (theta_terms) sits beside cross_weight in pair_tile.h, because kernels_igrad.hip shares it too.
//
// What is deliberately NOT shared:
//   * kernels_batch_predict.hip's sqdist4: four chains interleaved, one coordinate load for four pairs -- another shape, for registers.
//   * the fill loops.  The batch kernels decompose the entry index with & 127 and >> 7, Vecchia divides by the model's own run-time extent;
//     one loop would put a division into the batch kernel.  kernels_batch_gpc.hip's gc_image is image_entry's sibling with another
//     entry formula (I + sw K sw from the slab, no kernel value) and stays where it is.
//   * the finish of the theta sums over the waves.  Batch adds eight waves into gacc and stores from there, Vecchia adds four, stores
//     straight to `out` and puts NaN for a flagged point, and their ARD passes walk the pairs differently (registers against the image):
//     a shared form with the wave count, the store and the flag as parameters is longer than the two originals together.
//   * kernels_batch_loo.hip's 1/2 log 2 pi.  Its literal 0.91893853320467274178 is the double 0x1.d67f1c864beb5p-1; half of LOG_2PI
//     below is 0x1.d67f1c864beb4p-1, one ulp less.  One constant for both would move the bits of the evidence or of the LOO score.
//   * kernels_sgrad.hip's `pair` lambda: the same weight also feeds its dz sums, so the branch cannot be cut at the theta terms.
#pragma once
#include "chol_tile.h"
#include "pair_tile.h"

namespace gprc {

namespace {

constexpr int SPEC_DOUBLES = (sizeof(KernelSpec) + 7) / 8;   // a KernelSpec at the end of a workgroup's LDS doubles
constexpr double LOG_2PI = 1.8378770664093453;

// s of the points at xi and xj (d coordinates each); SCALED: the coordinates times p[r] = 1 / l_r first.  Two equal points give s = 0
// exactly (bt_scaled_diff).  The caller picks the rows: direct, through its index list, or the pair's larger index first.
template <bool SCALED>
__device__ __forceinline__ double sqdist(const double* xi, const double* xj, int64_t d, const double* p) {
  double s = 0.0;
  for (int64_t r = 0; r < d; ++r) {
    double df;
    if constexpr (SCALED) df = bt_scaled_diff(xi[r], xj[r], p[r]);
    else df = xi[r] - xj[r];
    s = fma(df, df, s);
  }
  return s;
}

// the record prm (np_store constants of make_deriv_spec) into ks, by the workgroup's nthreads threads (t: the thread); the caller places
// the barrier
template <int KID>
__device__ __forceinline__ void load_spec(KernelSpec& ks, const double* prm, int np_store, int n_params, int t, int nthreads) {
  if (t == 0) { ks.id = KID; ks.n_params = n_params; }
  for (int k = t; k < np_store; k += nthreads) ks.p[k] = prm[k];
}

// entry (r, c) of the image of K + noise I of a model of n points: kv() is the pair's kernel value, asked for only where it counts
template <class KV>
__device__ __forceinline__ double image_entry(int r, int c, int n, double noise, KV kv) {
  double v = 0.0;
  if (r >= c) {
    if (r < n) {
      v = kv();
      if (r == c) v += noise;
    } else {
      v = r == c ? 1.0 : 0.0;
    }
  }
  return v;
}

// (W rhs)_k, W = L^-1 of the factored image S (its diagonal in Wdiag), n points: thread t = (k = t >> 2, q = t & 3); i = q, q + 4, ... < k
// in one fma chain.  The q == 0 thread of row k hands the finished value (0 from n on) to the caller's epilogue, done(k, value).
template <class Done>
__device__ __forceinline__ void winv_forward(const double* S, const double* Wdiag, const double* rhs, int n, int t, Done done) {
  const int k = t >> 2, q = t & 3;
  double acc = 0.0;
  if (k < n)
    for (int i = q; i < k; i += 4) acc = fma(S[i + k * BLD], rhs[i], acc);
  acc += __shfl_xor(acc, 1, 64);
  acc += __shfl_xor(acc, 2, 64);
  if (q == 0) done(k, k < n ? fma(Wdiag[k], rhs[k], acc) : 0.0);
}

// (W^T rhs)_i: thread t = (i = t >> 2, q = t & 3); k = i + 1 + q, i + 5 + q, ... < n in one fma chain; done(i, value) as above
template <class Done>
__device__ __forceinline__ void winv_transposed(const double* S, const double* Wdiag, const double* rhs, int n, int t, Done done) {
  const int i = t >> 2, q = t & 3;
  double acc = 0.0;
  if (i < n)
    for (int k = i + 1 + q; k < n; k += 4) acc = fma(S[i + k * BLD], rhs[k], acc);
  acc += __shfl_xor(acc, 1, 64);
  acc += __shfl_xor(acc, 2, 64);
  if (q == 0) done(i, i < n ? fma(Wdiag[i], rhs[i], acc) : 0.0);
}

// the sum of at most 128 entries, entry t in thread t (v = 0 where there is none): wave w < 2 leaves its wave_sum in two[OFF + w].  No
// barrier in here: the caller places one, reached by the whole workgroup, and reads two[OFF] + two[OFF + 1] behind it.  (OFF: the slot in
// the caller's array, a constant of the index rather than of the pointer: the classifier's code comes out as it was that way.)
template <int OFF = 0>
__device__ __forceinline__ void sum128(double v, double* two, int wave, int lane) {
  if (wave < 2) {
    v = wave_sum(v);
    if (lane == 0) two[OFF + wave] = v;
  }
}
// two such sums behind one barrier: v0 to four[OFF + w], v1 to four[OFF + 2 + w]
template <int OFF = 0>
__device__ __forceinline__ void sum128(double v0, double v1, double* four, int wave, int lane) {
  if (wave < 2) {
    v0 = wave_sum(v0);
    v1 = wave_sum(v1);
    if (lane == 0) { four[OFF + wave] = v0; four[OFF + 2 + wave] = v1; }
  }
}

}  // namespace

}  // namespace gprc
