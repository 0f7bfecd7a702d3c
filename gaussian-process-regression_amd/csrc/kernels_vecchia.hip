// kernels_vecchia.hip -- the conditionals of the Vecchia likelihood for gfx950 (gprc_lgpr_vecchia_logp_grad; DESIGN.md section 7, "Vecchia
// likelihood"): log p(y_i | y_N(i)) and the raw sums of its exact gradient, ONE CONDITIONAL PER WORKGROUP, many per launch.
//
// Workgroup g of a launch (256 threads, four waves) owns point i = i0 + g and runs, without leaving its CU,
//   gather   the point's row of the stored neighbour indices (rank r < m; the first rank of -1 ends the model): the model is the points
//            [N(i) in neighbour order, then i LAST], p + 1 <= 128 of them, p = min(m, i); their indices and targets go to LDS, the
//            coordinates are read through the indices wherever they are needed (L1 / L2) -- no gathered n m d copy exists;
//   fill     K_y = K + noise I into an LDS image of 16 nblk rows and columns, nblk = ceil((p + 1) / 16) -- the model's own block count, not
//            the launch's: kernel_value<KID> of the squared distance (small_model.h's sqdist: coordinates ascending, one fma chain, the
//            ARD kernels scale by 1 / l_c first); rows and columns >= p + 1 are the identity, everything above the diagonal is zero;
//   factor   blocked right-looking Cholesky in place with chol_tile.h's pieces and NO inverse blocks: per 16-column step wave 0's diag16
//            (the 16 x 16 diagonal block; its inverse W_ss stays transposed above that block's diagonal), the panel X_I = A_I W_ss^T and the
//            trailing C_IJ -= X_I X_J^T on v_mfma_f64_16x16x4_f64 (block_mma), blocks dealt to the four waves in order; a non-positive pivot
//            is noted in an LDS word (the one atomic) and the arithmetic finishes;
//   solve    z = L^-1 y forward, then a = L^-T z and w = L^-T e_p backward together, 16 rows at a time: the off-diagonal part against L,
//            the diagonal block against its stored inverse W_ss;
//   cond     -log L_pp - 1/2 z_p^2 - 1/2 log 2 pi;
//   gradient (when asked for) a' = a - z_p w (a'_p = 0), G = a a^T - a' a'^T - w w^T -- the difference of the full model's and the
//            sub-model's alpha alpha^T - K_y^-1 -- contracted over the pairs r > s against cross_weight<KID> by pair_tile.h's theta_terms,
//            which also contracts kernels_batch.hip's M: pairs count twice, gammaexp skips s = 0, the ARD kernels park 2 G_rs h_rs in the
//            image (L is no longer needed) and take a second pass over the coordinates; and sum_r G_rr for d / d noise.
// What a point leaves: cond_i, then the n_params sums WITHOUT the factors that do not depend on the pair, then sum_r G_rr, at
// out + (i - i0) (n_params + 2); its info word (0, or the first non-positive pivot, 1-based).  A flagged point's values are all NaN.
// vecchia_reduce_kernel then adds groups of 256 consecutive points BY GLOBAL INDEX (launches start at multiples of 256) into one row per
// group; the host adds the rows in order in long double and applies 1/2 and cross_grad_finish once.
//
// LDS (dynamic, sized from the call's m through NBMAX = 1, 2, 4, 8 blocks: image 16 NBMAX x (16 NBMAX + 16) doubles + vectors):
//   m <= 15: 7 632 B, m <= 31: 16 784 B, m <= 63: 47 376 B (three workgroups a CU), m <= 127: 157 712 B (one).
//
// Order of summation, fixed and a function of (p, d, kernel) alone -- a point's bits do not depend on the launch, the chunk or its place:
//   squared distance   coordinates ascending, one fma chain
//   factor             diag16's and the MFMA's own chains; which wave takes a block does not enter its arithmetic
//   solves             thread (row r, part q), q < 16: columns q, q + 16, ... in one fma chain; the 16 parts by xor 8, 4, 2, 1;
//                      the diagonal block: one product a part, the same tree
//   theta sums         pair e = r (p + 1) + s, r > s, belongs to thread e mod 256; a thread's pairs ascending in one fma chain; the 64 lanes
//                      by wave_sum; the four waves as (w0 + w1) + (w2 + w3)  (ARD: the same per coordinate)
//   sum G_rr           entry r to thread r < 128; each of the two waves by wave_sum; wave 0 + wave 1
//   groups of 256      point i to thread i mod 256; wave_sum; (w0 + w1) + (w2 + w3)
// No atomics except the one compare-and-swap on the workgroup's LDS flag; no scratch (profiles/vecchia_isa.txt).
#include "small_model.h"

namespace gprc {

namespace {

constexpr int VC_THREADS = 256;
constexpr int VC_WAVES = VC_THREADS / 64;

constexpr int vc_n(int nbmax) { return 16 * nbmax; }
constexpr int vc_ld(int nbmax) { return 16 * nbmax + 16; }   // + 16: consecutive k-slices of an MFMA operand move by 32 banks, as BLD does
// S, Wd, wdiag, six vectors (y, z, a, w, two right-hand sides), the waves' partials, the indices (ints), three words
constexpr int vc_lds_doubles(int nbmax) { return vc_n(nbmax) * vc_ld(nbmax) + 256 + 7 * vc_n(nbmax) + VC_WAVES * PT_D + vc_n(nbmax) / 2 + 2; }
static_assert(sizeof(double) * vc_lds_doubles(8) <= 163840, "the widest image must fit a workgroup's 160 KiB");

__device__ __forceinline__ double vc_sum16(double v) {   // the 16 lanes of a row, every lane gets the sum
  v += __shfl_xor(v, 8, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 1, 64);
  return v;
}

template <int KID, int NBMAX>
__global__ __launch_bounds__(VC_THREADS) void vecchia_kernel(const VecchiaArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  constexpr bool ARD = is_ard(KID);
  constexpr int N = vc_n(NBMAX), LD = vc_ld(NBMAX);
  double* S = sm;
  double* Wd = S + N * LD;
  double* wdiag = Wd + 256;
  double* yv = wdiag + N;
  double* zv = yv + N;
  double* av = zv + N;
  double* wv = av + N;
  double* tv = wv + N;     // the right-hand side of a 16-row step (z, then a); later a'
  double* tw = tv + N;     // ... of w
  double* red = tw + N;    // VC_WAVES x PT_D
  int* pts = reinterpret_cast<int*>(red + VC_WAVES * PT_D);   // N
  int* words = pts + N;    // [0], [1]: the leading non-negative ranks of waves 0 and 1; [2]: the flag
  const KernelSpec& ks = *a.ks;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int64_t i = a.i0 + blockIdx.x;
  const int64_t d = a.d;
  const double qnan = __builtin_nan("");

  // ---- gather
  {
    const int j = t < a.m ? a.nbr[i * a.m + t] : -1;
    const unsigned long long neg = __ballot(j < 0);
    if (wave < 2 && lane == 0) words[wave] = neg ? __ffsll((long long)neg) - 1 : 64;
    if (t == 0) words[2] = 0;
    __syncthreads();
    const int lead = words[0] < 64 ? words[0] : 64 + words[1];
    const int pt = t < lead ? j : (t == lead ? (int)i : -1);
    if (t < N) {
      pts[t] = pt;
      yv[t] = pt >= 0 ? a.y[pt] : 0.0;
    }
  }
  __syncthreads();
  const int p = words[0] < 64 ? words[0] : 64 + words[1];   // the point itself is row p, the last of the model
  const int np1 = p + 1, nblk = (np1 + 15) >> 4, Nm = 16 * nblk;

  // ---- fill
  for (int e = t; e < Nm * Nm; e += VC_THREADS) {
    const int c = e / Nm, r = e - c * Nm;
    S[r + c * LD] = image_entry(r, c, np1, a.noise, [=, &a, &ks] {
      const int gr = pts[r], gc = pts[c];
      return kernel_value<KID>(sqdist<ARD>(a.X + (int64_t)gr * d, a.X + (int64_t)gc * d, d, ks.p), ks);
    });
  }
  __syncthreads();

  // ---- factor: L in the lower triangle, W_ss = L_ss^-1 transposed above the diagonal of its own block, its diagonal in wdiag
  {
    const int q = lane >> 4, r = lane & 15;
    for (int s = 0; s < nblk; ++s) {
      const int c0 = 16 * s;
      if (wave == 0) diag16<LD>(S + c0 + c0 * LD, Wd, wdiag + c0, words + 2, c0);
      __syncthreads();
      for (int I = s + 1 + wave; I < nblk; I += VC_WAVES) {   // D'[x][y] = sum_k Wd[x][k] A_I[y][k] = X_I[y][x]
        const double4_t acc = block_mma<0>(Wd, 16, S + 16 * I + c0 * LD, LD, (double4_t){0.0, 0.0, 0.0, 0.0});
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) S[(16 * I + r) + (c0 + q + 4 * rr) * LD] = acc[rr];
      }
      __syncthreads();
      const int mm = nblk - s - 1, total = mm * (mm + 1) / 2;
      for (int b = wave; b < total; b += VC_WAVES) {          // D'[x][y] = C_IJ[y][x]: lanes run down the rows of C_IJ
        int ii = 0;
        while ((ii + 1) * (ii + 2) / 2 <= b) ++ii;
        const int I = s + 1 + ii, J = s + 1 + (b - ii * (ii + 1) / 2);
        double4_t acc;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) acc[rr] = S[(16 * I + r) + (16 * J + q + 4 * rr) * LD];
        acc = block_mma<1>(S + 16 * J + c0 * LD, LD, S + 16 * I + c0 * LD, LD, acc);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) S[(16 * I + r) + (16 * J + q + 4 * rr) * LD] = acc[rr];
      }
      __syncthreads();
    }
  }

  // ---- solve: thread (row r16 of the step, part k16)
  const int r16 = t >> 4, k16 = t & 15;
  for (int s = 0; s < nblk; ++s) {             // z = L^-1 y
    const int c0 = 16 * s, row = c0 + r16;
    double acc = 0.0;
    for (int k = k16; k < c0; k += 16) acc = fma(S[row + k * LD], zv[k], acc);
    acc = vc_sum16(acc);
    if (k16 == 0) tv[row] = yv[row] - acc;
    __syncthreads();
    const double w = k16 < r16 ? S[(c0 + k16) + row * LD] : (k16 == r16 ? wdiag[row] : 0.0);   // W_ss[r16][k16]
    const double v = vc_sum16(w * tv[c0 + k16]);
    if (k16 == 0) zv[row] = v;
    __syncthreads();
  }
  for (int s = nblk - 1; s >= 0; --s) {        // a = L^-T z, w = L^-T e_p
    const int c0 = 16 * s, col = c0 + r16;
    double acc_a = 0.0, acc_w = 0.0;
    for (int k = c0 + 16 + k16; k < Nm; k += 16) {
      const double l = S[k + col * LD];
      acc_a = fma(l, av[k], acc_a);
      acc_w = fma(l, wv[k], acc_w);
    }
    acc_a = vc_sum16(acc_a);
    acc_w = vc_sum16(acc_w);
    if (k16 == 0) {
      tv[col] = zv[col] - acc_a;
      tw[col] = (col == p ? 1.0 : 0.0) - acc_w;
    }
    __syncthreads();
    const double w = k16 > r16 ? S[col + (c0 + k16) * LD] : (k16 == r16 ? wdiag[col] : 0.0);   // W_ss[k16][r16]
    const double va = vc_sum16(w * tv[c0 + k16]), vw = vc_sum16(w * tw[c0 + k16]);
    if (k16 == 0) {
      av[col] = va;
      wv[col] = vw;
    }
    __syncthreads();
  }

  // ---- cond
  const bool flagged = words[2] != 0;
  const double zp = zv[p];
  double* out = a.out + (i - a.i0) * a.out_stride;
  if (t == 0) {
    out[0] = flagged ? qnan : -log(S[p + p * LD]) - 0.5 * (zp * zp) - 0.5 * LOG_2PI;
    a.info[i - a.i0] = words[2];
  }
  if (!a.want_grad) return;

  // ---- gradient
  if (t < N) tv[t] = (t < np1 && t != p) ? fma(-zp, wv[t], av[t]) : 0.0;   // a'
  __syncthreads();
  double a0 = 0.0, a1 = 0.0;
  for (int e = t; e < np1 * np1; e += VC_THREADS) {
    const int r = e / np1, s = e - r * np1;
    if (r > s) {
      double g = av[r] * av[s];
      g = fma(-tv[r], tv[s], g);
      g = fma(-wv[r], wv[s], g);
      const double gij = 2.0 * g;
      const int gr = pts[r], gs = pts[s];
      const double sq = sqdist<ARD>(a.X + (int64_t)gr * d, a.X + (int64_t)gs * d, d, ks.p);
      theta_terms<KID>(gij, sq, ks, a0, a1, S[r + s * LD]);   // (ARD parks its value over L, which nobody reads again)
    }
  }
  const int np = a.n_params;
  if constexpr (ARD) {
    for (int64_t c0 = 0; c0 < d; c0 += PT_D) {   // a thread re-reads the entries it wrote: no barrier in front
      const int dc = (int)((d - c0 < PT_D) ? (d - c0) : PT_D);
      double acc[PT_D];
#pragma unroll
      for (int cc = 0; cc < PT_D; ++cc) acc[cc] = 0.0;
      for (int e = t; e < np1 * np1; e += VC_THREADS) {
        const int r = e / np1, s = e - r * np1;
        if (r > s) {
          const double wh = S[r + s * LD];
          const double* xr = a.X + (int64_t)pts[r] * d + c0;
          const double* xs = a.X + (int64_t)pts[s] * d + c0;
#pragma unroll
          for (int cc = 0; cc < PT_D; ++cc)
            if (cc < dc) {
              const double df = bt_scaled_diff(xr[cc], xs[cc], ks.p[c0 + cc]);
              acc[cc] = fma(wh, df * df, acc[cc]);
            }
        }
      }
#pragma unroll
      for (int cc = 0; cc < PT_D; ++cc)
        if (cc < dc) {
          const double v = wave_sum(acc[cc]);
          if (lane == 0) red[wave * PT_D + cc] = v;
        }
      __syncthreads();
      if (t < dc) {
        const double v = sum4_pairs(red[t], red[PT_D + t], red[2 * PT_D + t], red[3 * PT_D + t]);
        out[1 + c0 + t] = flagged ? qnan : v;
      }
      __syncthreads();
    }
  } else {
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
    if (lane == 0) { red[wave * PT_D] = a0; red[wave * PT_D + 1] = a1; }
    __syncthreads();
    if (t < np) {
      const double v = sum4_pairs(red[t], red[PT_D + t], red[2 * PT_D + t], red[3 * PT_D + t]);
      out[1 + t] = flagged ? qnan : v;
    }
    __syncthreads();
  }

  // ---- d / d noise: sum_r G_rr
  {
    double g = 0.0;
    if (t < np1) {
      g = av[t] * av[t];
      g = fma(-tv[t], tv[t], g);
      g = fma(-wv[t], wv[t], g);
    }
    sum128(g, red, wave, lane);
    __syncthreads();
    if (t == 0) out[1 + np] = flagged ? qnan : red[0] + red[1];
  }
}

// group g of the launch: the points [256 g, 256 g + 256) of its `count`; row g of grp gets the sums of the columns in use and, last, the
// number of flagged points; cond (may be null) gets the points' cond_i
__global__ __launch_bounds__(256) void vecchia_reduce_kernel(const VecchiaReduceArgs a) {
  __shared__ double red[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t j = (int64_t)blockIdx.x * 256 + t;
  const bool in = j < a.count;
  const double* row = a.out + j * a.out_stride;
  double* g = a.grp + (int64_t)blockIdx.x * (a.out_stride + 1);
  if (a.cond && in) a.cond[j] = row[0];
  const int cols = a.want_grad ? a.out_stride : 1;
  for (int k = 0; k <= cols; ++k) {
    double v = 0.0;
    if (in) v = k < cols ? row[k] : (a.info[j] != 0 ? 1.0 : 0.0);
    v = wave_sum(v);
    if (lane == 0) red[wave] = v;
    __syncthreads();
    if (t == 0) g[k < cols ? k : a.out_stride] = sum4_pairs(red[0], red[1], red[2], red[3]);
    __syncthreads();
  }
}

template <int KID, int NBMAX>
int launch_one(hipStream_t s, const VecchiaArgs& a, int64_t count) {
  return launch_with_lds<vecchia_kernel<KID, NBMAX>>("vecchia_kernel", dim3((unsigned)count), dim3(VC_THREADS), sizeof(double) * vc_lds_doubles(NBMAX), s, a);
}

}  // namespace

int launch_vecchia(hipStream_t s, int kernel, const VecchiaArgs& a, int64_t count) {
  GPRC_TRY(check_grad_kernel("vecchia", kernel));
  if (count < 1 || count > GPRC_VECCHIA_CHUNK || a.i0 % 256 != 0 || !a.X || !a.y || !a.ks || !a.out || !a.info || a.d < 1 || a.m < 0 || a.m > 127 ||
      (a.m > 0 && !a.nbr) || a.n_params < 1 || a.out_stride != a.n_params + 2) {
    set_error("vecchia: bad launch arguments");
    return GPRC_ERR_ARG;
  }
  int rc = 0;
  with_gradient_kernel(kernel, [&](auto kid) {
    constexpr int KID = decltype(kid)::value;
    if (a.m <= 15) rc = launch_one<KID, 1>(s, a, count);
    else if (a.m <= 31) rc = launch_one<KID, 2>(s, a, count);
    else if (a.m <= 63) rc = launch_one<KID, 4>(s, a, count);
    else rc = launch_one<KID, 8>(s, a, count);
  });
  return rc;
}

int launch_vecchia_reduce(hipStream_t s, const VecchiaReduceArgs& a) {
  if (a.count < 1) return 0;
  hipLaunchKernelGGL(vecchia_reduce_kernel, dim3((unsigned)((a.count + 255) / 256)), dim3(256), 0, s, a);
  GPRC_LAUNCH_CHECK();
  return 0;
}

}  // namespace gprc
