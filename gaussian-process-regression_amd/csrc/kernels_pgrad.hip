// kernels_pgrad.hip -- the contraction of the prediction gradients for gfx950 (gprc_gpr_predict_grad).
//
//   d mu / d x*_c      =      sum_j alpha_j dk(x*, x_j) / d x*_c
//   d sigma^2 / d x*_c = -2 sum_j w_j     dk(x*, x_j) / d x*_c,     w = K_y^-1 k*
//
// and every supported kernel has dk / d x*_c = -h_j (x*_c - x_jc) t_c with one scalar h per pair (s = |x* - x_j|^2):
//   sqrexp        h = k / l^2                       the device sums k (x*_c - x_jc),            the tail multiplies by 1 / l^2
//   sqrexp_ard    h = k, t_c = 1 / l_c^2            coordinates staged divided by l_c: k (x*_c - x_jc) / l_c,        by 1 / l_c
//   gammaexp      h = k gamma u / s, u = (s / l^2)^(gamma / 2); 0 at s = 0       k u / s (x*_c - x_jc),              by gamma
//   ratquad       h = k / (q l^2), q = 1 + s / (2 alpha l^2)                     k / q (x*_c - x_jc),                by 1 / l^2
//   matern32      h = 3 e^-a / l^2, a = sqrt(3 s) / l                            e^-a (x*_c - x_jc),                 by 3 / l^2
//   matern52      h = 5/3 (1 + a) e^-a / l^2, a = sqrt(5 s) / l                  (1 + a) e^-a (x*_c - x_jc),         by 5 / (3 l^2)
//   matern32_ard, matern52_ard    the same with l = 1 on coordinates staged divided by l_c, t_c = 1 / l_c^2;         by 3 / l_c, 5 / (3 l_c)
// (h is finite at s = 0 for the Matern kernels and the difference is 0: that pair contributes an exact 0.)
// The difference is formed directly (x* sum p - sum p x cancels for points far from the origin).
//
// A workgroup owns one row tile of the chunk (128 test points, two per lane), one STRIPE of column tiles (64 training points each,
// 16 per wave) and one group of PG_Z coordinates.  Per tile the squared distances are formed from all d coordinates staged through
// LDS 16 at a time, as the fill forms them; h follows; then the lane adds alpha_j h (x*_c - x_jc) -- and, WITH_VAR, w_ij h (x*_c - x_jc)
// with w read from the solved chunk, 16 bytes a lane, 1 KiB contiguous per wave and column -- into its 2 x PG_Z (x 2) running sums,
// which stay in registers across the stripe together with the lane's own 2 x PG_Z coordinates.  No derivative array exists.
// The solved chunk is stored COLUMN-REVERSED (training point j in column n_pad - 1 - j: it left the solve with the reversed factor
// that way); the kernel maps the index, there is no second reversal pass.
// For d > PG_Z the coordinate groups are further workgroups (blockIdx.z); each forms the distances and h again.  Sixteen sums per
// row and quantity would need 128 more registers a lane and halve the occupancy for every d; d <= 8 pays nothing.
//
// Order of summation is fixed: a lane's columns ascending, tile after tile of the stripe, the four waves in wave order; one partial
// per (stripe, coordinate, row); the stripes are added in order by pred_grad_sum_kernel.  No atomics.  The stripe is a function of
// n_pad alone, so a row's result does not depend on how the test points are chunked, bit for bit.
//
// The tile shape, the staging, the distance loop, h per pair (pair_weight) and the tail's factor (deriv_tail_factor) are pair_tile.h's:
// the last two are shared with the sample paths' gradient product (kernels_paths.hip).
#include "pair_tile.h"

#include <algorithm>

namespace gprc {

namespace {

constexpr int PG_Z = 8;     // coordinates whose sums one workgroup forms
constexpr int PG_MAX_STRIPES = 32;

struct PgradArgs {
  const double* Xs;      // d x m test points of the chunk
  const double* X;       // d x n training points
  const double* alpha;   // n_pad
  const double* W;       // m_pad x n_pad, column-reversed (WITH_VAR only)
  double* pmean;         // stripes x d x m_pad (may be null WITH_VAR)
  double* pvar;          // stripes x d x m_pad (WITH_VAR only)
  int64_t m, n, d, ldw, m_pad, n_pad;
  int64_t stripe_tiles, ntiles;
  KernelSpec ks;         // derived constants, see make_deriv_spec
};

// (h without the factor the tail applies: pair_tile.h's pair_weight)
template <int KID, bool WITH_VAR>
__global__ __launch_bounds__(256) void pred_grad_kernel(PgradArgs a) {
  __shared__ __attribute__((aligned(16))) double As[PT_D][PT_R];
  __shared__ double Bs[PT_C][PT_D + 1];
  __shared__ double Bz[PT_C][PG_Z + 1];   // the workgroup's own coordinates of the tile's training points
  __shared__ double Al[PT_C];
  __shared__ __attribute__((aligned(16))) double Red[4][PG_Z][PT_R];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t ti = (int64_t)blockIdx.x * PT_R;
  const int64_t stripe = blockIdx.y;
  const int64_t z0 = (int64_t)blockIdx.z * PG_Z;
  const int dz = (int)((a.d - z0 < PG_Z) ? (a.d - z0) : PG_Z);
  const int64_t tile0 = stripe * a.stripe_tiles;
  const int64_t tile1 = (tile0 + a.stripe_tiles < a.ntiles) ? tile0 + a.stripe_tiles : a.ntiles;
  const int64_t gi0 = ti + 2 * lane;
  constexpr bool ARD = is_ard(KID);   // coordinates staged divided by their length scale

  double xs0[PG_Z], xs1[PG_Z], gm0[PG_Z], gm1[PG_Z], gv0[PG_Z], gv1[PG_Z];
#pragma unroll
  for (int r = 0; r < PG_Z; ++r) {
    const double sc = (ARD && r < dz) ? a.ks.p[z0 + r] : 1.0;
    xs0[r] = (r < dz && gi0 < a.m) ? a.Xs[gi0 * a.d + z0 + r] * sc : 0.0;
    xs1[r] = (r < dz && gi0 + 1 < a.m) ? a.Xs[(gi0 + 1) * a.d + z0 + r] * sc : 0.0;
    gm0[r] = gm1[r] = gv0[r] = gv1[r] = 0.0;
  }

  for (int64_t tile = tile0; tile < tile1; ++tile) {
    const int64_t tj = tile * PT_C;
    double s0[16], s1[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) { s0[c] = 0.0; s1[c] = 0.0; }
    for (int64_t r0 = 0; r0 < a.d; r0 += PT_D) {
      const int dc = (int)((a.d - r0 < PT_D) ? (a.d - r0) : PT_D);
      __syncthreads();
      if (a.d > PT_D || tile == tile0) {   // (d <= 16: the test points' only chunk stays in LDS for the whole stripe)
        stage_points<ARD>(a.Xs, ti, a.m, a.d, r0, dc, PT_R, a.ks.p, t, [&](int i, int r, double v) { As[r][i] = v; });
      }
      stage_points<ARD>(a.X, tj, a.n, a.d, r0, dc, PT_C, a.ks.p, t, [&](int j, int r, double v) { Bs[j][r] = v; });
      if (r0 == 0) {
        if (t < PT_C) Al[t] = (tj + t < a.n) ? a.alpha[tj + t] : 0.0;
        stage_points<ARD>(a.X, tj, a.n, a.d, z0, dz, PT_C, a.ks.p, t, [&](int j, int r, double v) { Bz[j][r] = v; });
      }
      __syncthreads();
      accum_sqdist(As, Bs, dc, lane, wave, s0, s1);
    }

    // rows gi0, gi0 + 1 < m_pad and columns n_pad - 1 - (tj + 63) .. n_pad - 1 - tj inside [0, n_pad): every load is inside the chunk
    const double* wp = WITH_VAR ? a.W + gi0 + (a.n_pad - 1 - (tj + wave * 16)) * a.ldw : nullptr;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const int cj = wave * 16 + c;
      const double h0 = pair_weight<KID>(s0[c], a.ks), h1 = pair_weight<KID>(s1[c], a.ks);
      const double al = Al[cj];   // zero in the padding
      const double p0 = al * h0, p1 = al * h1;
      double q0 = 0.0, q1 = 0.0;
      if constexpr (WITH_VAR) {
        const double2 w = *reinterpret_cast<const double2*>(wp - c * a.ldw);   // exact zeros in the padding columns and rows
        q0 = w.x * h0;
        q1 = w.y * h1;
      }
#pragma unroll
      for (int r = 0; r < PG_Z; ++r) {
        if (r < dz) {
          const double b = Bz[cj][r];
          const double d0 = xs0[r] - b, d1 = xs1[r] - b;
          gm0[r] = fma(p0, d0, gm0[r]);
          gm1[r] = fma(p1, d1, gm1[r]);
          if constexpr (WITH_VAR) {
            gv0[r] = fma(q0, d0, gv0[r]);
            gv1[r] = fma(q1, d1, gv1[r]);
          }
        }
      }
    }
  }

  // the four waves' sums in wave order, one partial per (stripe, coordinate, row)
  auto write_partials = [&](const double (&g0)[PG_Z], const double (&g1)[PG_Z], double* out) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PG_Z; ++r) *reinterpret_cast<double2*>(&Red[wave][r][2 * lane]) = make_double2(g0[r], g1[r]);
    __syncthreads();
    for (int e = t; e < dz * PT_R; e += 256) {
      const int r = e / PT_R, i = e - r * PT_R;
      out[(stripe * a.d + z0 + r) * a.m_pad + ti + i] = sum4_in_order(Red[0][r][i], Red[1][r][i], Red[2][r][i], Red[3][r][i]);
    }
  };
  if (a.pmean) write_partials(gm0, gm1, a.pmean);
  if constexpr (WITH_VAR) write_partials(gv0, gv1, a.pvar);
}

// out[c + d i] = f_c * sum over the stripes, in order, of part[(st d + c) m_pad + i];  f_c = sign * (ard ? iso * ks.p[c] : iso)
__global__ __launch_bounds__(256) void pred_grad_sum_kernel(const double* part, int64_t stripes, int64_t d, int64_t m_pad, int64_t m, double sign,
                                                            double iso, int ard, KernelSpec ks, double* out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;   // rows fastest: the partials are read contiguously
  if (idx >= m * d) return;
  const int64_t c = idx / m, i = idx - c * m;
  double s = 0.0;
  for (int64_t st = 0; st < stripes; ++st) s += part[(st * d + c) * m_pad + i];
  out[c + d * i] = (sign * (ard ? iso * ks.p[c] : iso)) * s;
}

// column tiles per stripe: at most PG_MAX_STRIPES stripes (n_pad = 65536: 2048 columns each)
int64_t stripe_tiles_of(int64_t n_pad) { return (n_pad / PT_C + PG_MAX_STRIPES - 1) / PG_MAX_STRIPES; }

}  // namespace

int64_t pred_grad_stripes(int64_t n_pad) {
  const int64_t st = stripe_tiles_of(n_pad);
  return (n_pad / PT_C + st - 1) / st;
}

int launch_pred_grad(hipStream_t s, const KernelSpec& ks, const double* Xs, int64_t m, int64_t m_pad, const double* X, int64_t n, int64_t n_pad,
                     int64_t d, const double* alpha, const double* W, int64_t ldw, double* pmean, double* pvar) {
  if (m <= 0) return 0;
  GPRC_TRY(check_grad_kernel("predict_grad", ks.id));
  if (!pmean && !pvar) { set_error("pred_grad: no output"); return GPRC_ERR_ARG; }
  if (m_pad % PT_R || m_pad < m || n_pad % PT_C || n_pad < n || d < 1) { set_error("pred_grad: bad padding"); return GPRC_ERR_ARG; }
  if (pvar && (!W || ldw < m_pad || (ldw & 1) || (reinterpret_cast<uintptr_t>(W) & 15))) {
    set_error("pred_grad: the solved chunk must be 16-byte aligned with an even leading dimension >= m_pad");
    return GPRC_ERR_ARG;
  }
  const int64_t zgroups = (d + PG_Z - 1) / PG_Z;
  if (zgroups > 65535) { set_error("pred_grad: too many coordinates"); return GPRC_ERR_ARG; }
  PgradArgs a{Xs, X, alpha, W, pmean, pvar, m, n, d, ldw, m_pad, n_pad, stripe_tiles_of(n_pad), n_pad / PT_C, make_deriv_spec(ks)};
  const dim3 grid((unsigned)(m_pad / PT_R), (unsigned)pred_grad_stripes(n_pad), (unsigned)zgroups);
  // per element and coordinate group: the distance (3 d), h (~40), the sums (3 or 5 per coordinate); bytes: the solved chunk once
  const double elems = (double)m_pad * (double)n_pad * (double)zgroups;
  ProfScope ps(s, PK_PRED_GRAD, elems * (3.0 * d + 40.0 + (pvar ? 5.0 : 3.0) * PG_Z), 8.0 * ((pvar ? (double)m_pad * n_pad : 0.0) + (double)(m + n) * d + n));
  with_gradient_kernel(ks.id, [&](auto kid) {
    if (a.pvar) hipLaunchKernelGGL((pred_grad_kernel<decltype(kid)::value, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((pred_grad_kernel<decltype(kid)::value, false>), grid, dim3(256), 0, s, a);
  });
  GPRC_LAUNCH_CHECK();
  return 0;
}

int launch_pred_grad_sum(hipStream_t s, const KernelSpec& ks, const double* part, int64_t n_pad, int64_t d, int64_t m_pad, int64_t m, bool variance,
                         double* out) {
  if (m <= 0) return 0;
  GPRC_TRY(check_grad_kernel("predict_grad", ks.id));
  // the factor the tail applies (ARD: its constant times 1 / l_c per coordinate, from the spec)
  const double iso = deriv_tail_factor(ks);
  // dk / dx* = -h (x* - x) t: the mean's gradient carries -1, the variance's -2 * -1
  hipLaunchKernelGGL(pred_grad_sum_kernel, dim3((unsigned)((m * d + 255) / 256)), dim3(256), 0, s, part, pred_grad_stripes(n_pad), d, m_pad, m,
                     variance ? 2.0 : -1.0, iso, is_ard(ks.id) ? 1 : 0, make_deriv_spec(ks), out);
  GPRC_LAUNCH_CHECK();
  return 0;
}

}  // namespace gprc
