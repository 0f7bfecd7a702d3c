// kernels_batch_predict.hip -- predictions from a fitted batch of small GPs for gfx950 (gprc_gpr_batch_predict; DESIGN.md section 7,
// "Batched predict"): posterior mean and latent variance of B models of n_b <= 128 points at each model's test points, one launch.
//
// What a fitted batch keeps per model (gprc_batch.hip): the points, alpha, W = L^-1 as potf2_blocked_body stores it (chol_tile.h: 128 x 128
// doubles, column-major, W[k][i] at k + 128 i, zero above the diagonal, the identity in rows and columns >= n_b) and the parameter
// record of kernels_batch.hip (the constants of make_deriv_spec, the noise, n_b).  With K*[k][j] = k(x_k, x*_j):
//   mean_j = sum_k K*[k][j] alpha_k,     var_j = k(x*_j, x*_j) - sum_i V[i][j]^2,   V = W K*.
//
// ONE WAVE owns 16 test points of one model and needs no other wave.  Lane (lc = lane & 15, lr = lane >> 4) holds column lc of K*: the
// entries k = 4 m + lr, m = 0 .. 31, each formed ONCE -- kernel_value<KID> of the squared distance, coordinates ascending in one fma chain,
// ARD coordinates scaled by bt_scaled_diff as the fit kernel scales them (a test point equal to a training point gives s = 0 exactly) --
// and kept in registers: entry m is exactly the B operand of the v_mfma_f64_16x16x4_f64 whose contraction index runs over 4 m .. 4 m + 3.
// The A operand is W[16 I + lc][4 m + lr], read from an LDS image of the model's W (leading dimension 144, as the factor body's image:
// the operand read is conflict-free).  Row block I of V contracts k only up to the end of block I -- W is triangular -- and the blocks stop
// at the last 16-row block that holds points: 4 + 8 + ... + 32 = 144 MFMAs per 16 points at n_b = 128.  Entries k >= n_b of K* are zero
// (their points are never read), so the identity rows of W add nothing.  Without var_out neither the image nor the products exist.
//
// A workgroup (eight waves) loads one model's alpha and W once (at most 128 KB) and loops over tiles of test points: workgroup (sp, g) of
// the (split, models) grid takes tiles sp 8 + wave, + 8 split, ...; the host picks the split so that a small batch still fills the CUs.
// LDS: 128 x 144 doubles of W, 128 of alpha, the KernelSpec: 150 536 B of the 163 840 B a workgroup may have, one workgroup per CU.
//
// Order of summation, fixed and a function of (n_b, d, kernel) alone -- a test point's bits depend on its model and its coordinates, not on
// its tile, the split, the batch, the other test points or which outputs are asked for:
//   squared distance   coordinates ascending, one fma chain
//   mean_j             lane (lc = j, lr): k = lr, 4 + lr, 8 + lr, ... < 16 ceil(n_b / 16) in one fma chain from 0; then the four lr groups
//                      as (q0 + q1) + (q2 + q3) (two xor-shuffles, 16 then 32; every lane of the column ends with the same bits)
//   V block            the MFMA's own chain over k ascending from 0
//   sum_i V[i][j]^2    lane (lc = j, lr): block I ascending, register g ascending (row 16 I + lr + 4 g), one fma chain from 0; the same
//                      two shuffles;   var_j = k(x*, x*) - that sum, unclamped
// No atomics; no register spills and no scratch (profiles/batch_predict_isa.txt).  A model whose factorisation was flagged (info != 0) gets
// NaN in both outputs and reads nothing but its info word.
//
// GRAD = true (gprc_gpr_batch_predict_grad; DESIGN.md section 7, "Batched prediction gradients and LOO") is the same body -- k_block,
// v_block and the two reductions below are shared, so mean and var are the bits above by construction -- with the gradients with respect
// to the test points, gprc_gpr_predict_grad's formulas in kernels_pgrad.hip's decomposition dk / dx*_c = -h (x*_c - x_kc) t_c:
//   dmean[d j + c] = -t_c sum_k (alpha_k h_kj) (x*_jc - x_kc),     dvar[d j + c] = 2 t_c sum_k (u_kj h_kj) (x*_jc - x_kc),   U = W^T V.
// V is already in B-operand layout: lane (lc, lr) ends row block I with acc[g] = V[16 I + 4 g + lr][lc], which is the B operand of the
// MFMA that contracts rows 16 I + 4 g .. + 3, so U needs no shuffle and no LDS round trip; row block Kb of U contracts i from block Kb to
// the last block (again 144 MFMAs at n_b = 128) and lands as u_k for k = 16 Kb + 4 g + lr, the k of the lane's K*.  Its A operand is W^T.
// Read from the image as stored that is a column walk, lanes 144 doubles apart, an 8-way bank conflict on every operand.  Instead the
// load MIRRORS the strict lower triangle of the image into its upper triangle, which held zeros: W^T's off-diagonal blocks are then read
// in W's own conflict-free pattern, and only the diagonal blocks' operands (4 MFMAs of a block's chain, in V's product and in U's) are
// masked with a select.  The mirror is written once per model (16 x 16 blocks in turn over the waves, an 8-way conflicted write).
// Registers, a lane: the mean's gradient goes FIRST (32 weights alpha h, dead before K* is born); then K* whole and V from the LAST row
// block to the first -- block I reads K* up to the end of block I, so K* and V together take 36 doubles, not 64 --; then U in V's place
// and u h in U's.  h is formed again from the squared distance for each gradient rather than kept (profiles/batch_predict_grad_isa.txt).
// The coordinates of X are read through L1 / L2, one coordinate at a time: d is not bounded and no per-coordinate sum lives in a register.
// Without dvar_out no mirror and no U; without var_out and dvar_out no image of W at all.  Order of summation, in addition to the above:
//   h's squared distance   as K*'s
//   U block            the MFMA's own chain over i ascending from 16 Kb
//   d.. [d j + c]      lane (lc = j, lr): k = lr, 4 + lr, 8 + lr, ... in one fma chain from 0 of (x*_c - x_kc) times the weight (ARD:
//                      bt_scaled_diff, an exact 0 at a training point); the four lr groups as the mean's; then one multiplication by
//                      -t_c or 2 t_c, t_c = deriv_tail_factor (ARD: times the record's 1 / l_c)
// A gammaexp pair at distance 0 has h = 0 (pair_weight).  The gradient bits of a test point depend on its model and coordinates alone.
#include "small_model.h"

namespace gprc {

namespace {

constexpr int BP_WAVES = BATCH_PREDICT_WAVES;
constexpr int BP_THREADS = 64 * BP_WAVES;
constexpr size_t BP_SMEM_BYTES = sizeof(double) * (PB * BLD + PB + SPEC_DOUBLES);
static_assert(BP_SMEM_BYTES <= 163840, "the batched predict kernel's LDS must fit a workgroup's 160 KiB");
static_assert(BATCH_PREDICT_TILE == 16 && PB == 128 && BLD % 2 == 0, "the lane layout is the 16 x 16 x 4 MFMA's");

typedef double v4d __attribute__((ext_vector_type(4)));

template <int KID, bool GRAD>
__global__ __launch_bounds__(BP_THREADS) void batch_predict_kernel(BatchPredictArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  constexpr bool ARD = is_ard(KID);
  double* Wl = sm;                      // PB x BLD: W[i][c] at i + c BLD
  double* av = sm + PB * BLD;           // alpha
  KernelSpec& ks = *reinterpret_cast<KernelSpec*>(av + PB);
  const int t = threadIdx.x, lane = t & 63, lc = lane & 15, lr0 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int64_t b = a.b0 + blockIdx.y;
  const int64_t ns = a.ns_each ? a.ns_each[b] : a.ns_max;
  const int64_t tiles = (ns + BATCH_PREDICT_TILE - 1) / BATCH_PREDICT_TILE;
  const int64_t first = (int64_t)blockIdx.x * BP_WAVES, step = (int64_t)gridDim.x * BP_WAVES;
  if (first >= tiles) return;           // the whole workgroup: this model has fewer tiles than the widest one
  double* mean = a.mean ? a.mean + b * a.ld_out : nullptr;
  double* var = a.var ? a.var + b * a.ld_out : nullptr;
  double* dmean = nullptr;
  double* dvar = nullptr;
  if constexpr (GRAD) {
    dmean = a.dmean ? a.dmean + b * a.ld_grad : nullptr;
    dvar = a.dvar ? a.dvar + b * a.ld_grad : nullptr;
  }
  const int64_t d = a.d;

  if (a.info[b] != 0) {                 // not positive definite: flagged by the fit, NaN here
    const double qnan = __builtin_nan("");
    for (int64_t tile = first + wave; tile < tiles; tile += step) {
      const int64_t j = tile * BATCH_PREDICT_TILE + lc;
      if (lr0 == 0 && j < ns) {
        if (mean) mean[j] = qnan;
        if (var) var[j] = qnan;
        if constexpr (GRAD) {
          for (int64_t c = 0; c < d; ++c) {
            if (dmean) dmean[j * d + c] = qnan;
            if (dvar) dvar[j * d + c] = qnan;
          }
        }
      }
    }
    return;
  }

  const double* prm = a.prm + b * a.prm_stride;
  const double* X = a.X + b * a.x_stride;
  const double* Xs = a.Xs + b * a.xs_stride;
  const int nb = (int)prm[a.np_store + 1];
  const int nblk = (nb + 15) >> 4, kend = 16 * nblk;
  const bool need_w = var || dvar;      // the image of W and the product V = W K*

  // ---- load: the spec, alpha, and (variance) rows and columns < kend of W, two rows a thread and load
  load_spec<KID>(ks, prm, a.np_store, a.n_params, t, BP_THREADS);
  if (t < PB) av[t] = a.alpha[b * PB + t];
  if (need_w) {
    const double* W = a.W + b * (PB * PB);
    const int i2 = 2 * (t & 63);
    if (i2 < kend) {
#pragma unroll 4
      for (int c = t >> 6; c < kend; c += BP_WAVES)
        *reinterpret_cast<double2*>(Wl + i2 + c * BLD) = *reinterpret_cast<const double2*>(W + i2 + c * PB);
    }
  }
  if constexpr (GRAD) {
    // ---- (variance gradient) the strict lower triangle of the image mirrored into its upper one, which is zero: the image is then
    // symmetric, W^T's off-diagonal blocks are read as W's are, and only the diagonal blocks' operands are masked.  16 x 16 blocks in
    // turn over the waves; the read is the operand pattern (conflict-free), the transposed write is 8-way conflicted, once per model.
    if (dvar) {
      __syncthreads();
      int cnt = 0;
      for (int I = 0; I < nblk; ++I)
        for (int J = 0; J <= I; ++J, ++cnt) {
          if ((cnt & (BP_WAVES - 1)) != wave) continue;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int r = 16 * I + lc, c = 16 * J + 4 * g + lr0;
            if (r > c) Wl[c + r * BLD] = Wl[r + c * BLD];
          }
        }
    }
  }
  __syncthreads();

  const double kss = kernel_value<KID>(0.0, ks);
  double tail = 0.0;
  if constexpr (GRAD) tail = deriv_tail_factor(ks);      // (the record keeps the caller's p[0], which is all the factor reads)
  for (int64_t tile = first + wave; tile < tiles; tile += step) {
    const int64_t j = tile * BATCH_PREDICT_TILE + lc;
    const double* xs = Xs + (j < ns ? j : ns - 1) * d;   // a column past the count repeats the last point and is not stored
    // lr as this turn's own value: what hangs on it (32 row pointers, 32 alphas, the operand addresses) is formed where it is used, not
    // kept in 130 registers across the turns -- the registers are K*'s
    int lr = lr0;
    asm volatile("" : "+v"(lr));
    // squared distances of the lane's test point to the training points k = 16 I + 4 u + lr, u = 0 .. 3
    auto sqdist4 = [&](int I, int lrow, double (&s)[4]) {
      const double* xk[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = 16 * I + 4 * u + lrow;
        xk[u] = X + (int64_t)(k < nb ? k : nb - 1) * d;
        s[u] = 0.0;
      }
      auto coordinate = [&](int64_t r) {
        const double xr = xs[r];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          double df;
          if constexpr (ARD) df = bt_scaled_diff(xk[u][r], xr, ks.p[r]);
          else df = xk[u][r] - xr;
          s[u] = fma(df, df, s[u]);
        }
      };
      if constexpr (GRAD) {                               // (not unrolled: the registers an unrolled loop takes are the weights' and V's)
#pragma clang loop unroll(disable)
        for (int64_t r = 0; r < d; ++r) coordinate(r);
      } else {
        for (int64_t r = 0; r < d; ++r) coordinate(r);
      }
    };
    double kst[32];
    double vu[GRAD ? 32 : 1];                             // GRAD: the weights alpha h; then V; then u = W^T V in its place; then u h
    double mu = 0.0, ss = 0.0;
    // ---- entries 4 I .. 4 I + 3 of the lane's column of K*: k = 16 I + 4 u + lr; the mean's chain
    auto k_block = [&](int I) {
      double s[4];
      sqdist4(I, lr, s);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = 16 * I + 4 * u + lr;
        const double v = k < nb ? kernel_value<KID>(s[u], ks) : 0.0;
        kst[4 * I + u] = v;
        mu = fma(v, av[k], mu);
      }
    };
    // ---- row block I of V = W K*: k up to the end of block I
    auto v_block = [&](int I) {
      v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int m = 0; m < 4 * (I + 1); ++m) {
        double aw = Wl[(16 * I + lc) + (4 * m + lr) * BLD];
        if constexpr (GRAD) {                             // the diagonal block: above the diagonal the image may hold the mirror
          if (m >= 4 * I) aw = (4 * (m - 4 * I) + lr <= lc) ? aw : 0.0;
        }
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(aw, kst[m], acc, 0, 0, 0);
      }
      return acc;
    };
    // ---- (GRAD) the weights of the lane's 32 pairs: h from the squared distance, formed again -- the registers that held K* and its
    // distances hold something else by now -- times alpha_k (the mean's gradient) or times what w holds, u_k (the variance's)
    auto weights = [&](double (&w)[GRAD ? 32 : 1], auto by_alpha) {
#pragma unroll
      for (int I = 0; I < 8; ++I) {
        if (I < nblk) {
          double s[4];
          sqdist4(I, lr, s);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int k = 16 * I + 4 * u + lr;
            const double h = k < nb ? pair_weight<KID>(s[u], ks) : 0.0;
            if constexpr (decltype(by_alpha)::value) w[4 * I + u] = av[k] * h;
            else w[4 * I + u] = w[4 * I + u] * h;
          }
        }
      }
    };
    // ---- (GRAD) out[d j + c] = (sign t_c) sum_k w_k (x*_c - x_kc), the coordinates one at a time: one fma chain over the lane's k
    // ascending, the lr groups as the mean's.  dk / dx*_c = -h (x*_c - x_kc) t_c: the mean's gradient carries -1, the variance's -2 * -1
    // (kernels_pgrad.hip's tail)
    auto contract = [&](const double (&w)[GRAD ? 32 : 1], double* out, double sign) {
      for (int64_t c = 0; c < d; ++c) {
        int lq = lr;
        asm volatile("" : "+v"(lq));                      // (the 32 addresses are formed here, per coordinate, not kept)
        const double xc = xs[c];
        double q = 0.0;
#pragma unroll
        for (int I = 0; I < 8; ++I) {
          if (I < nblk) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int k = 16 * I + 4 * u + lq;
              const double xk = X[(int64_t)(k < nb ? k : nb - 1) * d + c];
              double df;
              if constexpr (ARD) df = bt_scaled_diff(xc, xk, ks.p[c]);
              else df = xc - xk;
              q = fma(df, w[4 * I + u], q);
            }
          }
        }
        q += __shfl_xor(q, 16, 64);
        q += __shfl_xor(q, 32, 64);
        const double f = ARD ? tail * ks.p[c] : tail;
        if (lr == 0 && j < ns) out[j * d + c] = (sign * f) * q;
      }
    };
    if constexpr (!GRAD) {
#pragma unroll
      for (int I = 0; I < 8; ++I) {
        if (I < nblk) {                                   // uniform over the workgroup
          k_block(I);
          if (need_w) {
            const v4d acc = v_block(I);
#pragma unroll
            for (int g = 0; g < 4; ++g) ss = fma(acc[g], acc[g], ss);
          }
        }
      }
    } else {
      // The mean's gradient first, while nothing else is held: its 32 weights and the coordinate loop.
      if (dmean) {
        weights(vu, std::true_type{});
        contract(vu, dmean, -1.0);
      }
      // Mean and variance: the same blocks and the same chains as above in another order of blocks.  All of K* first, then V from the
      // LAST row block to the first -- block I reads K* up to the end of block I, so its four entries of K* die as its four of V are
      // born, and K* and V together never take more than 36 doubles a lane -- then the squares, block I ascending as above.
#pragma unroll
      for (int I = 0; I < 8; ++I)
        if (I < nblk) k_block(I);
      if (need_w) {
#pragma unroll
        for (int I = 7; I >= 0; --I) {
          if (I < nblk) {
            __builtin_amdgcn_sched_barrier(0);            // one block's operands in flight, not eight's
            const v4d acc = v_block(I);
#pragma unroll
            for (int g = 0; g < 4; ++g) vu[4 * I + g] = acc[g];
          }
        }
#pragma unroll
        for (int I = 0; I < 8; ++I) {
          if (I < nblk) {
#pragma unroll
            for (int g = 0; g < 4; ++g) ss = fma(vu[4 * I + g], vu[4 * I + g], ss);
          }
        }
      }
    }
    mu += __shfl_xor(mu, 16, 64);
    mu += __shfl_xor(mu, 32, 64);
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);
    if (lr == 0 && j < ns) {
      if (mean) mean[j] = mu;
      if (var) var[j] = kss - ss;
    }
    if constexpr (GRAD) {
      if (dvar) {
        // ---- row block Kb of U = W^T V: i from block Kb to the last block, the MFMA's own chain over i ascending; acc[g] = u_k,
        // k = 16 Kb + 4 g + lr, takes the place of V block Kb, which no later block reads
#pragma unroll
        for (int Kb = 0; Kb < 8; ++Kb) {
          if (Kb < nblk) {
            __builtin_amdgcn_sched_barrier(0);
            v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int I = Kb; I < 8; ++I) {
              if (I < nblk) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                  double aw = Wl[(16 * Kb + lc) + (16 * I + 4 * g + lr) * BLD];   // W[16 I + 4 g + lr][16 Kb + lc], from the mirror
                  if (I == Kb) aw = (lc <= 4 * g + lr) ? aw : 0.0;
                  acc = __builtin_amdgcn_mfma_f64_16x16x4f64(aw, vu[4 * I + g], acc, 0, 0, 0);
                }
              }
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) vu[4 * Kb + g] = acc[g];
          }
        }
        weights(vu, std::false_type{});
        contract(vu, dvar, 2.0);
      }
    }
  }
}

}  // namespace

namespace {

template <bool GRAD>
int launch_batch_predict_any(const char* who, hipStream_t s, int kernel, const BatchPredictArgs& a, int64_t models, int split) {
  GPRC_TRY(check_grad_kernel(who, kernel));
  const bool outputs = a.mean || a.var || (GRAD && (a.dmean || a.dvar));
  if (models < 1 || models > 65535 || split < 1 || split > 65535 || !a.X || !a.prm || !a.alpha || !a.W || !a.info || !a.Xs || !outputs ||
      a.d < 1 || a.ns_max < 1 || a.ld_out < a.ns_max || a.np_store < a.n_params || a.np_store > MAX_PARAMS || a.n_params < 1 ||
      (GRAD && (a.dmean || a.dvar) && a.ld_grad < a.d * a.ns_max)) {
    set_error(std::string(who) + ": bad launch arguments");
    return GPRC_ERR_ARG;
  }
  int rc = 0;
  with_gradient_kernel(kernel, [&](auto kid) {
    rc = launch_with_lds<batch_predict_kernel<decltype(kid)::value, GRAD>>(who, dim3((unsigned)split, (unsigned)models), dim3(BP_THREADS), BP_SMEM_BYTES, s, a);
  });
  return rc;
}

}  // namespace

int launch_batch_predict(hipStream_t s, int kernel, const BatchPredictArgs& a, int64_t models, int split) {
  return launch_batch_predict_any<false>("batch_predict", s, kernel, a, models, split);
}

int launch_batch_predict_grad(hipStream_t s, int kernel, const BatchPredictArgs& a, int64_t models, int split) {
  return launch_batch_predict_any<true>("batch_predict_grad", s, kernel, a, models, split);
}

}  // namespace gprc
