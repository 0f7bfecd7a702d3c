// host_quadrature.h -- Gauss quadrature from a Lanczos tridiagonal, on the host and free of HIP (the stochastic Lanczos quadrature of
// gprc_igpr_logp_grad, gprc_iter.hip; DESIGN.md section 7, "Iterative GPR evidence"; tests/test_igpr_logp_cpu.py compiles it alone).
//
//   T = tridiag(off, diag, off), m x m, symmetric:   e_1^T f(T) e_1 = sum_i v_1i^2 f(lambda_i)
//
// with lambda_i the eigenvalues of T and v_1i the first components of its orthonormal eigenvectors (Golub & Welsch 1969): the implicit
// QL iteration with Wilkinson's shift, carrying the first row of the accumulated rotations and nothing else of the eigenvectors,
// O(m^2) flop and O(m) memory.  QL is backward stable: the computed pairs are exact for T + E, |E|_2 <= c m u |T|_2.
#pragma once
#include <cmath>
#include <vector>

namespace gprc {

enum { QUAD_OK = 0, QUAD_NOT_POSITIVE = 1, QUAD_NO_CONVERGENCE = 2, QUAD_BAD_ARGUMENT = 3 };

// In place: diag (m) becomes the eigenvalues of T (in no particular order), first (m) the first components of their eigenvectors; off
// holds the m - 1 off-diagonal entries and is left as it is.  m >= 1.  QUAD_NO_CONVERGENCE after 60 sweeps for one eigenvalue.
inline int tridiag_eigen_first(int m, double* diag, const double* off, double* first) {
  if (m < 1 || !diag || !first || (m > 1 && !off)) return QUAD_BAD_ARGUMENT;
  std::vector<double> e((size_t)m, 0.0);   // e[i] couples i and i + 1; e[m - 1] = 0
  for (int i = 0; i + 1 < m; ++i) e[i] = off[i];
  for (int i = 0; i < m; ++i) first[i] = i == 0 ? 1.0 : 0.0;
  const double eps = 0x1p-52;
  for (int l = 0; l < m; ++l) {
    for (int sweep = 0;; ++sweep) {
      int k = l;   // the first negligible coupling from l on: [l, k] is an unreduced block
      for (; k + 1 < m; ++k)
        if (std::fabs(e[k]) <= eps * (std::fabs(diag[k]) + std::fabs(diag[k + 1]))) break;
      if (k == l) break;   // diag[l] has converged
      if (sweep == 60) return QUAD_NO_CONVERGENCE;
      // Wilkinson's shift from the leading 2 x 2 of the block, then one implicit QL sweep from the bottom of the block up
      double g = (diag[l + 1] - diag[l]) / (2.0 * e[l]);
      double r = std::hypot(g, 1.0);
      g = diag[k] - diag[l] + e[l] / (g + std::copysign(r, g));
      double s = 1.0, c = 1.0, p = 0.0;
      int i = k - 1;
      for (; i >= l; --i) {
        double f = s * e[i];
        const double b = c * e[i];
        r = std::hypot(f, g);
        e[i + 1] = r;
        if (r == 0.0) {   // the block splits: undo the pending shift and start over
          diag[i + 1] -= p;
          e[k] = 0.0;
          break;
        }
        s = f / r;
        c = g / r;
        g = diag[i + 1] - p;
        r = (diag[i] - g) * s + 2.0 * c * b;
        p = s * r;
        diag[i + 1] = g + p;
        g = c * r - b;
        f = first[i + 1];   // the rotation, applied to the first row of the eigenvector matrix
        first[i + 1] = s * first[i] + c * f;
        first[i] = c * first[i] - s * f;
      }
      if (r == 0.0 && i >= l) continue;
      diag[l] -= p;
      e[l] = g;
      e[k] = 0.0;
    }
  }
  return QUAD_OK;
}

// *out = e_1^T log(T) e_1 = sum_i v_1i^2 log lambda_i, the terms added in index order in long double.  diag (m) and off (m - 1) are not
// modified.  QUAD_NOT_POSITIVE when an eigenvalue is <= 0 or not finite (T is not positive definite in floating point).
inline int tridiag_log_quadrature(int m, const double* diag, const double* off, double* out) {
  if (m < 1 || !diag || !out || (m > 1 && !off)) return QUAD_BAD_ARGUMENT;
  std::vector<double> d(diag, diag + m), e, v((size_t)m);
  if (m > 1) e.assign(off, off + (m - 1));
  const int rc = tridiag_eigen_first(m, d.data(), e.data(), v.data());
  if (rc != QUAD_OK) return rc;
  long double sum = 0.0L;
  for (int i = 0; i < m; ++i) {
    if (!(d[i] > 0.0) || !std::isfinite(d[i])) return QUAD_NOT_POSITIVE;
    sum += (long double)v[i] * (long double)v[i] * std::log((long double)d[i]);
  }
  *out = (double)sum;
  return QUAD_OK;
}

// The Lanczos tridiagonal of the preconditioned matrix from the coefficients of m steps of (preconditioned) conjugate gradients:
//   diag[0] = 1 / alpha_0,  diag[j] = 1 / alpha_j + beta_{j-1} / alpha_{j-1},  off[j] = sqrt(beta_j) / alpha_j   (j < m - 1)
// alpha: m entries, beta: at least m - 1.  diag: m, off: m - 1 (may be null for m = 1).
inline void cg_tridiagonal(int m, const double* alpha, const double* beta, double* diag, double* off) {
  for (int j = 0; j < m; ++j) {
    diag[j] = 1.0 / alpha[j] + (j > 0 ? beta[j - 1] / alpha[j - 1] : 0.0);
    if (j + 1 < m) off[j] = std::sqrt(beta[j]) / alpha[j];
  }
}

}  // namespace gprc
