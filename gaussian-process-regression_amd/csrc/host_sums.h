// host_sums.h -- the long-double tails the host finishes a reduction with, free of any device header so that they compile into a
// plain C++ program (a sanitizer build, for one).  The order is fixed, so two calls on the same values give the same bits.
#pragma once
#include <stdint.h>

namespace gprc {

// v[0] + v[1] + ... + v[n - 1], summed in index order in long double, rounded once
inline double sum_in_order(const double* v, int64_t n) {
  long double acc = 0.0L;
  for (int64_t i = 0; i < n; ++i) acc += (long double)v[i];
  return (double)acc;
}

}  // namespace gprc
