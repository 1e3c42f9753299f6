// The start probability of a span scheme, host only: span_params.cpp and
// denoise_params.cpp both solve 1 - prod_k (1 - s * q_k) = target for s by bisection in double.
#pragma once

namespace lddl {

// P(a word is reached) for a word with n - 1 words before it: the span of the word k places back
// reaches it iff it started (s) and is longer than k (q_k); the starts are independent.
inline double span_coverage(double s, const double* q, int n) {
  double miss = 1.0;
  for (int k = 0; k < n; ++k) miss *= 1.0 - s * q[k];
  return 1.0 - miss;
}

// s in [0, 1] with span_coverage(s) = target; the coverage rises with s from 0 at s = 0, and the
// caller has made sure that target lies in (0, span_coverage(1))
inline double span_solve_start(double target, const double* q, int n) {
  double lo = 0.0, hi = 1.0;
  for (int it = 0; it < 200; ++it) {
    const double mid = 0.5 * (lo + hi);
    if (mid <= lo || mid >= hi) break;
    (span_coverage(mid, q, n) < target ? lo : hi) = mid;
  }
  return 0.5 * (lo + hi);
}

}  // namespace lddl
