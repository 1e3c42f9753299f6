// lddl_denoise_params_make: the host side of BART text infilling. From the weights
// of the span lengths 0 .. n it makes the cumulative table the kernel compares a draw with, and
// the start probability at which a word deep in a row is deleted or replaced with probability
// mask_ratio. The bisection is span_params.cpp's (span_solve.h).
#include "common.h"
#include "lddl_amd.h"
#include "span_solve.h"

#include <cmath>

extern "C" int lddl_denoise_params_make(double mask_ratio, int32_t n, const double* weights,
                                        lddl_denoise_params* out) {
  if (!out) LDDL_FAIL(-1, "null denoise params");
  if (n < 1 || n > LDDL_SPAN_MAX_N)
    LDDL_FAIL(-1, "longest span %d outside [1, %d]", n, LDDL_SPAN_MAX_N);
  if (!(mask_ratio >= 0.0 && mask_ratio <= 1.0)) LDDL_FAIL(-1, "mask_ratio outside [0, 1]");
  double w[LDDL_SPAN_MAX_N + 1], sum = 0.0;
  for (int k = 0; k <= n; ++k) {
    if (weights) {
      if (!(weights[k] >= 0.0) || !std::isfinite(weights[k]))
        LDDL_FAIL(-1, "span weight %d is negative or not a number", k);
      w[k] = weights[k];
    } else {  // Poisson(3): w_k proportional to 3^k / k!
      w[k] = k == 0 ? 1.0 : w[k - 1] * 3.0 / k;
    }
    sum += w[k];
  }
  if (!(sum > 0.0)) LDDL_FAIL(-1, "span weights are all zero");
  // q[k] = P(len > k) and cum[k] = P(len <= k), k = 0 .. n - 1
  double q[LDDL_SPAN_MAX_N], acc = 0.0;
  for (int k = 0; k < n; ++k) {
    acc += w[k] / sum;
    q[k] = std::fmax(0.0, 1.0 - acc);
    out->cum[k] = (float)std::fmin(acc, 1.0);
  }
  for (int k = n; k < LDDL_SPAN_MAX_N; ++k) out->cum[k] = 1.0f;
  out->n = n;
  const double reach = lddl::span_coverage(1.0, q, n);  // what s = 1 deletes or replaces
  if (mask_ratio > reach + 1e-12)
    LDDL_FAIL(-1, "mask_ratio %.12g cannot be reached: every head starting a span gives %.12g",
              mask_ratio, reach);
  if (mask_ratio == 0.0) out->p_start = 0.0f;
  else if (mask_ratio >= reach) out->p_start = 1.0f;
  else out->p_start = (float)lddl::span_solve_start(mask_ratio, q, n);
  return 0;
}
