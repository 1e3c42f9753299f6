// lddl_span_params_make: the host side of n-gram (span) dynamic masking. From the
// length distribution it makes the cumulative table the kernels compare a draw with, and the
// start probability at which a word deep in a row is masked with probability mlm_probability.
#include "common.h"
#include "lddl_amd.h"
#include "span_solve.h"

#include <cmath>

extern "C" int lddl_span_params_make(double mlm_probability, int32_t n, const double* weights,
                                     lddl_span_params* out) {
  if (!out) LDDL_FAIL(-1, "null span params");
  if (n < 1 || n > LDDL_SPAN_MAX_N)
    LDDL_FAIL(-1, "span length %d outside [1, %d]", n, LDDL_SPAN_MAX_N);
  if (!(mlm_probability >= 0.0 && mlm_probability <= 1.0))
    LDDL_FAIL(-1, "mlm_probability outside [0, 1]");
  double w[LDDL_SPAN_MAX_N];
  if (weights) {
    double sum = 0.0;
    for (int k = 0; k < n; ++k) {
      if (!(weights[k] >= 0.0)) LDDL_FAIL(-1, "span weight %d is negative or not a number", k);
      sum += w[k] = weights[k];
    }
    if (!(std::fabs(sum - 1.0) <= 1e-9)) LDDL_FAIL(-1, "span weights sum to %.12g, not 1", sum);
  } else {  // P(len = k) proportional to 1 / k
    double sum = 0.0;
    for (int k = 0; k < n; ++k) sum += 1.0 / (k + 1);
    for (int k = 0; k < n; ++k) w[k] = 1.0 / (k + 1) / sum;
  }
  // q[k] = P(len > k), q[0] = 1; cum[k - 1] = P(len <= k)
  double q[LDDL_SPAN_MAX_N], acc = 0.0;
  for (int k = 0; k < n; ++k) {
    q[k] = k == 0 ? 1.0 : std::fmax(0.0, 1.0 - acc);
    acc += w[k];
    if (k < n - 1) out->cum[k] = (float)std::fmin(acc, 1.0);
  }
  for (int k = n - 1; k < LDDL_SPAN_MAX_N - 1; ++k) out->cum[k] = 1.0f;
  out->n = n;
  if (n == 1 || mlm_probability == 0.0 || mlm_probability == 1.0) {
    out->p_start = (float)mlm_probability;
    return 0;
  }
  // the coverage rises strictly with s (q[0] = 1) from 0 at s = 0 to 1 at s = 1
  out->p_start = (float)lddl::span_solve_start(mlm_probability, q, n);
  return 0;
}
