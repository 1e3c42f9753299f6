// CPU check of the time-sliced plan's host decisions (csrc/plan_split.h): whether a plan is
// sliced, the quantum and the hand-off ring's size. Built with AddressSanitizer + UBSan by
// tests/test_plan_slice.py; exits non-zero on the first failed expectation.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "plan_split.h"

using lddl::kPlanSliceAuto;
using lddl::kPlanSliceK;
using lddl::plan_slice_on;
using lddl::plan_slice_quantum;
using lddl::plan_slice_ring_entries;

#define EXPECT(c)                                                    \
  do {                                                               \
    if (!(c)) {                                                      \
      fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

// hand-offs of one partition of u units planned with quantum q: a yield before every slice but
// the first
static int64_t handoffs(int64_t u, int64_t q) { return u <= 0 ? 0 : (u + q - 1) / q - 1; }

int main() {
  const int64_t cap = 7168;
  // ---- whether to slice ----
  // automatic: never at n_part <= capacity or for an unknown capacity; above the capacity only
  // where the automatic mode is switched on
  for (int64_t n : {int64_t(0), int64_t(1), cap - 1, cap}) EXPECT(!plan_slice_on(n, cap, -1));
  for (int64_t c : {int64_t(-5), int64_t(0), int64_t(1)}) EXPECT(!plan_slice_on(9537, c, -1));
  EXPECT(plan_slice_on(cap + 1, cap, -1) == kPlanSliceAuto);
  EXPECT(plan_slice_on(9537, cap, -1) == kPlanSliceAuto);
  // never
  EXPECT(!plan_slice_on(9537, cap, 0));
  // forced: at any size and capacity, but not without partitions
  for (int64_t n : {int64_t(1), int64_t(8), cap, int64_t(9537)})
    for (int64_t c : {int64_t(0), int64_t(1), cap})
      for (int64_t k : {int64_t(1), int64_t(7), int64_t(1000000), INT64_MAX}) EXPECT(plan_slice_on(n, c, k));
  EXPECT(!plan_slice_on(0, cap, 5));
  EXPECT(!plan_slice_on(-3, cap, 5));

  // ---- quantum ----
  EXPECT(plan_slice_quantum(1000, 7) == 7);
  EXPECT(plan_slice_quantum(0, 7) == 7);
  EXPECT(plan_slice_quantum(1000, INT64_MAX) == INT64_MAX);
  EXPECT(plan_slice_quantum(0, -1) == 1);
  EXPECT(plan_slice_quantum(-9, -1) == 1);
  EXPECT(plan_slice_quantum(INT64_MAX, -1) == INT64_MAX / kPlanSliceK + (INT64_MAX % kPlanSliceK != 0));
  for (int64_t u = 1; u < 3000; ++u) {
    const int64_t q = plan_slice_quantum(u, -1);
    EXPECT(q >= 1 && q * kPlanSliceK >= u && (q - 1) * kPlanSliceK < u);  // ceil(u / K)
    EXPECT(handoffs(u, q) <= kPlanSliceK - 1);
  }

  // ---- ring entries: never below the hand-offs the quantum implies ----
  // partitions of uneven sizes (empty ones among them), forced quanta and the automatic one
  for (int64_t n_part : {int64_t(1), int64_t(2), int64_t(7), int64_t(100)})
    for (int64_t knob : {int64_t(-1), int64_t(1), int64_t(2), int64_t(7), int64_t(1000), int64_t(1000000)})
      for (int64_t shape = 0; shape < 4; ++shape) {
        int64_t total = 0, need = 0;
        for (int64_t p = 0; p < n_part; ++p) {
          const int64_t u = shape == 0 ? 0 : shape == 1 ? 1 + p : shape == 2 ? (p % 3 ? 0 : 997) : 5 * (400 + 13 * p);
          total += u;
          need += handoffs(u, plan_slice_quantum(u, knob));
        }
        const int64_t r = plan_slice_ring_entries(n_part, total, knob);
        EXPECT(r >= need);
        EXPECT(r >= 16 && r <= total + 16);  // (never more than one entry per unit, plus the margin)
        if (knob < 0) EXPECT(r <= n_part * (kPlanSliceK - 1) + 16);
        // partitions may cover fewer units than the bound the caller has (dropped documents)
        EXPECT(plan_slice_ring_entries(n_part, total + 1000, knob) >= r);
      }
  EXPECT(plan_slice_ring_entries(0, 0, -1) == 16);
  EXPECT(plan_slice_ring_entries(-4, -4, 3) == 16);
  EXPECT(plan_slice_ring_entries(9537, 5 * 2000000, -1) == 9537 * (kPlanSliceK - 1) + 16);
  EXPECT(plan_slice_ring_entries(9537, 5 * 2000000, 1) == 5 * 2000000 + 16);

  // ---- saturating arithmetic ----
  EXPECT(plan_slice_ring_entries(INT64_MAX, INT64_MAX, -1) == INT64_MAX);
  EXPECT(plan_slice_ring_entries(INT64_MAX, INT64_MAX, 1) == INT64_MAX);
  EXPECT(plan_slice_ring_entries(INT64_MAX, 10, -1) == 26);
  EXPECT(plan_slice_ring_entries(3, INT64_MAX, -1) == 3 * (kPlanSliceK - 1) + 16);
  EXPECT(plan_slice_ring_entries(3, INT64_MAX, INT64_MAX) == 17);
  EXPECT(plan_slice_ring_entries(1, INT64_MAX - 3, 1) == INT64_MAX);
  printf("plan_slice_check ok\n");
  return 0;
}
