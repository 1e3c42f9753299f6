// CPU check of the split plan's host decisions (csrc/plan_split.h): the split-point rule and the
// capacity extrapolation. Built with AddressSanitizer + UBSan by tests/test_plan_split.py; exits
// non-zero on the first failed expectation.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "plan_split.h"

using lddl::plan_split_point;
using lddl::plan_suggest_capacity;

#define EXPECT(c)                                                    \
  do {                                                               \
    if (!(c)) {                                                      \
      fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

int main() {
  // ---- split point ----
  const int64_t cap = 7168;
  // automatic: only when the partitions exceed the capacity; the head is half the capacity, so
  // the tail is never under half of the partitions (no tail below any threshold)
  EXPECT(plan_split_point(0, cap, -1) == 0);
  EXPECT(plan_split_point(1, cap, -1) == 0);
  EXPECT(plan_split_point(cap, cap, -1) == 0);
  EXPECT(plan_split_point(cap + 1, cap, -1) == cap / 2);
  EXPECT(plan_split_point(9537, cap, -1) == cap / 2);
  EXPECT(plan_split_point(9537, 0, -1) == 0);  // unknown capacity: one range
  EXPECT(plan_split_point(9537, 1, -1) == 0);  // (no head of 0 partitions)
  EXPECT(plan_split_point(9537, -5, -1) == 0);
  // never
  EXPECT(plan_split_point(9537, cap, 0) == 0);
  // forced: exactly min(k, n_part), whatever the capacity
  EXPECT(plan_split_point(9537, cap, 1) == 1);
  EXPECT(plan_split_point(9537, cap, 9536) == 9536);
  EXPECT(plan_split_point(9537, cap, 9537) == 9537);
  EXPECT(plan_split_point(9537, cap, 1 << 30) == 9537);
  EXPECT(plan_split_point(3, 0, 2) == 2);
  EXPECT(plan_split_point(0, cap, 5) == 0);  // no partitions: nothing to split
  for (int64_t n = 0; n < 300; ++n)
    for (int64_t c = 0; c < 300; c += 7)
      for (int64_t k = -1; k < 12; ++k) {
        const int64_t s = plan_split_point(n, c, k);
        EXPECT(s >= 0 && s <= n);
        if (k > 0 && n > 0) EXPECT(s == (k < n ? k : n));
        if (k < 0 && s) EXPECT(s == c / 2 && s >= 1 && n > c && (n - s) * 2 > n);
        if (k < 0 && n <= c) EXPECT(s == 0);
      }

  // ---- capacity ----
  // never below the head count
  for (int64_t h : {int64_t(0), int64_t(1), int64_t(1000), int64_t(1) << 40})
    for (int64_t all : {int64_t(0), int64_t(1), int64_t(5000), int64_t(100000000000)})
      for (int64_t th : {int64_t(0), int64_t(1), int64_t(4000), int64_t(100000000000)})
        EXPECT(plan_suggest_capacity(h, all, th) >= h);
  // the proportion, with the margin on top
  {
    const int64_t c = plan_suggest_capacity(6400, 1000000, 640000);  // x 1 / 0.64 = 10000
    EXPECT(c >= 10000 && c <= 10000 + 10000 / 64 + 1024);
  }
  EXPECT(plan_suggest_capacity(0, 10, 0) == 1024);   // empty head: the margin alone
  EXPECT(plan_suggest_capacity(-3, 10, 5) == 1024);  // (negative counts clamp to 0)
  // monotone in the head count and in the total
  {
    int64_t prev = -1;
    for (int64_t h = 0; h < 200000; h += 37) {
      const int64_t c = plan_suggest_capacity(h, 2500000000, 1600000000);
      EXPECT(c >= prev);
      prev = c;
    }
    prev = -1;
    for (int64_t all = 0; all < 4000000000; all += 9999991) {
      const int64_t c = plan_suggest_capacity(123456, all, 1600000000);
      EXPECT(c >= prev);
      prev = c;
    }
  }
  // 10^11 tokens: the product is far beyond 64 bits, the result is not
  {
    const int64_t T = 100000000000;  // kept tokens = output tokens at dup 1
    const int64_t c = plan_suggest_capacity(5 * (T / 100 * 64), T, T / 100 * 64);
    EXPECT(c >= 5 * T && c <= 5 * T + 5 * T / 64 + 1024 + 64);
    // saturation instead of wrap-around
    EXPECT(plan_suggest_capacity(INT64_MAX, INT64_MAX, 1) == INT64_MAX);
    EXPECT(plan_suggest_capacity(INT64_MAX, 0, 0) == INT64_MAX);
  }
  // ---- the mode of a replay plan ----
  // The rules, written out here on their own: sliced iff there are partitions, no split is forced,
  // slicing is not off, and it is forced or (automatic, enabled) the sliced capacity is >= 2 and
  // below the partitions; else split (masking, partitions, the knob not 0) at the forced head or
  // half the one-shot capacity when that is >= 2 and below the partitions; else one range. Each
  // capacity is asked at most once and only where it is used.
  {
    const int64_t caps[] = {0, 1, 2, 7, 16, 40};
    for (int64_t n = 0; n <= 40; ++n)
      for (int64_t c_shot : caps)
        for (int64_t c_sliced : caps)
          for (int masking = 0; masking < 2; ++masking)
            for (int64_t split_knob : {int64_t(-1), int64_t(0), int64_t(1), int64_t(5), int64_t(100)})
              for (int64_t slice_knob : {int64_t(-1), int64_t(0), int64_t(1), int64_t(9)}) {
                if (split_knob > 0 && slice_knob > 0) continue;  // (refused by the knob parser)
                int asked[2] = {0, 0};
                auto capacity_of = [&](bool sliced, int64_t* capacity) {
                  ++asked[sliced];
                  *capacity = sliced ? c_sliced : c_shot;
                  return 0;
                };
                lddl::ReplayMode m;
                m.sliced = true;
                m.split = 77;
                EXPECT(lddl::plan_replay_mode(n, masking != 0, split_knob, slice_knob, capacity_of, &m) == 0);
                const bool may_slice = n > 0 && split_knob <= 0 && slice_knob != 0;
                const bool ask_sliced = may_slice && (slice_knob > 0 || lddl::kPlanSliceAuto);
                const bool want_sliced =
                    ask_sliced && (slice_knob > 0 || (c_sliced >= 2 && c_sliced < n));
                const bool may_split = !want_sliced && masking && n > 0 && split_knob != 0;
                int64_t want_split = 0;
                if (may_split && split_knob > 0) want_split = split_knob < n ? split_knob : n;
                if (may_split && split_knob < 0 && c_shot >= 2 && c_shot < n) want_split = c_shot / 2;
                EXPECT(m.sliced == want_sliced);
                EXPECT(m.split == want_split);
                EXPECT(!(m.sliced && m.split));
                EXPECT(m.capacity == (ask_sliced ? c_sliced : 0));  // (handed on: not asked twice)
                EXPECT(asked[1] == (ask_sliced ? 1 : 0));
                EXPECT(asked[0] == (may_split && split_knob < 0 ? 1 : 0));
              }
    // an error of the query comes back as it is, with the mode at one range
    for (int fail_sliced = 0; fail_sliced < 2; ++fail_sliced) {
      auto failing = [&](bool sliced, int64_t* capacity) {
        *capacity = 7;
        return sliced == (fail_sliced != 0) ? -42 : 0;
      };
      lddl::ReplayMode m;
      m.sliced = true;
      m.split = 77;
      m.capacity = 77;
      // 40 partitions, capacity 7, everything automatic: the sliced query comes first; with
      // slicing off, the one-shot query decides the split
      EXPECT(lddl::plan_replay_mode(40, true, -1, fail_sliced ? -1 : 0, failing, &m) == -42);
      EXPECT(!m.sliced && m.split == 0 && m.capacity == 0);
    }
  }
  printf("plan_split_check ok\n");
  return 0;
}
