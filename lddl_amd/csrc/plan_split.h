// The two host decisions of the split replay plan (pairs.hip): where the planner's partitions are
// cut into a head and a tail range, and how large the caller's output buffers should be when only
// the head's counts are known. (Host-only and free of the HIP runtime, so a CPU program can test
// it: tests/plan_split_check.cpp.)
#pragma once
#include <cstdint>

namespace lddl {

// Partitions of the head range, or 0 for one range (no split).
//   capacity: planner workgroups (one wave, one partition each) the device holds at once
//   knob:     LDDL_PLAN_SPLIT: -1 automatic, 0 never, k > 0 a head of exactly min(k, n_part)
// Automatic: split only when the partitions exceed the capacity, so that some of them wait for a
// free slot and the launch ends in a long ramp-down; the head is then HALF the capacity. The two
// launches are dispatched from two queues side by side, so a head of up to half the capacity is
// resident from the start whatever the queues' order, and it is complete early enough for its
// downstream work to end before the tail does. (Measured on the 9,537-partition headline,
// capacity 7,168: pair stage 160.9 ms in one range; head = capacity 159.5, 6,144: 155.2,
// 4,800: 153.3, 3,584: 153.1, 2,400: 153.6. The tail is then always more than half of the
// partitions, so no minimum-tail rule is needed.)
inline int64_t plan_split_point(int64_t n_part, int64_t capacity, int64_t knob) {
  if (n_part <= 0 || knob == 0) return 0;
  if (knob > 0) return knob < n_part ? knob : n_part;
  if (capacity < 2 || n_part <= capacity) return 0;
  return capacity / 2;
}

// Output capacity suggested from the head's count: the partitions are statistically alike, so
// the total is about head_count * kept tokens (all) / kept tokens (head); plus 1/64 and 1024
// entries of margin. Never below head_count, monotone in head_count and in tok_all, saturating
// at INT64_MAX (the product is taken in 128 bits).
inline int64_t plan_suggest_capacity(int64_t head_count, int64_t tok_all, int64_t tok_head) {
  if (head_count < 0) head_count = 0;
  unsigned __int128 v = (unsigned __int128)(uint64_t)head_count;
  if (tok_head > 0 && tok_all > tok_head)
    v = (v * (unsigned __int128)(uint64_t)tok_all + (uint64_t)tok_head - 1) / (uint64_t)tok_head;
  v += v / 64 + 1024;
  const unsigned __int128 lim = (unsigned __int128)INT64_MAX;
  return (int64_t)(v > lim ? lim : v);
}

}  // namespace lddl
