// The host decisions of the replay plan (pairs.hip). Its mode: one range in one shot, one range
// time-sliced, or a head and a tail range (plan_replay_mode, the one place that knows the
// precedence). The split plan: where the partitions are cut, and how large the caller's output
// buffers should be when only the head's counts are known. The time-sliced plan: whether to
// slice, the quantum and the hand-off ring's size. (Host-only and free of the HIP runtime, so a
// CPU program can test it: tests/plan_split_check.cpp, tests/plan_slice_check.cpp.)
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

// ---- the time-sliced plan (pairs.hip, plan_replay_kernel's sliced mode) ----
// A sliced plan is one range planned by persistent waves: a wave works on a partition for a
// quantum of documents, parks its state and takes the next partition from a FIFO, so all the
// partitions share all the wave slots instead of the last ones running alone.

// Slices per partition of the automatic quantum (the partition's dup x documents / K). The
// chains end together to within one slice, so shorter slices shorten the launch's ramp-down,
// against ~K hand-offs per partition. (Measured on the 9,537-partition headline, partitions of
// ~1,335 units, pair stage: K = 3: 152.5 ms, 5: 152.4, 10: 151.6, 20: 150.5;
// profiles/r08_sliced_ab.txt.)
constexpr int64_t kPlanSliceK = 20;

// Whether the automatic mode slices at all (profiles/r08_sliced_ab.txt; the knob always can).
constexpr bool kPlanSliceAuto = true;

// Whether a one-range replay plan runs time-sliced.
//   capacity: planner workgroups the device holds at once (0: unknown)
//   knob:     LDDL_PLAN_SLICE: -1 automatic, 0 never, k > 0 always, with a quantum of k documents
// Automatic: only when the partitions exceed the capacity (else every partition has a slot from
// the start and there is nothing to share).
inline bool plan_slice_on(int64_t n_part, int64_t capacity, int64_t knob) {
  if (n_part <= 0 || knob == 0) return false;
  if (knob > 0) return true;
  return kPlanSliceAuto && capacity >= 2 && n_part > capacity;
}

// Documents (counted over the duplicate passes) a wave plans of a partition of `units` = dup x
// documents before it yields: the knob's count, else 1/K of the partition, rounded up; >= 1.
// (plan_replay_kernel computes the same per partition.)
inline int64_t plan_slice_quantum(int64_t units, int64_t knob) {
  if (knob > 0) return knob;
  if (units <= 0) return 1;
  return units / kPlanSliceK + (units % kPlanSliceK != 0);
}

// Entries of the hand-off ring: never below the hand-offs the quantum implies. A partition of u
// units yields ceil(u / q) - 1 <= u / q times, so a forced quantum q gives at most
// units_total / q in all; the automatic quantum at most K - 1 per partition (and never more than
// one per unit). Plus 16 entries of margin; saturating at INT64_MAX.
inline int64_t plan_slice_ring_entries(int64_t n_part, int64_t units_total, int64_t knob) {
  if (n_part < 0) n_part = 0;
  if (units_total < 0) units_total = 0;
  unsigned __int128 v;
  if (knob > 0) {
    v = (unsigned __int128)((uint64_t)units_total / (uint64_t)knob);
  } else {
    v = (unsigned __int128)(uint64_t)n_part * (uint64_t)(kPlanSliceK - 1);
    if (v > (unsigned __int128)(uint64_t)units_total) v = (uint64_t)units_total;
  }
  v += 16;
  const unsigned __int128 lim = (unsigned __int128)INT64_MAX;
  return (int64_t)(v > lim ? lim : v);
}

// ---- the mode of a replay plan: one range in one shot, time-sliced, or split ----
struct ReplayMode {
  bool sliced = false;
  int64_t split = 0;     // partitions of the head range (0: one range); never with `sliced`
  int64_t capacity = 0;  // of the sliced instantiation, where it was asked (it sizes the grid)
};

// The precedence: a forced split beats slicing, slicing beats the automatic split, no masking
// means no split, a split is never sliced. capacity_of(bool sliced, int64_t* capacity) is the
// occupancy query of either planner instantiation (non-zero: an error, handed through with *m at
// one range); each is asked at most once and only where its answer is used: the sliced one
// whenever the knobs allow slicing, the one-shot one for the automatic split.
template <typename CapacityOf>
inline int plan_replay_mode(int64_t n_part, bool masking, int64_t split_knob, int64_t slice_knob,
                            CapacityOf&& capacity_of, ReplayMode* m) {
  *m = ReplayMode{};
  int64_t capacity = 0;  // (a forced split point takes none)
  int rc;
  if (n_part > 0 && split_knob <= 0 && slice_knob != 0 && (slice_knob > 0 || kPlanSliceAuto)) {
    if ((rc = capacity_of(true, &capacity))) return rc;
    m->sliced = plan_slice_on(n_part, capacity, slice_knob);
    m->capacity = capacity;
  }
  if (m->sliced || !masking || n_part <= 0 || split_knob == 0) return 0;
  if (split_knob < 0 && (rc = capacity_of(false, &capacity))) return rc;
  m->split = plan_split_point(n_part, capacity, split_knob);
  return 0;
}

}  // namespace lddl
