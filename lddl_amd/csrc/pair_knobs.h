// The environment knobs the pair stage reads when a plan starts (check_plan_args, pairs_api.hip):
// what each accepts and the message it is rejected with. (Host-only and free of the HIP runtime,
// like plan_split.h, so a CPU program can test it: tests/pair_knobs_check.cpp.) No stage reads a
// knob of its own: each takes its values from PlanWork::knobs.
#pragma once
#include <cstdint>
#include <cstdlib>

#include "common.h"
#include "knobs.h"

namespace lddl {

// A/B knobs of the mask replay, LDDL_FY_MODE / LW / RA / PF (what they select: resolve_masks)
struct FyKnobs {
  int mode, lw, ra, pf;
};

// the A/B knobs take only the values a test runs (unsupported values and
// combinations were ignored without notice)
inline int read_fy_knobs(FyKnobs* k) {
  *k = FyKnobs{env_int("LDDL_FY_MODE", -1), env_int("LDDL_FY_LW", 16), env_int("LDDL_FY_RA", 1),
               env_int("LDDL_FY_PF", 4)};
  if (k->mode < -1 || k->mode > 1) LDDL_FAIL(-1, "LDDL_FY_MODE must be -1 (auto), 0 or 1");
  if (k->lw != 16 && k->lw != 32) LDDL_FAIL(-1, "LDDL_FY_LW must be 16 or 32");
  if (k->ra < 0 || k->ra > 3) LDDL_FAIL(-1, "LDDL_FY_RA must be 0 .. 3");
  if (k->pf != 2 && k->pf != 4 && k->pf != 8) LDDL_FAIL(-1, "LDDL_FY_PF must be 2, 4 or 8");
  if (k->pf != 4 && k->ra != 1) LDDL_FAIL(-1, "LDDL_FY_PF applies with LDDL_FY_RA=1 only");
  if ((k->ra != 1 || k->pf != 4) && (k->mode == 0 || k->lw == 32))
    LDDL_FAIL(-1, "LDDL_FY_RA / PF select 16-lane branch-free variants (not with LDDL_FY_MODE=0 "
                  "or LDDL_FY_LW=32)");
  return 0;
}

// Every knob of check_plan_args, read in the order their messages have always come.
//   split (LDDL_PLAN_SPLIT, A/B knob of the split replay plan): unset or -1 = automatic
//   (plan_split_point), 0 = one range, k > 0 = a head range of exactly min(k, n_part) partitions.
//   slice (LDDL_PLAN_SLICE, A/B knob of the time-sliced replay plan): unset or -1 = automatic
//   (plan_slice_on), 0 = never, k > 0 = always, with a quantum of k documents.
//   waves (LDDL_PLAN_WAVES, tests and A/B): the persistent grid of a sliced plan, g >= 1
//   workgroups (unset or -1: what the device holds at once).
//   slice_dense (LDDL_PLAN_SLICE_DENSE, A/B, 0 .. 2): who packs `dense` in a sliced plan.
//   mask_pool (LDDL_AMD_MASK_POOL, tests): entries of the first attempt's mask pool, to force a
//   re-plan (unset = -1: sized from the kept tokens).
//   native_lds_words (LDDL_NATIVE_LDS_WORDS, tests): the cap on the LDS words of the native
//   planner's walk tables, so that the global-prefix path runs (unset = -1: kNativeLdsWordsCap).
//   shuffle_global (LDDL_SHUFFLE_GLOBAL, tests): set at all, whatever the value, forces the
//   partition shuffle's large-partition (global-memory) path.
struct PlanKnobs {
  int64_t split = -1, slice = -1, waves = -1, slice_dense = 1, mask_pool = -1, native_lds_words = -1;
  bool shuffle_global = false;
  FyKnobs fy;
};

inline int read_plan_knobs(PlanKnobs* k) {
  *k = PlanKnobs{};
  const struct { const char *name, *msg; int64_t lo, hi, *out; } ints[] = {
      {"LDDL_PLAN_SPLIT", "LDDL_PLAN_SPLIT must be -1 (auto), 0 or a partition count", -1, INT64_MAX, &k->split},
      {"LDDL_PLAN_SLICE", "LDDL_PLAN_SLICE must be -1 (auto), 0 or a quantum of documents", -1, INT64_MAX,
       &k->slice},
      {"LDDL_PLAN_WAVES", "LDDL_PLAN_WAVES must be -1 (auto) or a workgroup count up to 2^20", -1, 1 << 20,
       &k->waves},
      {"LDDL_PLAN_SLICE_DENSE", "LDDL_PLAN_SLICE_DENSE must be 0, 1 or 2", 0, 2, &k->slice_dense},
      {"LDDL_AMD_MASK_POOL", "LDDL_AMD_MASK_POOL must be an entry count >= 0", 0, INT64_MAX, &k->mask_pool},
      {"LDDL_NATIVE_LDS_WORDS", "LDDL_NATIVE_LDS_WORDS must be a word count >= 0", 0, INT64_MAX,
       &k->native_lds_words}};
  for (const auto& e : ints) {
    if (int rc = read_int_knob(e.name, e.lo, e.msg, e.out)) return rc;
    if (*e.out > e.hi || (e.out == &k->waves && *e.out == 0)) LDDL_FAIL(-1, "%s", e.msg);
  }
  k->shuffle_global = getenv("LDDL_SHUFFLE_GLOBAL") != nullptr;
  if (k->split > 0 && k->slice > 0)
    LDDL_FAIL(-1, "LDDL_PLAN_SPLIT and LDDL_PLAN_SLICE are both forced: a split plan is not sliced");
  return read_fy_knobs(&k->fy);
}

}  // namespace lddl
