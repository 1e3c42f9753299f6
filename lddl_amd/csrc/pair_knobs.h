// The environment knobs the pair stage reads when a plan starts (check_plan_args, pairs_api.hip):
// what each accepts and the message it is rejected with. (Host-only and free of the HIP runtime,
// like plan_split.h, so a CPU program can test it: tests/pair_knobs_check.cpp.) The knobs read
// later, where they apply, stay with their stages: LDDL_NATIVE_LDS_WORDS (pairs_native.hip),
// LDDL_AMD_MASK_POOL and LDDL_PLAN_SLICE_DENSE (the replay planner, pairs.hip), LDDL_SHUFFLE_GLOBAL
// (pairs_shuffle.hip).
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

// Every knob of check_plan_args, in the order their messages have always come.
//   LDDL_PLAN_SPLIT (A/B knob of the split replay plan): unset or -1 = automatic
//   (plan_split_point), 0 = one range, k > 0 = a head range of exactly min(k, n_part) partitions.
//   LDDL_PLAN_SLICE (A/B knob of the time-sliced replay plan): unset or -1 = automatic
//   (plan_slice_on), 0 = never, k > 0 = always, with a quantum of k documents.
//   LDDL_PLAN_WAVES (tests and A/B): the persistent grid of a sliced plan, g >= 1 workgroups
//   (unset or -1: what the device holds at once).
inline int read_plan_knobs(FyKnobs* fy, int64_t* split, int64_t* slice, int64_t* waves) {
  *split = *slice = *waves = -1;
  static const char kWavesMsg[] = "LDDL_PLAN_WAVES must be -1 (auto) or a workgroup count up to 2^20";
  int rc;
  if ((rc = read_int_knob("LDDL_PLAN_SPLIT", -1, "LDDL_PLAN_SPLIT must be -1 (auto), 0 or a partition count",
                          split)) ||
      (rc = read_int_knob("LDDL_PLAN_SLICE", -1,
                          "LDDL_PLAN_SLICE must be -1 (auto), 0 or a quantum of documents", slice)) ||
      (rc = read_int_knob("LDDL_PLAN_WAVES", -1, kWavesMsg, waves)))
    return rc;
  if (*waves == 0 || *waves > (1 << 20)) LDDL_FAIL(-1, "%s", kWavesMsg);
  if (*split > 0 && *slice > 0)
    LDDL_FAIL(-1, "LDDL_PLAN_SPLIT and LDDL_PLAN_SLICE are both forced: a split plan is not sliced");
  return read_fy_knobs(fy);
}

}  // namespace lddl
