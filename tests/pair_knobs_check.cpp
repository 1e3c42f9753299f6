// CPU check of the pair stage's environment knobs (csrc/pair_knobs.h): every accepted value,
// every rejected value and the message it is rejected with. Built with AddressSanitizer + UBSan
// together with csrc/errors.cpp by tests/test_pair_knobs.py; exits non-zero on the first failed
// expectation.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "lddl_amd.h"
#include "pair_knobs.h"

using lddl::FyKnobs;
using lddl::PlanKnobs;
using lddl::read_plan_knobs;

#define EXPECT(c)                                                    \
  do {                                                               \
    if (!(c)) {                                                      \
      fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

static const char* const kAll[] = {"LDDL_PLAN_SPLIT", "LDDL_PLAN_SLICE", "LDDL_PLAN_WAVES",
                                   "LDDL_PLAN_SLICE_DENSE", "LDDL_AMD_MASK_POOL", "LDDL_NATIVE_LDS_WORDS",
                                   "LDDL_SHUFFLE_GLOBAL", "LDDL_FY_MODE", "LDDL_FY_LW", "LDDL_FY_RA",
                                   "LDDL_FY_PF"};

struct Knobs {
  int rc;
  FyKnobs fy;
  int64_t split, slice, waves, dense, pool;
  int64_t lds_words;
  bool shuffle_global;
};

// the knobs as a plan would read them with the environment {name = value, ...} (null: unset)
static Knobs read_with(const char* n0, const char* v0, const char* n1 = nullptr, const char* v1 = nullptr,
                       const char* n2 = nullptr, const char* v2 = nullptr) {
  for (const char* k : kAll) unsetenv(k);
  if (n0 && v0) setenv(n0, v0, 1);
  if (n1 && v1) setenv(n1, v1, 1);
  if (n2 && v2) setenv(n2, v2, 1);
  PlanKnobs p;
  p.split = p.slice = p.waves = p.slice_dense = p.mask_pool = p.native_lds_words = 99;
  p.shuffle_global = true;
  p.fy = FyKnobs{99, 99, 99, 99};
  const int rc = read_plan_knobs(&p);
  return Knobs{rc, p.fy, p.split, p.slice, p.waves, p.slice_dense, p.mask_pool, p.native_lds_words,
               p.shuffle_global};
}

static bool rejected(const Knobs& k, const char* msg) {
  return k.rc == -1 && strcmp(lddl_last_error(), msg) == 0;
}

static const char kSplitMsg[] = "LDDL_PLAN_SPLIT must be -1 (auto), 0 or a partition count";
static const char kSliceMsg[] = "LDDL_PLAN_SLICE must be -1 (auto), 0 or a quantum of documents";
static const char kWavesMsg[] = "LDDL_PLAN_WAVES must be -1 (auto) or a workgroup count up to 2^20";
static const char kDenseMsg[] = "LDDL_PLAN_SLICE_DENSE must be 0, 1 or 2";
static const char kPoolMsg[] = "LDDL_AMD_MASK_POOL must be an entry count >= 0";
static const char kLdsWordsMsg[] = "LDDL_NATIVE_LDS_WORDS must be a word count >= 0";
static const char kBothMsg[] = "LDDL_PLAN_SPLIT and LDDL_PLAN_SLICE are both forced: a split plan is not sliced";
static const char kRaPfMsg[] =
    "LDDL_FY_RA / PF select 16-lane branch-free variants (not with LDDL_FY_MODE=0 or LDDL_FY_LW=32)";

int main() {
  // ---- nothing set: every knob automatic, the mask replay's defaults ----
  {
    const Knobs k = read_with(nullptr, nullptr);
    EXPECT(k.rc == 0 && k.split == -1 && k.slice == -1 && k.waves == -1);
    EXPECT(k.fy.mode == -1 && k.fy.lw == 16 && k.fy.ra == 1 && k.fy.pf == 4);
    EXPECT(k.dense == 1 && k.pool == -1);  // the waves that leave the queue; the pool sized by the plan
    EXPECT(k.lds_words == -1 && !k.shuffle_global);  // the default cap; the shuffle's path by size
  }
  // ---- LDDL_PLAN_SPLIT and LDDL_PLAN_SLICE: -1, 0 or a count; a whole decimal number ----
  const struct {
    const char* name;
    const char* msg;
    int64_t Knobs::*field;
  } counts[] = {{"LDDL_PLAN_SPLIT", kSplitMsg, &Knobs::split}, {"LDDL_PLAN_SLICE", kSliceMsg, &Knobs::slice}};
  for (const auto& c : counts) {
    for (int64_t v : {int64_t(-1), int64_t(0), int64_t(7)}) {
      char text[32];
      snprintf(text, sizeof text, "%lld", (long long)v);
      const Knobs k = read_with(c.name, text);
      EXPECT(k.rc == 0 && k.*c.field == v);
      EXPECT(k.split + k.slice + k.waves == v - 2);  // (the other two stay automatic)
    }
    for (const char* bad : {"-2", "x", "3x", ""}) EXPECT(rejected(read_with(c.name, bad), c.msg));
  }
  // ---- LDDL_PLAN_WAVES: -1 or 1 .. 2^20 ----
  for (int64_t v : {int64_t(-1), int64_t(1), int64_t(1048576)}) {
    char text[32];
    snprintf(text, sizeof text, "%lld", (long long)v);
    const Knobs k = read_with("LDDL_PLAN_WAVES", text);
    EXPECT(k.rc == 0 && k.waves == v && k.split == -1 && k.slice == -1);
  }
  for (const char* bad : {"0", "-2", "1048577", "x"})
    EXPECT(rejected(read_with("LDDL_PLAN_WAVES", bad), kWavesMsg));
  // ---- LDDL_PLAN_SLICE_DENSE: 0, 1 or 2; LDDL_AMD_MASK_POOL: an entry count ----
  for (int64_t v : {int64_t(0), int64_t(1), int64_t(2)}) {
    char text[32];
    snprintf(text, sizeof text, "%lld", (long long)v);
    const Knobs k = read_with("LDDL_PLAN_SLICE_DENSE", text);
    EXPECT(k.rc == 0 && k.dense == v && k.pool == -1 && k.split == -1 && k.slice == -1 && k.waves == -1);
  }
  for (const char* bad : {"x", "", "-1", "3", "1x"})
    EXPECT(rejected(read_with("LDDL_PLAN_SLICE_DENSE", bad), kDenseMsg));
  for (int64_t v : {int64_t(0), int64_t(100), int64_t(1) << 40}) {
    char text[32];
    snprintf(text, sizeof text, "%lld", (long long)v);
    const Knobs k = read_with("LDDL_AMD_MASK_POOL", text);
    EXPECT(k.rc == 0 && k.pool == v && k.dense == 1 && k.split == -1 && k.slice == -1 && k.waves == -1);
  }
  for (const char* bad : {"x", "", "-5", "-1", "100x"})
    EXPECT(rejected(read_with("LDDL_AMD_MASK_POOL", bad), kPoolMsg));
  // (their messages come after LDDL_PLAN_WAVES', dense before pool, and before LDDL_FY_*')
  EXPECT(rejected(read_with("LDDL_PLAN_SLICE_DENSE", "3", "LDDL_PLAN_WAVES", "0"), kWavesMsg));
  EXPECT(rejected(read_with("LDDL_AMD_MASK_POOL", "x", "LDDL_PLAN_WAVES", "x"), kWavesMsg));
  EXPECT(rejected(read_with("LDDL_AMD_MASK_POOL", "x", "LDDL_PLAN_SLICE_DENSE", "x"), kDenseMsg));
  EXPECT(rejected(read_with("LDDL_FY_MODE", "2", "LDDL_PLAN_SLICE_DENSE", "3"), kDenseMsg));
  EXPECT(rejected(read_with("LDDL_FY_MODE", "2", "LDDL_AMD_MASK_POOL", "-5"), kPoolMsg));
  // (and, malformed, before the conflict of the two forced knobs)
  EXPECT(rejected(read_with("LDDL_PLAN_SPLIT", "2", "LDDL_PLAN_SLICE", "3", "LDDL_AMD_MASK_POOL", ""), kPoolMsg));
  // ---- LDDL_NATIVE_LDS_WORDS: a word count >= 0 (text used to read as 0) ----
  for (int64_t v : {int64_t(0), int64_t(64), int64_t(24576), int64_t(1) << 40}) {
    char text[32];
    snprintf(text, sizeof text, "%lld", (long long)v);
    const Knobs k = read_with("LDDL_NATIVE_LDS_WORDS", text);
    EXPECT(k.rc == 0 && k.lds_words == v && !k.shuffle_global);
    EXPECT(k.pool == -1 && k.dense == 1 && k.split == -1 && k.slice == -1 && k.waves == -1);
  }
  for (const char* bad : {"x", "", "-1", "-5", "64x", "6 4"})
    EXPECT(rejected(read_with("LDDL_NATIVE_LDS_WORDS", bad), kLdsWordsMsg));
  // (its message comes after LDDL_AMD_MASK_POOL's, before LDDL_FY_*' and before the conflict)
  EXPECT(rejected(read_with("LDDL_NATIVE_LDS_WORDS", "x", "LDDL_AMD_MASK_POOL", "x"), kPoolMsg));
  EXPECT(rejected(read_with("LDDL_NATIVE_LDS_WORDS", "x", "LDDL_PLAN_SPLIT", "x"), kSplitMsg));
  EXPECT(rejected(read_with("LDDL_FY_MODE", "2", "LDDL_NATIVE_LDS_WORDS", "-1"), kLdsWordsMsg));
  EXPECT(rejected(read_with("LDDL_PLAN_SPLIT", "2", "LDDL_PLAN_SLICE", "3", "LDDL_NATIVE_LDS_WORDS", "x"),
                  kLdsWordsMsg));
  // ---- LDDL_SHUFFLE_GLOBAL: set at all means forced, and nothing is refused ----
  for (const char* any : {"1", "0", "", "x"}) {
    const Knobs k = read_with("LDDL_SHUFFLE_GLOBAL", any);
    EXPECT(k.rc == 0 && k.shuffle_global && k.lds_words == -1 && k.pool == -1 && k.dense == 1);
    EXPECT(k.split == -1 && k.slice == -1 && k.waves == -1 && k.fy.mode == -1);
  }
  {
    const Knobs k = read_with("LDDL_SHUFFLE_GLOBAL", "1", "LDDL_NATIVE_LDS_WORDS", "64");
    EXPECT(k.rc == 0 && k.shuffle_global && k.lds_words == 64);
    // (it is read after the numbers and before LDDL_FY_*: their refusals stand beside it)
    EXPECT(rejected(read_with("LDDL_SHUFFLE_GLOBAL", "1", "LDDL_NATIVE_LDS_WORDS", "x"), kLdsWordsMsg));
    EXPECT(rejected(read_with("LDDL_SHUFFLE_GLOBAL", "1", "LDDL_FY_MODE", "2"),
                    "LDDL_FY_MODE must be -1 (auto), 0 or 1"));
  }
  // ---- a forced split is not sliced; "one range" may be ----
  EXPECT(rejected(read_with("LDDL_PLAN_SPLIT", "2", "LDDL_PLAN_SLICE", "3"), kBothMsg));
  {
    const Knobs k = read_with("LDDL_PLAN_SPLIT", "0", "LDDL_PLAN_SLICE", "3");
    EXPECT(k.rc == 0 && k.split == 0 && k.slice == 3 && k.waves == -1);
  }
  // (a malformed knob is reported before the conflict, in the order split, slice, waves)
  EXPECT(rejected(read_with("LDDL_PLAN_SPLIT", "2", "LDDL_PLAN_SLICE", "3", "LDDL_PLAN_WAVES", "0"), kWavesMsg));
  EXPECT(rejected(read_with("LDDL_PLAN_SPLIT", "x", "LDDL_PLAN_SLICE", "y"), kSplitMsg));
  // ---- LDDL_FY_*: the six combinations read_fy_knobs rejects ----
  EXPECT(rejected(read_with("LDDL_FY_MODE", "2"), "LDDL_FY_MODE must be -1 (auto), 0 or 1"));
  EXPECT(rejected(read_with("LDDL_FY_LW", "8"), "LDDL_FY_LW must be 16 or 32"));
  EXPECT(rejected(read_with("LDDL_FY_RA", "4"), "LDDL_FY_RA must be 0 .. 3"));
  EXPECT(rejected(read_with("LDDL_FY_PF", "3"), "LDDL_FY_PF must be 2, 4 or 8"));
  EXPECT(rejected(read_with("LDDL_FY_PF", "8", "LDDL_FY_RA", "2"), "LDDL_FY_PF applies with LDDL_FY_RA=1 only"));
  EXPECT(rejected(read_with("LDDL_FY_RA", "2", "LDDL_FY_MODE", "0"), kRaPfMsg));
  EXPECT(rejected(read_with("LDDL_FY_PF", "8", "LDDL_FY_LW", "32"), kRaPfMsg));
  // ... and values it takes (atoi semantics: LDDL_FY_* keep them)
  {
    const Knobs k = read_with("LDDL_FY_MODE", "1", "LDDL_FY_RA", "3");
    EXPECT(k.rc == 0 && k.fy.mode == 1 && k.fy.lw == 16 && k.fy.ra == 3 && k.fy.pf == 4);
    const Knobs m = read_with("LDDL_FY_MODE", "0", "LDDL_FY_LW", "32");
    EXPECT(m.rc == 0 && m.fy.mode == 0 && m.fy.lw == 32 && m.fy.ra == 1 && m.fy.pf == 4);
    // the plan knobs are checked first
    EXPECT(rejected(read_with("LDDL_FY_MODE", "2", "LDDL_PLAN_SLICE", "-2"), kSliceMsg));
  }
  printf("pair_knobs_check ok\n");
  return 0;
}
