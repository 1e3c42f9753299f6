// Reading an environment knob as a number, for the knob parsers (pair_knobs.h, tok_knobs.h).
// Host-only and free of the HIP runtime, so a CPU program can test what includes it.
#pragma once
#include <cstdint>
#include <cstdlib>

#include "common.h"

namespace lddl {

inline int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// A knob that takes a whole decimal number >= lo: unset leaves *out as it is; anything else
// (no digits, trailing characters, a value below lo) fails with `msg`.
inline int read_int_knob(const char* name, long long lo, const char* msg, int64_t* out) {
  const char* e = getenv(name);
  if (!e) return 0;
  char* end = nullptr;
  const long long v = strtoll(e, &end, 10);
  if (end == e || *end || v < lo) LDDL_FAIL(-1, "%s", msg);
  *out = v;
  return 0;
}

}  // namespace lddl
