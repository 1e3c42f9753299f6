// Python's character classes on the device, for the units that read the table
// lddl_punkt_set_params uploaded (segment.hip, bart.hip): ASCII whitespace by a bit test, and the
// class bits of any other code point through the two-level table (tools/make_punkt_tables.py).
// Each translation unit gets its own copy (anonymous namespace).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lddl {

// class bits: `\s` / str.isspace(), str.isupper(), str.islower(), [^\W\d], `\d`
enum : uint32_t { kPSpace = 1, kPUpper = 2, kPLower = 4, kPAlnod = 8, kPDigit = 16 };

struct ClassTab {
  const uint16_t* l1;    // page of code points [256 k, 256 k + 256)
  const uint8_t* pages;  // class bits, 256 per page
};

// All the device tables of lddl_punkt_set_params, as the segmenter's kernels take them.
struct PkEnt;  // punkt_params.h
struct PunktTab {
  ClassTab cls;
  const int32_t* lower;  // (cp, lower) pairs, sorted
  int32_t n_lower;
  const PkEnt* hash;
  uint32_t hmask;
  int32_t n_rec;
  const uint8_t* keys;
};

namespace {

// Python `\s` / str.isspace() on ASCII: \t \n \v \f \r, \x1c-\x1f, space
__device__ __forceinline__ bool ascii_space(uint32_t c) {
  return c < 64 && ((0x00000001F0003E00ull >> c) & 1ull);
}

// class bits of a code point >= 0x80 (0 past U+10FFFF: a malformed sequence decodes to one)
__device__ __forceinline__ uint32_t class_bits(const ClassTab& t, uint32_t cp) {
  if (cp >= 0x110000u) return 0;
  return t.pages[(uint32_t)t.l1[cp >> 8] * 256u + (cp & 255u)];
}

}  // namespace
}  // namespace lddl
