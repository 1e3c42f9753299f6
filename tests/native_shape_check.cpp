// CPU check of the native planner's launch shapes (csrc/native_shape.h): the walk tables' LDS
// words, mask_native_kernel's shape over every (seq, max_pred) a plan can have, and
// mask_ww_native_kernel's over every seq. Built with AddressSanitizer + UBSan by
// tests/test_native_shape.py; exits non-zero on the first failed expectation.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "native_shape.h"

using lddl::MaskShape;
using lddl::WalkLds;
using lddl::WwShape;

#define EXPECT(c)                                                    \
  do {                                                               \
    if (!(c)) {                                                      \
      fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

// bytes a wave of mask_native_kernel uses, written out a second time: a bitmap of `words` 32-bit
// words per lane, and per staged mask a 4-byte token and a 2-byte position
static size_t mask_wave_bytes(int32_t seq, int32_t max_pred, int32_t ppw) {
  const size_t words = (size_t)(seq + 31) / 32;
  return words * 64 * 4 + (size_t)ppw * (size_t)(max_pred > 1 ? max_pred : 1) * (4 + 2);
}

static void expect_mask(int32_t seq, int32_t max_pred, int32_t ppw, int32_t stage_cap, size_t wave_bytes,
                        int waves, int64_t per_wg) {
  const MaskShape m = lddl::native_mask_shape(seq, max_pred);
  EXPECT(m.ppw == ppw && m.stage_cap == stage_cap && m.wave_bytes == wave_bytes && m.waves == waves &&
         m.pairs_per_wg() == per_wg);
}

int main() {
  constexpr size_t kBudget = 65536;
  static_assert(lddl::kNativeMaskLds == kBudget, "the mask kernels' LDS budget");
  static_assert(lddl::kNativeLdsWordsCap == 24576, "the walk tables' default cap");
  size_t largest = 0;
  // ---- mask_native_kernel: every seq check_plan_args lets a masking plan have, every max_pred ----
  for (int32_t seq = 5; seq <= 4096; ++seq) {
    for (int32_t mp = 1; mp <= seq; ++mp) {
      const MaskShape m = lddl::native_mask_shape(seq, mp);
      EXPECT(m.words == (seq + 31) / 32);
      // ppw: a power of two in 1 .. 64, the largest whose bytes per wave fit the budget, or 1
      EXPECT(m.ppw >= 1 && m.ppw <= 64 && (m.ppw & (m.ppw - 1)) == 0);
      EXPECT(m.ppw == 1 || mask_wave_bytes(seq, mp, m.ppw) <= kBudget);
      EXPECT(m.ppw == 64 || mask_wave_bytes(seq, mp, 2 * m.ppw) > kBudget);
      EXPECT(m.stage_cap == m.ppw * mp);
      EXPECT(m.wave_bytes == mask_wave_bytes(seq, mp, m.ppw));
      EXPECT(m.waves >= 1 && m.waves <= 4);
      EXPECT(m.lds_bytes() == m.wave_bytes * (size_t)m.waves && m.lds_bytes() <= kBudget);
      EXPECT(m.threads() == 64u * (unsigned)m.waves && m.pairs_per_wg() == (int64_t)m.ppw * m.waves);
      if (m.lds_bytes() > largest) largest = m.lds_bytes();
    }
    // (max_pred 0, a plan without masking, sizes as 1)
    const MaskShape z = lddl::native_mask_shape(seq, 0), o = lddl::native_mask_shape(seq, 1);
    EXPECT(z.ppw == o.ppw && z.stage_cap == o.stage_cap && z.wave_bytes == o.wave_bytes && z.waves == o.waves);
  }
  EXPECT(largest == kBudget);  // (the budget is reached, never passed)
  // the grid covers every pair, with no workgroup to spare
  for (int64_t n : {int64_t(1), int64_t(255), int64_t(256), int64_t(257), int64_t(1) << 31}) {
    const MaskShape m = lddl::native_mask_shape(128, 19);
    EXPECT((int64_t)m.grid(n) * m.pairs_per_wg() >= n && ((int64_t)m.grid(n) - 1) * m.pairs_per_wg() < n);
    const WwShape w = lddl::native_ww_shape(128);
    EXPECT((int64_t)w.grid(n) * w.waves >= n && ((int64_t)w.grid(n) - 1) * w.waves < n);
  }
  // ---- the values of the formulas as they stood at the launch site ----
  expect_mask(128, 19, 64, 1216, 8320, 4, 256);
  expect_mask(512, 77, 64, 4928, 33664, 1, 64);
  expect_mask(512, 512, 16, 8192, 53248, 1, 16);
  expect_mask(4096, 614, 8, 4912, 62240, 1, 8);
  expect_mask(4096, 4096, 1, 4096, 57344, 1, 1);
  // ---- mask_ww_native_kernel ----
  for (int32_t seq = 5; seq <= 4096; ++seq) {
    const WwShape w = lddl::native_ww_shape(seq);
    EXPECT(w.seqp % 64 == 0 && w.seqp >= seq - 3 && w.seqp < seq - 3 + 64);
    EXPECT(w.wave_bytes == (size_t)8 * (size_t)(w.seqp + w.seqp / 64 + 1));
    EXPECT(w.waves >= 1 && w.waves <= 4);
    EXPECT(w.lds_bytes() == w.wave_bytes * (size_t)w.waves && w.lds_bytes() <= kBudget);
    EXPECT(w.threads() == 64u * (unsigned)w.waves);
  }
  {
    const WwShape a = lddl::native_ww_shape(128), b = lddl::native_ww_shape(4096);
    EXPECT(a.seqp == 128 && a.wave_bytes == 1048 && a.waves == 4);
    EXPECT(b.seqp == 4096 && b.wave_bytes == 33288 && b.waves == 1);
  }
  // ---- the walk tables: max(1, min(need_max, cap)); the global prefix iff need_max > cap ----
  for (int64_t cap : {lddl::kNativeLdsWordsCap, int64_t(64)}) {  // (64: what the GPU test sets)
    const struct { unsigned long long need; int32_t words; bool global; } cases[] = {
        {0, 1, false},
        {1, 1, false},
        {(unsigned long long)cap - 1, (int32_t)cap - 1, false},
        {(unsigned long long)cap, (int32_t)cap, false},
        {(unsigned long long)cap + 1, (int32_t)cap, true}};
    for (const auto& c : cases) {
      const WalkLds w = lddl::native_walk_lds(c.need, cap);
      EXPECT(w.words == c.words && w.global_prefix == c.global && w.bytes() == (size_t)4 * (size_t)c.words);
    }
  }
  {  // a cap of 0 (the knob's smallest value): one word, the global prefix for any partition
    const WalkLds w = lddl::native_walk_lds(5, 0);
    EXPECT(w.words == 1 && w.global_prefix);
    EXPECT(!lddl::native_walk_lds(0, 0).global_prefix);
  }
  printf("native_shape_check ok\n");
  return 0;
}
