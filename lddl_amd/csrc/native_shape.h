// The launch shapes of the native planner's three dynamic-LDS kernels (plan_native_kernel,
// pairs_native.hip; mask_native_kernel and mask_ww_native_kernel, pairs_native_mask.hip) as pure
// functions of the plan's parameters: the launch sites take every grid, block, LDS size and
// shape argument from here and compute none. (Host-only and free of the HIP runtime, like
// plan_split.h, so a CPU program can test it: tests/native_shape_check.cpp.)
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace lddl {

// dynamic LDS a mask workgroup asks for at most (a CU has 160 KB; up to 4 waves share the budget)
constexpr size_t kNativeMaskLds = 65536;
// LDS words of one partition's walk tables at most (96 KB per workgroup), unless
// LDDL_NATIVE_LDS_WORDS says otherwise; larger partitions read a global prefix
constexpr int64_t kNativeLdsWordsCap = 24576;

// plan_native_kernel: the walk tables of the largest partition take need_max words
// (native_part_need_kernel); the launch stages up to `cap` of them in LDS.
struct WalkLds {
  int32_t words;       // the kernel's lds_words: max(1, min(need_max, cap))
  bool global_prefix;  // some partition exceeds the cap: the global prefix must exist
  size_t bytes() const { return (size_t)4 * words; }
};
inline WalkLds native_walk_lds(unsigned long long need_max, int64_t cap) {
  return WalkLds{(int32_t)std::max<int64_t>(1, std::min<int64_t>((int64_t)need_max, cap)),
                 (int64_t)need_max > cap};
}

// mask_native_kernel. Per wave: the 64 lanes' bitmaps + the staged masks of its ppw pairs
// (<= max_pred each, 6 bytes a mask); up to 4 waves per workgroup within kNativeMaskLds. 64 pairs
// per wave while their staging fits that budget, else half as many until it does (seq 4096 at
// ratio 0.15: 8; one pair of 4096 masks, ratio 1.0, takes 56 KB). Sized for 64 pairs whatever the
// ratio, seq 512 at ratio 1.0 (196 KB) or seq 2500 at 0.15 would ask for more LDS than a CU has.
struct MaskShape {
  int32_t words;      // bitmap words per lane (NativeArgs::words)
  int32_t ppw;        // pairs per wave: a power of two, 1 .. 64
  int32_t stage_cap;  // staged masks per wave: ppw * max(max_pred, 1)
  size_t wave_bytes;  // LDS per wave
  int waves;          // per workgroup, 1 .. 4
  int64_t pairs_per_wg() const { return (int64_t)ppw * waves; }
  size_t lds_bytes() const { return wave_bytes * waves; }
  unsigned threads() const { return 64u * (unsigned)waves; }
  unsigned grid(int64_t n_pairs) const { return (unsigned)((n_pairs + pairs_per_wg() - 1) / pairs_per_wg()); }
};
inline MaskShape native_mask_shape(int32_t seq, int32_t max_pred) {
  MaskShape s;
  s.words = (seq + 31) / 32;
  const int32_t mp = std::max(max_pred, 1);
  auto wave_bytes = [&](int32_t pairs) { return (size_t)s.words * 64 * 4 + (size_t)pairs * mp * 6; };
  s.ppw = 64;
  while (s.ppw > 1 && wave_bytes(s.ppw) > kNativeMaskLds) s.ppw >>= 1;
  s.stage_cap = s.ppw * mp;
  s.wave_bytes = wave_bytes(s.ppw);
  s.waves = (int)std::max<size_t>(1, std::min<size_t>(4, kNativeMaskLds / s.wave_bytes));
  return s;
}

// mask_ww_native_kernel: one wave per pair; per wave an 8-byte entry per token of the longest
// pair (seq - 3, rounded up to whole windows) and a ballot per window + 1; up to 4 waves within
// kNativeMaskLds.
struct WwShape {
  int32_t seqp;       // tokens of the longest pair, in whole 64-token windows
  size_t wave_bytes;  // LDS per wave
  int waves;          // per workgroup (= pairs per workgroup), 1 .. 4
  size_t lds_bytes() const { return wave_bytes * waves; }
  unsigned threads() const { return 64u * (unsigned)waves; }
  unsigned grid(int64_t n_pairs) const { return (unsigned)((n_pairs + waves - 1) / waves); }
};
inline WwShape native_ww_shape(int32_t seq) {
  WwShape s;
  s.seqp = (seq - 3 + 63) / 64 * 64;
  s.wave_bytes = (size_t)8 * (s.seqp + s.seqp / 64 + 1);
  s.waves = (int)std::max<size_t>(1, std::min<size_t>(4, kNativeMaskLds / s.wave_bytes));
  return s;
}

}  // namespace lddl
