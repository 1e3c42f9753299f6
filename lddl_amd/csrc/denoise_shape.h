// The launch shape of denoise_kernel (denoise.hip) as a pure function of the batch:
// the launch site takes grid, block and LDS size from here and computes none. (Host-only and
// free of the HIP runtime, like native_shape.h, so a CPU program can check it.)
#pragma once
#include <cstddef>
#include <cstdint>

namespace lddl {

// Units of a sample (LDDL_DENOISE_MAX_UNITS): a sentence each, the last one the tail. Four int32
// tables of kDenoiseStride entries per wave, 4224 bytes: a workgroup of four waves asks for
// 16.5 KB, so nine of them fit a CU's 160 KB and LDS never caps the waves of a CU below the
// eight per SIMD its registers allow. 512 units would halve that for documents of more than 255
// sentences inside one row, which the tail unit serves.
constexpr int kDenoiseUnits = 256;
constexpr int kDenoiseStride = kDenoiseUnits + 8;  // one entry past the last unit, 32-byte rows
constexpr int kDenoiseTables = 4;                  // opos, ppos (participants first), pkey, order
constexpr int kDenoiseWaves = 4;                   // waves (= samples) per workgroup

struct DenoiseShape {
  int waves;          // per workgroup
  size_t wave_bytes;  // LDS per wave
  unsigned grid;      // workgroups
  size_t lds_bytes() const { return wave_bytes * waves; }
  unsigned threads() const { return 64u * (unsigned)waves; }
};
inline DenoiseShape denoise_shape(int32_t batch) {
  DenoiseShape s;
  s.waves = kDenoiseWaves;
  s.wave_bytes = sizeof(int32_t) * kDenoiseTables * kDenoiseStride;
  s.grid = batch > 0 ? (unsigned)(((int64_t)batch + s.waves - 1) / s.waves) : 0u;
  return s;
}

}  // namespace lddl
