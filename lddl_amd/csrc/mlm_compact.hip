// Compact MLM targets from dense labels (past the reference): the masked slots of
// labels[R, L] (label != ignore_index) in position order, as fixed-shape device arrays, so that a
// training step gathers the MLM head's inputs without labels.nonzero() (a host wait and a shape
// that changes every step).
//
//   rows form: P slots per row      -> positions / ids / weights [R, P], num_masked [R]
//   flat form: `capacity` slots over labels.view(-1), ascending r * L + x
//                                   -> flat positions / ids [capacity], num_masked [R], total [1]
//
// One wave per row, kEncWaves rows per block, as in the collate kernels. A row is walked in
// 64-slot windows with lane = slot: the window's ballot(label != ignore) and the popcount of the
// lanes below give a masked slot's rank in its window, a wave-uniform running count carries the
// rank across windows. kWin windows are loaded before the first of their ballots, so no load
// waits for a popcount (the rank chain is scalar work on values already there). Every lane
// reaches every ballot; a lane past L loads the row's last slot and is predicated to ignore_index.
//
// The flat form needs the number of masked slots in the rows before a row: a count pass writes
// num_masked, then each wave of the write pass sums num_masked over all rows (the total) and over
// the rows before its own (its base). That is R / 64 loads per lane from a line set of 4 R bytes
// which every wave shares in L2: nothing beside the outputs is allocated, nothing waits for the
// host. Every element of every output is written exactly once per call.
#include "common.h"
#include "device.h"
#include "lddl_amd.h"

namespace lddl {
namespace {

constexpr int kEncWaves = 4;  // rows per block (collate_dev.h's house value)
constexpr int kWin = 4;       // 64-slot windows loaded ahead of their ballots

// Walks lab[0, L) with the whole wave; put(x, v, rank) runs in the lane of every masked slot x
// (label v), rank = number of masked slots before x in the row. Returns the row's count.
template <typename Put>
__device__ inline int32_t walk_row(const int64_t* __restrict__ lab, int64_t L, int64_t ignore,
                                   Put put) {
  const int lane = lane_id();
  int32_t n = 0;
  for (int64_t w0 = 0; w0 < L; w0 += 64 * kWin) {  // L < 2^31: n fits
    int64_t v[kWin];
#pragma unroll
    for (int u = 0; u < kWin; ++u) {
      const int64_t x = w0 + 64 * u + lane;
      const int64_t t = lab[x < L ? x : L - 1];  // clamped, not branched: the loads stay together
      v[u] = x < L ? t : ignore;
    }
#pragma unroll
    for (int u = 0; u < kWin; ++u) {
      const bool masked = v[u] != ignore;
      const uint64_t m = ballot(masked);
      if (masked) put(w0 + 64 * u + lane, v[u], n + (int32_t)popc_below(m));
      n += __popcll(m);
    }
  }
  return n;
}

__global__ void __launch_bounds__(64 * kEncWaves) mlm_compact_rows_kernel(
    const int64_t* __restrict__ labels, int64_t R, int64_t L, int64_t ignore, int64_t P,
    int64_t* __restrict__ positions, int64_t* __restrict__ ids, float* __restrict__ weights,
    int32_t* __restrict__ num_masked) {
  const int64_t row = (int64_t)blockIdx.x * kEncWaves + wave_id();
  if (row >= R) return;
  const int64_t o = row * P;
  const int32_t n = walk_row(labels + row * L, L, ignore, [&](int64_t x, int64_t v, int32_t rank) {
    if (rank < P) {  // on overflow the first P in position order stay
      positions[o + rank] = x;
      ids[o + rank] = v;
      weights[o + rank] = 1.0f;
    }
  });
  for (int64_t j = (n < P ? n : P) + lane_id(); j < P; j += 64) {
    positions[o + j] = 0;
    ids[o + j] = ignore;
    weights[o + j] = 0.0f;
  }
  if (lane_id() == 0) num_masked[row] = n;
}

__global__ void __launch_bounds__(64 * kEncWaves) mlm_count_rows_kernel(
    const int64_t* __restrict__ labels, int64_t R, int64_t L, int64_t ignore,
    int32_t* __restrict__ num_masked) {
  const int64_t row = (int64_t)blockIdx.x * kEncWaves + wave_id();
  if (row >= R) return;
  const int32_t n = walk_row(labels + row * L, L, ignore, [](int64_t, int64_t, int32_t) {});
  if (lane_id() == 0) num_masked[row] = n;
}

__global__ void __launch_bounds__(64 * kEncWaves) mlm_compact_flat_kernel(
    const int64_t* __restrict__ labels, int64_t R, int64_t L, int64_t ignore, int64_t capacity,
    const int32_t* __restrict__ num_masked, int64_t* __restrict__ positions,
    int64_t* __restrict__ ids, int64_t* __restrict__ total) {
  const int64_t row = (int64_t)blockIdx.x * kEncWaves + wave_id();
  if (row >= R) return;
  int64_t before = 0, all = 0;
  for (int64_t i0 = lane_id(); i0 < R + lane_id(); i0 += 64 * kWin) {  // kWin loads in flight
    int32_t c[kWin];
#pragma unroll
    for (int u = 0; u < kWin; ++u) {
      const int64_t i = i0 + 64 * u;
      c[u] = num_masked[i < R ? i : R - 1];
    }
#pragma unroll
    for (int u = 0; u < kWin; ++u) {
      const int64_t i = i0 + 64 * u;
      all += i < R ? c[u] : 0;
      before += i < row ? c[u] : 0;
    }
  }
  before = wave_sum(before);
  all = wave_sum(all);
  const int64_t flat0 = row * L;
  walk_row(labels + flat0, L, ignore, [&](int64_t x, int64_t v, int32_t rank) {
    const int64_t dst = before + rank;
    if (dst < capacity) {  // on overflow the first `capacity` in flat order stay
      positions[dst] = flat0 + x;
      ids[dst] = v;
    }
  });
  // the padding [min(total, capacity), capacity) is dealt over the waves, 64 slots at a time
  for (int64_t j = (all < capacity ? all : capacity) + row * 64 + lane_id(); j < capacity;
       j += R * 64) {
    positions[j] = 0;
    ids[j] = ignore;
  }
  if (row == 0 && lane_id() == 0) *total = all;
}

// the flat form of a batch without rows: all padding, total 0
__global__ void __launch_bounds__(256) mlm_pad_flat_kernel(int64_t ignore, int64_t capacity,
                                                           int64_t* __restrict__ positions,
                                                           int64_t* __restrict__ ids,
                                                           int64_t* __restrict__ total) {
  const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (int64_t j = i0; j < capacity; j += (int64_t)gridDim.x * 256) {
    positions[j] = 0;
    ids[j] = ignore;
  }
  if (i0 == 0) *total = 0;
}

constexpr int64_t kMaxBlocks = 0x7FFFFFFF;

}  // namespace
}  // namespace lddl

using namespace lddl;

extern "C" int lddl_mlm_compact_rows(void* stream, const int64_t* d_labels, int64_t R, int64_t L,
                                     int64_t ignore_index, int64_t P, int64_t* d_positions,
                                     int64_t* d_ids, float* d_weights, int32_t* d_num_masked) {
  if (!d_labels || !d_positions || !d_ids || !d_weights || !d_num_masked)
    LDDL_FAIL(-1, "lddl_mlm_compact_rows: null pointer");
  if (R < 0 || L < 0) LDDL_FAIL(-1, "lddl_mlm_compact_rows: R %lld, L %lld: negative size",
                                (long long)R, (long long)L);
  if (P < 1) LDDL_FAIL(-1, "lddl_mlm_compact_rows: P %lld < 1", (long long)P);
  if (L > 0x7FFFFFFF) LDDL_FAIL(-1, "lddl_mlm_compact_rows: L %lld > 2^31 - 1", (long long)L);
  const int64_t blocks = (R + kEncWaves - 1) / kEncWaves;
  if (blocks > kMaxBlocks) LDDL_FAIL(-1, "lddl_mlm_compact_rows: R %lld too large", (long long)R);
  if (R == 0) return 0;
  hipLaunchKernelGGL(mlm_compact_rows_kernel, dim3((unsigned)blocks), dim3(64 * kEncWaves), 0,
                     reinterpret_cast<hipStream_t>(stream), d_labels, R, L, ignore_index,
                     P, d_positions, d_ids, d_weights, d_num_masked);
  LDDL_HIP(hipGetLastError());
  return 0;
}

extern "C" int lddl_mlm_compact_flat(void* stream, const int64_t* d_labels, int64_t R, int64_t L,
                                     int64_t ignore_index, int64_t capacity,
                                     int64_t* d_flat_positions, int64_t* d_flat_ids,
                                     int32_t* d_num_masked, int64_t* d_total) {
  if (!d_labels || !d_flat_positions || !d_flat_ids || !d_num_masked || !d_total)
    LDDL_FAIL(-1, "lddl_mlm_compact_flat: null pointer");
  if (R < 0 || L < 0) LDDL_FAIL(-1, "lddl_mlm_compact_flat: R %lld, L %lld: negative size",
                                (long long)R, (long long)L);
  if (capacity < 1) LDDL_FAIL(-1, "lddl_mlm_compact_flat: capacity %lld < 1", (long long)capacity);
  if (L > 0x7FFFFFFF) LDDL_FAIL(-1, "lddl_mlm_compact_flat: L %lld > 2^31 - 1", (long long)L);
  const int64_t blocks = (R + kEncWaves - 1) / kEncWaves;
  if (blocks > kMaxBlocks) LDDL_FAIL(-1, "lddl_mlm_compact_flat: R %lld too large", (long long)R);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (R == 0) {
    const int64_t pad_blocks = (capacity + 255) / 256;
    hipLaunchKernelGGL(mlm_pad_flat_kernel, dim3((unsigned)(pad_blocks < 2048 ? pad_blocks : 2048)),
                       dim3(256), 0, st, ignore_index, capacity, d_flat_positions, d_flat_ids,
                       d_total);
    LDDL_HIP(hipGetLastError());
    return 0;
  }
  hipLaunchKernelGGL(mlm_count_rows_kernel, dim3((unsigned)blocks), dim3(64 * kEncWaves), 0, st,
                     d_labels, R, L, ignore_index, d_num_masked);
  hipLaunchKernelGGL(mlm_compact_flat_kernel, dim3((unsigned)blocks), dim3(64 * kEncWaves), 0, st,
                     d_labels, R, L, ignore_index, capacity, d_num_masked,
                     d_flat_positions, d_flat_ids, d_total);
  LDDL_HIP(hipGetLastError());
  return 0;
}
