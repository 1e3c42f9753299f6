// The row plan of sequence packing on the device: torch/seqpack.py's plan_rows,
// first-fit decreasing, for every batch of a round in one launch. The online loader's lengths
// live on the device and it has no workers, so the plan is made where the lengths are.
//
// One wave per batch (a block is one wave), at most kSeqPlanMaxBatch samples per batch:
//   1. the lengths go to LDS (sample i of the batch = rows[b0 + i]);
//   2. every sample's stable descending rank: the samples before it are those that are longer,
//      or as long with a lower index. Lane l ranks samples l, l + 64, ... against broadcast reads
//      of all lengths; the sorted (index, length) lists go to LDS;
//   3. the serial first-fit. Row r's free slots and sample count are held by lane r & 63 in
//      register r >> 6 (arrays indexed only by unrolled constants: no scratch). Every row starts
//      with `capacity` free, opened or not, so "the lowest open row with room, else a new row" is
//      the lowest row with room: one ballot per group of 64 rows and a trailing-zero count. g0,
//      wave-uniform, is the first group in which some row still takes the shortest sample: the
//      groups below it are skipped. The sorted lists are read 64 at a time into registers and
//      handed out by readlane, so no LDS read sits on the serial chain;
//   4. a wave scan over the rows' sample counts gives every row's first position in (row, start)
//      order, and a last pass over the samples writes the outputs.
// A wave is alone on its chain, so what it issues is what it costs: steps 2 to 4 are compiled
// for 1, 2, 4, 8 and 16 groups of 64 samples (and rows: R <= B), and a batch runs the smallest
// that holds it.
#include "common.h"
#include "ctx.h"
#include "device.h"
#include "lddl_amd.h"

namespace lddl {
namespace {

constexpr int kSeqPlanMaxBatch = LDDL_SEQPLAN_MAX_BATCH;
static_assert(kSeqPlanMaxBatch == 1024, "plan_kernel dispatches to 1 .. 16 groups of 64");

struct PlanArgs {
  const int32_t* num_tokens;  // nullable: then tok_off
  const int64_t* tok_off;
  const int64_t* rows;  // nullable: identity
  int64_t n_rows;
  const int64_t* batch_off;  // [n_batches + 1]
  int32_t capacity;
  int64_t* dst;
  int32_t* fill;
  int32_t* seq_in_row;
  int32_t* packed_idx;
  int32_t* num_rows;
};

// the wave's LDS, kSeqPlanMaxBatch words each
struct Lds {
  int32_t* len;    // by sample
  int32_t* ord;    // by rank: the sample
  int32_t* slen;   // by rank: its length
  int32_t* row;    // by sample (-1: takes no row)
  int32_t* start;
  int32_t* seq;
  int32_t* free;   // by row
  int32_t* cnt;
  int32_t* base;
};

// steps 2 to 4 for a batch of B <= NG * 64 samples whose lengths are in S.len
template <int NG>
__device__ void plan_batch(const PlanArgs& P, const Lds& S, int64_t k, int64_t b0, int32_t B,
                           int lane) {
  const int32_t cap = P.capacity;
  // 2. stable descending ranks
  {
    int32_t mine[NG], rank[NG];
#pragma unroll
    for (int G = 0; G < NG; ++G) {
      const int32_t i = G * 64 + lane;
      mine[G] = i < B ? S.len[i] : 0;
      rank[G] = 0;
    }
#pragma unroll 4
    for (int32_t j = 0; j < B; ++j) {
      const int32_t lj = S.len[j];  // broadcast
#pragma unroll
      for (int G = 0; G < NG; ++G)
        rank[G] += (lj > mine[G] || (lj == mine[G] && j < G * 64 + lane)) ? 1 : 0;
    }
#pragma unroll
    for (int G = 0; G < NG; ++G) {
      const int32_t i = G * 64 + lane;
      if (i < B) {
        S.ord[rank[G]] = i;
        S.slen[rank[G]] = mine[G];
      }
    }
  }
  wave_sync();

  // 3. first fit over the sorted samples
  int32_t free_[NG], cnt[NG];
#pragma unroll
  for (int G = 0; G < NG; ++G) {
    free_[G] = cap;
    cnt[G] = 0;
  }
  const int32_t minlen = B ? __builtin_amdgcn_readfirstlane(S.slen[B - 1]) : 0;
  int32_t R = 0, g0 = 0;
  for (int32_t k0 = 0; k0 < B; k0 += 64) {
    const int32_t kk = k0 + lane;
    const int32_t v_ord = kk < B ? S.ord[kk] : 0, v_len = kk < B ? S.slen[kk] : 0;
    const int32_t m = min(64, B - k0);
    for (int32_t j = 0; j < m; ++j) {
      const int32_t i = __builtin_amdgcn_readlane(v_ord, j);
      const int32_t n = __builtin_amdgcn_readlane(v_len, j);
      if (n > cap) continue;  // takes no row: S.row[i] stays -1
      // row R, still unopened, takes n: the search ends at or before its group (R < B)
#pragma unroll
      for (int G = 0; G < NG; ++G) {
        if (G < g0) continue;
        const uint64_t fits = ballot(free_[G] >= n);
        if (fits) {
          const int l = __builtin_ctzll(fits);
          if (lane == l) {
            S.row[i] = G * 64 + l;
            S.start[i] = cap - free_[G];
            S.seq[i] = ++cnt[G];
            free_[G] -= n;
          }
          R = max(R, G * 64 + l + 1);
          break;
        }
        // nothing that is still to come fits a row of this group
        if (G == g0 && !ballot(free_[G] >= minlen)) g0 = G + 1;
      }
    }
  }

  // 4. rows -> first position in (row, start) order; outputs
  int32_t run = 0;
#pragma unroll
  for (int G = 0; G < NG; ++G) {
    const int32_t incl = wave_incl_scan(cnt[G]);
    S.free[G * 64 + lane] = free_[G];
    S.cnt[G * 64 + lane] = cnt[G];
    S.base[G * 64 + lane] = run + incl - cnt[G];
    run += __builtin_amdgcn_readlane(incl, 63);
  }
  wave_sync();
  for (int32_t i = lane; i < B; i += 64) {
    const int32_t r = S.row[i];
    int64_t dst = -1;
    int32_t fill = 0, seq = 0, at = -1;
    if (r >= 0) {
      seq = S.seq[i];
      dst = (int64_t)r * cap + S.start[i];
      fill = S.len[i] + (seq == S.cnt[r] ? S.free[r] : 0);  // the row's last sample: its tail
      at = S.base[r] + seq - 1;
    }
    P.dst[b0 + i] = dst;
    P.fill[b0 + i] = fill;
    P.seq_in_row[b0 + i] = seq;
    P.packed_idx[b0 + i] = at;
  }
  if (lane == 0) P.num_rows[k] = R;
}

__global__ void __launch_bounds__(64) plan_kernel(PlanArgs P) {
  __shared__ int32_t s_mem[9][kSeqPlanMaxBatch];
  const Lds S{s_mem[0], s_mem[1], s_mem[2], s_mem[3], s_mem[4], s_mem[5], s_mem[6], s_mem[7],
              s_mem[8]};
  const int lane = threadIdx.x;
  const int64_t k = blockIdx.x;
  const int64_t b0 = P.batch_off[k], b1 = P.batch_off[k + 1];
  // the host cannot see the offsets without a wait: a range outside the arrays writes nothing but
  // num_rows = -1, a batch past the bound also marks its samples as taking no row
  if (b0 < 0 || b1 < b0 || b1 > P.n_rows) {
    if (lane == 0) P.num_rows[k] = -1;
    return;
  }
  if (b1 - b0 > kSeqPlanMaxBatch) {
    for (int64_t i = b0 + lane; i < b1; i += 64) {
      P.dst[i] = -1;
      P.fill[i] = 0;
      P.seq_in_row[i] = 0;
      P.packed_idx[i] = -1;
    }
    if (lane == 0) P.num_rows[k] = -1;
    return;
  }
  const int32_t B = (int32_t)(b1 - b0);

  // 1. lengths
  for (int32_t i = lane; i < B; i += 64) {
    const int64_t r = P.rows ? P.rows[b0 + i] : b0 + i;
    S.len[i] = P.num_tokens ? P.num_tokens[r] : (int32_t)(P.tok_off[r + 1] - P.tok_off[r]) + 3;
    S.row[i] = -1;
  }
  wave_sync();
  if (B <= 64) plan_batch<1>(P, S, k, b0, B, lane);
  else if (B <= 128) plan_batch<2>(P, S, k, b0, B, lane);
  else if (B <= 256) plan_batch<4>(P, S, k, b0, B, lane);
  else if (B <= 512) plan_batch<8>(P, S, k, b0, B, lane);
  else plan_batch<16>(P, S, k, b0, B, lane);
}

}  // namespace
}  // namespace lddl

using namespace lddl;

extern "C" int lddl_seqpack_plan(lddl_ctx* c, void* stream, const int32_t* d_num_tokens,
                                 const int64_t* d_tok_off, const int64_t* d_rows, int64_t n_rows,
                                 const int64_t* d_batch_off, int32_t n_batches, int32_t capacity,
                                 int64_t* d_dst, int32_t* d_fill, int32_t* d_seq_in_row,
                                 int32_t* d_packed_idx, int32_t* d_num_rows) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  if (n_batches <= 0) return 0;
  if (!d_num_tokens && !d_tok_off) LDDL_FAIL(-1, "null lengths: num_tokens or tok_off is needed");
  if (!d_batch_off) LDDL_FAIL(-1, "null batch offsets");
  if (!d_dst || !d_fill || !d_seq_in_row || !d_packed_idx || !d_num_rows)
    LDDL_FAIL(-1, "null output");
  if (capacity < 1) LDDL_FAIL(-1, "capacity %d < 1", capacity);
  if (n_rows < 0) LDDL_FAIL(-1, "n_rows %lld < 0", (long long)n_rows);
  // the batches tile [0, n_rows): more rows than n_batches full batches means one is too large
  if (n_rows > (int64_t)n_batches * kSeqPlanMaxBatch)
    LDDL_FAIL(-1, "%lld samples in %d batches: a batch of more than %d samples is unsupported",
              (long long)n_rows, n_batches, kSeqPlanMaxBatch);
  PlanArgs P{d_num_tokens, d_tok_off, d_rows, n_rows, d_batch_off, capacity, d_dst, d_fill,
             d_seq_in_row, d_packed_idx, d_num_rows};
  hipLaunchKernelGGL(plan_kernel, dim3((unsigned)n_batches), dim3(64), 0, as_stream(stream), P);
  LDDL_HIP(hipGetLastError());
  return 0;
}
