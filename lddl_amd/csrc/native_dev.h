// What the native planner's units share on the device (pairs_native.hip, pairs_native_mask.hip):
// the keyed Philox streams (part_key, the stream ids, CtrRng, token_rng), the kernels' arguments
// (NativeArgs) and two helpers of the masking (win_token, lemire_below). Each translation unit
// gets its own copy (anonymous namespace).
#pragma once
#include "pairs_plan.h"

namespace lddl {

// The native kernels' arguments (in namespace lddl proper, like PlanArgs: the type appears in the
// signature of launch_native_masks, which crosses units)
struct NativeArgs {
  const int32_t* ks_len;
  const int64_t* kd_off;
  const int64_t* kp_off;
  const int64_t* kscan;
  IdPtr dense;
  const int64_t* part_seed;
  int64_t n_part, n_units, unit0;  // units dup * (kp_off[0] .. kp_off[n_part])
  uint64_t native_seed, k_short;
  int32_t seq, dup, masking, cls_id, sep_id, mask_id, vocab_size;
  double ratio;
  int64_t* ucnt;        // count pass: pairs of each (duplicate, document) unit
  const int64_t* uoff;  // emit pass: first pair of each unit (exclusive scan of ucnt)
  const int64_t* part_base;
  PairDesc* desc;
  int32_t* nmask;
  int32_t* ncand;
  int32_t* ppart;
  const int64_t* moff;
  uint16_t* mpos;
  int32_t* mtok;
  int64_t* src;
  int64_t n_pairs;
  int32_t words;  // bitmap words per lane (mask kernel)
};

namespace {

// ---------------------------------------------------------------------------------------------
// Native RNG mode (LDDL_RNG_NATIVE): the same algorithms (create_pairs_from_document,
// _truncate_seq_pair, create_masked_lm_predictions, the partition shuffle) drawing from
// Philox4x32-10 instead of one sequential MT19937 per partition, so every (duplicate, document)
// walk and every pair's masking runs in its own lane. A stream is keyed by
// (native_seed, part_seed[p]) and counted by the unit's or pair's index inside its partition, so
// a partition's output does not depend on how partitions are batched or sharded.
// Distributions are those of the reference: in the walk, randint / _randbelow by the same
// bit-length rejection and random() < p on the same 53-bit integer, each truncation side a fair
// coin; in the masking, the masked set a uniform num_to_predict-subset of the candidates (Floyd's
// algorithm: the shuffled prefix of pretrain.py:197-207 is a uniform subset) and 80/10/10
// decisions per masked token, both from one 32-bit draw each (exact uniform integers by Lemire's
// multiply-shift with rejection).
// ---------------------------------------------------------------------------------------------
__device__ inline uint64_t mix64(uint64_t x) {  // splitmix64 finaliser
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__device__ inline uint64_t part_key(uint64_t native_seed, int64_t part_seed) {
  return mix64(native_seed ^ mix64((uint64_t)part_seed + 0x9E3779B97F4A7C15ull));
}

enum : uint32_t { kStreamWalk = 1, kStreamMask = 2, kStreamOrder = 3, kStreamDecide = 4 };
// streams of the whole-word path (CtrRng keeps 4 bits for the stream id)
enum : uint32_t { kStreamWordKey = 5, kStreamWordDecide = 6 };

struct CtrRng {
  uint2 key;
  uint32_t id0, id1, blk;
  uint4 buf;
  int have;
  __device__ CtrRng(uint64_t k, int64_t index, uint32_t stream)
      : key{(uint32_t)k, (uint32_t)(k >> 32)},
        id0((uint32_t)index),
        id1((uint32_t)((uint64_t)index >> 32) << 4 | stream),
        blk(0),
        have(0) {}
  __device__ uint32_t u32() {
    if (have == 0) {
      buf = Philox::gen(make_uint4(blk++, id0, id1, 0x6C64646Cu), key);
      have = 4;
    }
    --have;
    return have == 3 ? buf.x : have == 2 ? buf.y : have == 1 ? buf.z : buf.w;
  }
  __device__ uint64_t rand53() {  // the 53-bit integer behind random()
    const uint32_t a = u32() >> 5, b = u32() >> 6;
    return ((uint64_t)a << 26) | b;
  }
  __device__ bool coin() { return u32() < 0x80000000u; }
  __device__ uint32_t randbelow(uint32_t n) {  // _randbelow: k-bit draws until < n
    const int k = 32 - __clz(n);
    uint32_t r = u32() >> (32 - k);
    while (r >= n) r = u32() >> (32 - k);
    return r;
  }
  __device__ int64_t randint(int64_t a, int64_t b) { return a + randbelow((uint32_t)(b - a + 1)); }
  __device__ int32_t heads(int32_t n) {  // number of heads in n fair coins
    int32_t h = 0;
    for (; n >= 32; n -= 32) h += __popc(u32());
    if (n > 0) h += __popc(u32() & ((1u << n) - 1u));
    return h;
  }
};

// token t of the window [front, front + n) of the span starting at kept sentence k
__device__ inline int32_t win_token(const NativeArgs& A, int64_t k, int32_t front, int32_t t) {
  return A.dense.ld(A.kscan[k] + front + t);
}

// Uniform integer in [0, n) from a 32-bit draw: Lemire's multiply-shift with the exact rejection
// (taken with probability < n / 2^32, so the lanes of a wave stay in step).
__device__ inline uint32_t lemire_below(uint32_t x, uint32_t n, CtrRng& rng) {
  uint64_t m = (uint64_t)x * n;
  if ((uint32_t)m < n) {
    const uint32_t t = (0u - n) % n;
    while ((uint32_t)m < t) m = (uint64_t)rng.u32() * n;
  }
  return (uint32_t)(m >> 32);
}

// The draws that belong to token t of a pair: Philox blocks (t << 16) + 0, 1, .. of the pair's
// stream (t < 65536: check_plan_args bounds seq), so no two tokens share a block.
__device__ inline CtrRng token_rng(uint64_t key, int64_t pair_index, uint32_t stream, int32_t t) {
  CtrRng r(key, pair_index, stream);
  r.blk = (uint32_t)t << 16;
  return r;
}

}  // namespace

// pairs_native_mask.hip: the masks of the plan's A.n_pairs pairs, by mask_native_kernel or (whole
// word) mask_ww_native_kernel, on the planning stream; sets A.words
void launch_native_masks(const lddl_pairs* P, const PlanWork& W, NativeArgs& A);

}  // namespace lddl
