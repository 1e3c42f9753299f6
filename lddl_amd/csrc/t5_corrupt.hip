// T5 span corruption (include/lddl_amd.h states the semantics): output row i is
// block rows[i] of lddl_blocks_plan with exactly N of its n tokens noised in exactly k spans,
// written as the encoder input (the clean segments, a sentinel behind each) and the target (a
// sentinel and the noise behind it). One wave per row, kEncWaves rows per workgroup, no
// block-wide barrier, no global atomics, no temporaries, integer arithmetic only.
//
//   table    the wave stages rel[j] = P[s0 + j] - P[s0], j <= min(S, kBlkLdsSents), in LDS, as
//            blocks_kernel does; t5_token is that kernel's lookup
//   select   the k - 1 smallest of the N - 1 noise keys and of the M - 1 non-noise keys, both
//            sides in lock-step from one Philox call per item: three passes over u, 64 a
//            window, one 8-bit digit each from the top. A lane whose key matches the prefix
//            found so far adds 1 to its digit's bin (ds_add, 256 bins a side); t5_pick scans the
//            bins for the digit of rank k - 1 and carries the rank into the bin. The keys are
//            drawn again in every pass and never stored, so a row's length is not bounded by
//            LDS. Behind the third pass a side has its threshold key and `rem`, the number of
//            items equal to it that are still taken. k = 1 selects nothing and skips all of it
//   starts   one more pass: an item opens a segment iff key < threshold, or key == threshold
//            and fewer than rem equal items lie before it (ballot, popc_below and a wave-uniform
//            carry: the tie goes to the lower position); a second ballot and carry number the
//            selected items, and the lane writes its item to A[h] or Bn[g]
//   emit     by output slot, so the stores coalesce: input slot y bisects A[h] + h, target slot
//            z bisects Bn[g] + g (t5_locate); the slot is a sentinel or an item whose position
//            in the block follows from the other table, and t5_token reads it. The lane of
//            labels[z] also writes decoder_input_ids[z + 1]
//
// Every output element is written exactly once; every lane reaches every ballot, scan and
// shuffle (the counts are wave-uniform), the tails are predicated.
#include "common.h"
#include "ctx.h"
#include "t5_dev.h"

namespace lddl {
namespace {

__global__ void __launch_bounds__(64 * kEncWaves) t5_kernel(T5Args A) {
  __shared__ T5Wave lds[kEncWaves];
  const int w = wave_id(), lane = lane_id();
  const int32_t b = blockIdx.x * kEncWaves + w;
  if (b >= A.B) return;  // the whole wave; no block-wide barrier below
  T5Wave& W = lds[w];
  const int64_t blk = A.rows ? A.rows[b] : (int64_t)b;
  const int64_t s0 = A.block_sent[blk], s1 = A.block_sent[blk + 1];
  const int64_t S = s1 - s0, p0 = A.P[s0];
  const int32_t T = A.L - 2;
  const int64_t n64 = A.P[s1] - p0;  // the plan keeps a block within T
  const int32_t n = (int32_t)(n64 < 0 ? 0 : (n64 < T ? n64 : T));
  const int32_t U = (int32_t)(S < kBlkLdsSents ? (S < 0 ? 0 : S) : kBlkLdsSents);
  for (int32_t j = lane; j <= U; j += 64) {
    const int64_t r = A.P[s0 + j] - p0;
    W.rel[j] = (int32_t)(r < T + 1 ? r : T + 1);  // every q is below T: the clip orders the same
  }
  const T5Block K{W.rel, U, s0, s1, p0};

  int32_t N, k;
  t5_counts(n, A.dq, A.iq, A.n_sentinels, &N, &k);
  const int32_t M = n - N, kk = k > 0 ? k : 1;  // k = 0 (n < 2): one clean segment, no sentinel
  const int32_t cn = N - 1, cm = M - 1;          // the items of a side that have a key: 1 ..
  const int32_t cu = cn > cm ? cn : cm;
  const int64_t flat = (int64_t)b * A.L;

  // ---- select: the threshold key of a side and how many items equal to it are taken ----------
  uint32_t key_n = 0, key_m = 0, rem_n = 0, rem_m = 0;
  if (k > 1) {
    rem_n = rem_m = (uint32_t)(k - 1);
    for (int shift = 16; shift >= 0; shift -= 8) {
      *reinterpret_cast<uint4*>(&W.hist[0][4 * lane]) = make_uint4(0, 0, 0, 0);
      *reinterpret_cast<uint4*>(&W.hist[1][4 * lane]) = make_uint4(0, 0, 0, 0);
      wave_sync();
      for (int32_t u0 = 0; u0 < cu; u0 += 64) {
        const int32_t u = u0 + lane;
        const uint4 r = mask_draw(A.draw, flat + u);
        const uint32_t kn = r.x >> 8, km = r.y >> 8;
        if (u < cn && (kn >> (shift + 8)) == key_n)
          __hip_atomic_fetch_add(&W.hist[0][(kn >> shift) & 255u], 1u, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WAVEFRONT);
        if (u < cm && (km >> (shift + 8)) == key_m)
          __hip_atomic_fetch_add(&W.hist[1][(km >> shift) & 255u], 1u, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WAVEFRONT);
      }
      wave_sync();
      key_n = (key_n << 8) | t5_pick(W.hist[0], lane, rem_n);
      key_m = (key_m << 8) | t5_pick(W.hist[1], lane, rem_m);
      wave_sync();  // the bins are read before the next pass clears them
    }
  }

  // ---- starts: A[h], Bn[g] = the first item of non-noise segment h, noise segment g -----------
  if (lane == 0) {
    W.A[0] = 0;
    W.Bn[0] = 0;
    W.A[kk] = M;
    W.Bn[kk] = N;
  }
  if (k > 1) {
    uint32_t eq_n = 0, eq_m = 0, sel_n = 0, sel_m = 0;  // the carries between windows
    for (int32_t u0 = 0; u0 < cu; u0 += 64) {
      const int32_t u = u0 + lane;
      const uint4 r = mask_draw(A.draw, flat + u);
      const uint32_t kn = r.x >> 8, km = r.y >> 8;
      const bool en = u < cn && kn == key_n, em = u < cm && km == key_m;
      const uint64_t ben = ballot(en), bem = ballot(em);
      const bool sn = u < cn && (kn < key_n || (en && eq_n + popc_below(ben) < rem_n));
      const bool sm = u < cm && (km < key_m || (em && eq_m + popc_below(bem) < rem_m));
      const uint64_t bsn = ballot(sn), bsm = ballot(sm);
      const uint32_t g = sel_n + popc_below(bsn) + 1, h = sel_m + popc_below(bsm) + 1;
      if (sn && g < (uint32_t)k) W.Bn[g] = u + 1;
      if (sm && h < (uint32_t)k) W.A[h] = u + 1;
      eq_n += __popcll(ben);
      eq_m += __popcll(bem);
      sel_n += __popcll(bsn);
      sel_m += __popcll(bsm);
    }
  }
  wave_sync();

  // ---- emit ----------------------------------------------------------------------------------
  const int32_t src_len = M + k + 1, tgt_len = N + k + 1;
  if (lane == 0) {
    A.src_lengths[b] = src_len;
    A.tgt_lengths[b] = tgt_len;
  }
  // the eos slot: behind the row, or the last slot of a row that is too narrow
  const int32_t last_y = (src_len < A.in_len ? src_len : A.in_len) - 1;
  const int32_t last_z = (tgt_len < A.tgt_len ? tgt_len : A.tgt_len) - 1;
  const int64_t irow = (int64_t)b * A.in_len, trow = (int64_t)b * A.tgt_len;
  for (int32_t y0 = 0; y0 < A.in_len; y0 += 64) {
    const int32_t y = y0 + lane;
    int64_t id = y == last_y ? A.eos : A.pad;
    if (y < last_y) {
      const int32_t h = t5_locate(W.A, kk, y), m = y - h;
      const int32_t q = m + W.Bn[h];
      id = A.sentinel_first - h;  // the slot behind the segment, unless m is one of its items
      if (m < W.A[h + 1]) id = q < n ? t5_token(A, K, q) : A.pad;
    }
    if (y < A.in_len) {
      A.input_ids[irow + y] = id;
      A.attention_mask[irow + y] = y <= last_y ? 1 : 0;
    }
  }
  for (int32_t z0 = 0; z0 < A.tgt_len; z0 += 64) {
    const int32_t z = z0 + lane;
    int64_t id = z == last_z ? A.eos : A.ignore_index;
    if (z < last_z) {
      const int32_t g = t5_locate(W.Bn, kk, z), j = z - g - 1;
      const int32_t q = j + W.A[g + 1];
      id = A.sentinel_first - g;  // the slot before the segment, unless j is one of its items
      if (j >= W.Bn[g]) id = q < n ? t5_token(A, K, q) : A.pad;
    }
    if (z < A.tgt_len) {
      A.labels[trow + z] = id;
      if (z == 0) A.decoder_input_ids[trow] = A.dec_start;
      if (z + 1 < A.tgt_len) A.decoder_input_ids[trow + z + 1] = z <= last_z ? id : A.pad;
    }
  }
}

// the refusals the two entry points share
int t5_check(int64_t plan_seq_len, int64_t in_len, int64_t tgt_len, int32_t dq, int32_t iq,
             int32_t n_sentinels, int64_t sentinel_first) {
  if (plan_seq_len < 3 || plan_seq_len > (1 << 24))
    LDDL_FAIL(-1, "plan seq_len %lld: a block holds a piece at least, 2^24 slots at most",
              (long long)plan_seq_len);
  if (in_len < 1 || in_len > (1 << 24) || tgt_len < 1 || tgt_len > (1 << 24))
    LDDL_FAIL(-1, "in_len %lld or tgt_len %lld outside [1, 2^24]", (long long)in_len,
              (long long)tgt_len);
  if (dq < 1 || dq > 65535) LDDL_FAIL(-1, "dq %d: the noise density lies inside (0, 1)", dq);
  if (iq < 1 || iq > 65536)
    LDDL_FAIL(-1, "iq %d: the mean noise span length lies in [1, 65536]", iq);
  if (n_sentinels < 1 || n_sentinels > LDDL_T5_MAX_SPANS)
    LDDL_FAIL(-1, "n_sentinels %d outside [1, %d]", n_sentinels, LDDL_T5_MAX_SPANS);
  if (sentinel_first - n_sentinels + 1 < 0)
    LDDL_FAIL(-1, "sentinel_first %lld: the last of %d sentinels would be negative",
              (long long)sentinel_first, n_sentinels);
  return 0;
}

}  // namespace
}  // namespace lddl

using namespace lddl;

extern "C" int lddl_t5_lengths(int64_t tokens, int32_t dq, int32_t iq, int32_t n_sentinels,
                               int64_t* in_len, int64_t* tgt_len) {
  const int64_t L = tokens < 1 ? 0 : (tokens > (1 << 24) ? (1 << 24) + 1 : tokens + 2);
  if (t5_check(L, 1, 1, dq, iq, n_sentinels, n_sentinels)) return -1;
  if (!in_len || !tgt_len) LDDL_FAIL(-1, "null output");
  int32_t N, k;
  t5_counts(tokens, dq, iq, n_sentinels, &N, &k);
  *in_len = tokens - N + k + 1;
  *tgt_len = (int64_t)N + k + 1;
  return 0;
}

extern "C" int lddl_t5_corrupt(void* stream, const int32_t* d_ids, const int64_t* d_sent_off,
                               const int64_t* d_piece_off, const uint8_t* d_sent_sep,
                               const int64_t* d_block_sent, const int64_t* d_rows, int32_t batch,
                               int32_t plan_seq_len, int32_t in_len, int32_t tgt_len, int32_t dq,
                               int32_t iq, int32_t n_sentinels, int64_t sentinel_first,
                               int64_t eos_id, int64_t pad_id, int64_t decoder_start_id,
                               int64_t ignore_index, uint64_t seed, uint64_t counter,
                               int64_t* d_input_ids, int64_t* d_attention_mask, int64_t* d_labels,
                               int64_t* d_decoder_input_ids, int64_t* d_src_lengths,
                               int64_t* d_tgt_lengths) {
  if (t5_check(plan_seq_len, in_len, tgt_len, dq, iq, n_sentinels, sentinel_first)) return -1;
  if (batch <= 0) return 0;
  if (!d_ids || !d_sent_off || !d_piece_off || !d_sent_sep || !d_block_sent)
    LDDL_FAIL(-1, "null token table or plan");
  if (!d_input_ids || !d_attention_mask || !d_labels || !d_decoder_input_ids || !d_src_lengths ||
      !d_tgt_lengths)
    LDDL_FAIL(-1, "null output");
  const T5Args A{d_ids, d_sent_off, d_piece_off, d_sent_sep, d_block_sent, d_rows, batch,
                 plan_seq_len, in_len, tgt_len, dq, iq, n_sentinels, sentinel_first, eos_id,
                 pad_id, decoder_start_id, ignore_index, MaskDraw{0.f, 0, 0, 0, seed, counter},
                 d_input_ids, d_attention_mask, d_labels, d_decoder_input_ids, d_src_lengths,
                 d_tgt_lengths};
  hipLaunchKernelGGL(t5_kernel, dim3((unsigned)((batch + kEncWaves - 1) / kEncWaves)),
                     dim3(64 * kEncWaves), 0, as_stream(stream), A);
  LDDL_HIP(hipGetLastError());
  return 0;
}
