// BART denoising on the device (past the reference): sentence permutation and text
// infilling of tokenized documents in one pass, straight from ctx.tokenize's output. A row
// shrinks (a span of whole words becomes one noise token) and grows (a span of length 0 inserts
// one), and its source order is a permutation of ragged sentences, so a slot's source is a
// bisection of a position table and its destination a prefix sum over the decisions before it.
//
// One wave per sample, kDenoiseWaves samples per workgroup, four int32 tables of the sample's
// units in LDS (denoise_shape.h); no atomics, no block-wide barrier, no pass over global memory
// but the loads of the ids and the stores of the rows.
//
//   phase 1  units     lanes run over the sentences, 64 a window: length, wave prefix sum, clip
//                      to the budget T = L - 2 -> opos[u], the unit's first original position;
//                      the participants of the permutation (their unit and key) are compacted
//                      by ballot into ppos[] / pkey[]
//   phase 2  order     a participant counts the smaller (key, unit) pairs: its rank r; place
//                      ppos[r] takes its unit -> order[]; a scan of the lengths in that order
//                      -> ppos[k], place k's first permuted position (over the list, now dead)
//   phase 3  slots     64 permuted positions a step, lane = position: bisect ppos, load the id;
//                      heads by ballot, word by v_mbcnt; start and length draws; one max-scan
//                      for the exclusive reach; the word's fate to its continuations by ballot;
//                      emit count 0 / 1 / 2, one sum-scan for the destination; stores
//   phase 4  targets   labels and decoder_input_ids: a ragged copy in original order (opos)
//
// Between the windows of phase 3 the state is wave-uniform: the words before, the furthest
// reach, the pieces emitted, and whether the last word's continuations keep their ids (a word
// may straddle two windows). Every lane reaches every ballot and scan; the tails are predicated.
#include "common.h"
#include "ctx.h"
#include "denoise_dev.h"
#include "device.h"
#include "lddl_amd.h"

namespace lddl {
namespace {

__device__ inline int32_t last_lane(int32_t v) { return __builtin_amdgcn_readlane(v, 63); }

__global__ void __launch_bounds__(64 * kDenoiseWaves) denoise_kernel(DenoiseArgs A) {
  extern __shared__ __attribute__((aligned(16))) int32_t tables[];
  const int w = wave_id(), lane = lane_id();
  const int32_t b = blockIdx.x * kDenoiseWaves + w;
  if (b >= A.B) return;  // the whole wave; no block-wide barrier below
  int32_t* opos = tables + (size_t)w * kDenoiseTables * kDenoiseStride;
  int32_t* ppos = opos + kDenoiseStride;
  uint32_t* pkey = reinterpret_cast<uint32_t*>(ppos + kDenoiseStride);
  int32_t* order = ppos + 2 * kDenoiseStride;

  const int64_t d = A.rows ? A.rows[b] : (int64_t)b;
  const int64_t s0 = A.doc_sent_off[d];
  const int64_t S = A.doc_sent_off[d + 1] - s0;
  const int32_t U = (int32_t)(S < kDenoiseUnits ? S : kDenoiseUnits);
  const int32_t T = A.L - 2;
  const int64_t flat0 = (int64_t)b * A.draw_stride;

  // ---- phase 1: units ------------------------------------------------------------------------
  // carry = the pieces before the window, clipped to T, and so are the lengths: a window's sums
  // stay below 65 T < 2^31 (the entry point refuses seq_len > 2^24)
  int32_t carry = 0, np = 0;
  for (int64_t w0 = 0; w0 < S && (w0 < kDenoiseUnits || carry < T); w0 += 64) {
    const int64_t s = w0 + lane;
    int32_t l = s < S ? (A.sent_len[s0 + s] & kLenMask) : 0;
    l = l < T ? l : T;
    const int32_t incl = carry + (int32_t)wave_incl_scan(l);
    const int32_t cs = incl - l < T ? incl - l : T, ce = incl < T ? incl : T;
    carry = last_lane(incl);
    carry = carry < T ? carry : T;
    if (w0 < kDenoiseUnits) {  // the tail unit's first sentence is the last lane of these windows
      const uint4 rs = denoise_draw(A.sent_seed, A.counter, flat0 + s);
      const bool part = s < kDenoiseUnits - 1 && ce > cs && u01(rs.x) < A.permute_p;
      const uint64_t pm = ballot(part);
      if (s < U) {
        opos[s] = cs;
        order[s] = (int32_t)s;
      }
      if (part) {
        const int32_t j = np + (int32_t)popc_below(pm);
        ppos[j] = (int32_t)s;
        pkey[j] = rs.y;
      }
      np += __popcll(pm);
    }
  }
  const int32_t M = carry;  // the pieces the sample keeps
  if (lane == 0) opos[U] = M;
  wave_sync();
  if (S >= kDenoiseUnits) {  // the tail unit: its length is known only now; it is the last unit
    const int32_t u = kDenoiseUnits - 1;
    const uint4 rs = denoise_draw(A.sent_seed, A.counter, flat0 + u);
    const int part = __builtin_amdgcn_readfirstlane(
        (int)(M > opos[u] && u01(rs.x) < A.permute_p));
    if (part) {
      if (lane == 0) {
        ppos[np] = u;
        pkey[np] = rs.y;
      }
      np += 1;
    }
    wave_sync();
  }

  // ---- phase 2: order ------------------------------------------------------------------------
  // the participants are listed by unit, so (key, unit) orders like (key, list index)
  for (int32_t j0 = 0; j0 < np; j0 += 64) {
    const int32_t j = j0 + lane;
    if (j < np) {
      const uint32_t key = pkey[j];
      int32_t rank = 0;
      for (int32_t t = 0; t < np; ++t) {
        const uint32_t kt = pkey[t];
        rank += (kt < key || (kt == key && t < j)) ? 1 : 0;
      }
      order[ppos[rank]] = ppos[j];
    }
  }
  wave_sync();  // the list is dead from here: ppos becomes the position table
  int32_t pc = 0;
  for (int32_t k0 = 0; k0 < U; k0 += 64) {
    const int32_t k = k0 + lane;
    int32_t l = 0;
    if (k < U) {
      const int32_t o = order[k];
      l = opos[o + 1] - opos[o];
    }
    const int32_t incl = pc + (int32_t)wave_incl_scan(l);
    if (k < U) ppos[k] = incl - l;
    pc = last_lane(incl);
  }
  if (lane == 0) ppos[U] = M;
  wave_sync();

  // ---- phase 3: slots ------------------------------------------------------------------------
  int64_t* in_row = A.input_ids + (int64_t)b * A.L;
  int32_t words_before = 0, emitted = 0;
  uint32_t carry_max = 0;
  bool carry_kept = true;
  for (int32_t x0 = 0; x0 < M; x0 += 64) {
    const int32_t x = x0 + lane;
    const bool in = x < M;
    int32_t id = 0;
    bool first = false;
    if (in) {
      const int32_t k = denoise_locate(ppos, U, x);
      id = denoise_piece(A, s0, S, order[k], x - ppos[k], &first);
    }
    const bool head = in && (first || !cont_id(A.cont, id));
    const uint64_t hm = ballot(head);
    // heads at or below the lane: a continuation takes the word of its head
    const int32_t word = words_before + (int32_t)popc_below(hm) + (head ? 1 : 0) - 1;
    const uint4 r = denoise_draw(A.seed, A.counter, flat0 + x);
    int32_t len = -1;  // no start
    if (head && u01(r.x) < A.draw.p_start) len = denoise_len(A.draw, A.counter, flat0 + x);
    const uint32_t scanned = wave_incl_max(len >= 0 ? (uint32_t)(word + len) : 0u);
    // E(word): the lanes below a head hold the words before it
    uint32_t reach = (uint32_t)wave_prev((int)scanned);
    reach = lane == 0 ? 0u : reach;
    reach = reach > carry_max ? reach : carry_max;
    const bool deleted = (int32_t)reach > word;  // (of a head)
    // the continuations of a word keep their ids iff it is neither deleted nor replaced
    const uint64_t km = ballot(head && !deleted && len < 1);
    int32_t n_emit = 0;
    if (head) {
      n_emit = deleted ? 0 : (len == 0 ? 2 : 1);
    } else if (in) {
      const uint64_t le = hm & (~0ull >> (63 - lane));  // the heads below (the lane is none)
      n_emit = (le ? (km >> (63 - __clzll((long long)le))) & 1 : carry_kept) ? 1 : 0;
    }
    const int32_t incl = (int32_t)wave_incl_scan(n_emit);
    const int32_t dst = 1 + emitted + incl - n_emit;
    if (head && !deleted && len >= 0) {  // one noise token for the span, or the inserted one
      const int64_t noise = u01(r.y) < A.random_ratio
                                ? (int64_t)(((uint64_t)r.w * (uint64_t)A.vocab_len) >> 32)
                                : A.mask_id;
      if (dst < A.L - 1) in_row[dst] = noise;
      if (len == 0 && dst + 1 < A.L - 1) in_row[dst + 1] = id;
    } else if (n_emit && dst < A.L - 1) {
      in_row[dst] = id;
    }
    emitted += last_lane(incl);
    const uint32_t far = (uint32_t)last_lane((int32_t)scanned);
    carry_max = far > carry_max ? far : carry_max;
    words_before += __popcll(hm);
    if (hm) carry_kept = (km >> (63 - __clzll((long long)hm))) & 1;
  }
  // bos, eos, the padding, the mask row and the untruncated length
  const int32_t eos_at = (emitted < T ? emitted : T) + 1;
  int64_t* att_row = A.attention_mask + (int64_t)b * A.L;
  for (int32_t t = lane; t < A.L; t += 64) {
    if (t == 0) in_row[t] = A.bos;
    else if (t == eos_at) in_row[t] = A.eos;
    else if (t > eos_at) in_row[t] = A.pad;
    att_row[t] = t <= eos_at ? 1 : 0;
  }
  if (lane == 0) A.src_lengths[b] = emitted + 2;

  // ---- phase 4: targets ----------------------------------------------------------------------
  // labels = bos, the M pieces in original order, eos, ignore_index; the decoder row is labels
  // one slot to the right behind dec_start, pad where labels is ignored
  int64_t* lab_row = A.labels + (int64_t)b * A.L;
  int64_t* dec_row = A.decoder_input_ids + (int64_t)b * A.L;
  for (int32_t t = lane; t < A.L; t += 64) {
    int64_t lab = A.ignore_index;
    if (t == 0) {
      lab = A.bos;
      dec_row[0] = A.dec_start;
    } else if (t <= M) {
      const int32_t u = denoise_locate(opos, U, t - 1);
      bool first;
      lab = denoise_piece(A, s0, S, u, t - 1 - opos[u], &first);
    } else if (t == M + 1) {
      lab = A.eos;
    }
    lab_row[t] = lab;
    if (t + 1 < A.L) dec_row[t + 1] = t <= M + 1 ? lab : A.pad;
  }
}

// the span arguments of the kernel from the caller's struct: refused unless it is one that
// lddl_denoise_params_make can have written (or one made by hand to the same rules)
int denoise_draw_of(const lddl_denoise_params* dp, uint64_t seed, DenoiseDraw* out) {
  if (!dp) LDDL_FAIL(-1, "null denoise params");
  bool ok = dp->n >= 1 && dp->n <= kDenoiseMaxN && dp->p_start >= 0.f && dp->p_start <= 1.f;
  float prev = 0.f;
  for (int k = 0; ok && k < kDenoiseMaxN; ++k) {
    const float c = dp->cum[k];
    ok = k < dp->n ? (c >= prev && c <= 1.f) : c == 1.f;
    prev = c;
  }
  if (!ok) LDDL_FAIL(-1, "invalid denoise params (not made by lddl_denoise_params_make)");
  out->seed2 = seed ^ LDDL_SPAN_SEED_XOR;
  out->p_start = dp->p_start;
  for (int k = 0; k < kDenoiseMaxN; ++k) out->cum[k] = dp->cum[k];
  return 0;
}

}  // namespace
}  // namespace lddl

using namespace lddl;

static_assert(kDenoiseUnits == LDDL_DENOISE_MAX_UNITS, "the header's S_max is the kernel's");
static_assert(kDenoiseMaxN == LDDL_SPAN_MAX_N, "one longest span");

// Both entry points: the values are refused first, whatever the continuation bitmap's owner is;
// `owner_error` is that owner's refusal (a NULL ctx, a NULL bitmap), reported right after them.
static int denoise_launch(ContBits cont, const char* owner_error, const char* bitmap_error,
                          void* stream, const int32_t* d_ids, const int64_t* d_sent_off,
                          const int32_t* d_sent_len, const int64_t* d_doc_sent_off,
                          const int64_t* d_rows, int32_t batch, int32_t seq_len,
                          int64_t* d_input_ids, int64_t* d_attention_mask,
                          int64_t* d_decoder_input_ids, int64_t* d_labels, int32_t* d_src_lengths,
                          int64_t bos_id, int64_t eos_id, int64_t pad_id, int64_t mask_id,
                          int64_t decoder_start_id, int64_t ignore_index, int64_t vocab_len,
                          uint64_t seed, uint64_t counter, int32_t draw_stride, float permute_p,
                          float random_ratio, const lddl_denoise_params* params) {
  DenoiseDraw draw;
  if (denoise_draw_of(params, seed, &draw)) return -1;
  if (seq_len < 2 || seq_len > (1 << 24))  // 64 lengths of at most seq_len and a carry: int32
    LDDL_FAIL(-1, "seq_len %d: a row holds bos and eos at least, and 2^24 slots at most", seq_len);
  if (draw_stride < seq_len) LDDL_FAIL(-1, "draw_stride %d < seq_len %d", draw_stride, seq_len);
  if (!(permute_p >= 0.f && permute_p <= 1.f) || !(random_ratio >= 0.f && random_ratio <= 1.f))
    LDDL_FAIL(-1, "permute_p and random_ratio must lie in [0, 1]");
  if (vocab_len < 1 || vocab_len > (int64_t)1 << 32) LDDL_FAIL(-1, "vocab_len outside [1, 2^32]");
  if (owner_error) LDDL_FAIL(-1, "%s", owner_error);
  if (batch <= 0) return 0;
  if (!d_ids || !d_sent_off || !d_sent_len || !d_doc_sent_off) LDDL_FAIL(-1, "null token table");
  if (!d_input_ids || !d_attention_mask || !d_decoder_input_ids || !d_labels || !d_src_lengths)
    LDDL_FAIL(-1, "null output");
  if (bitmap_error) LDDL_FAIL(-1, "%s", bitmap_error);
  const DenoiseArgs A{d_ids, d_sent_off, d_sent_len, d_doc_sent_off, d_rows, batch, seq_len,
                      draw_stride, d_input_ids, d_attention_mask, d_decoder_input_ids, d_labels,
                      d_src_lengths, bos_id, eos_id, pad_id, mask_id, decoder_start_id,
                      ignore_index, vocab_len, seed, seed ^ LDDL_DENOISE_SENT_XOR, counter,
                      permute_p, random_ratio, cont, draw};
  const DenoiseShape sh = denoise_shape(batch);
  hipLaunchKernelGGL(denoise_kernel, dim3(sh.grid), dim3(sh.threads()), sh.lds_bytes(),
                     as_stream(stream), A);
  LDDL_HIP(hipGetLastError());
  return 0;
}

extern "C" int lddl_bart_denoise(lddl_ctx* c, void* stream, const int32_t* d_ids,
                                 const int64_t* d_sent_off, const int32_t* d_sent_len,
                                 const int64_t* d_doc_sent_off, const int64_t* d_rows,
                                 int32_t batch, int32_t seq_len, int64_t* d_input_ids,
                                 int64_t* d_attention_mask, int64_t* d_decoder_input_ids,
                                 int64_t* d_labels, int32_t* d_src_lengths, int64_t bos_id,
                                 int64_t eos_id, int64_t pad_id, int64_t mask_id,
                                 int64_t decoder_start_id, int64_t ignore_index,
                                 int64_t vocab_len, uint64_t seed, uint64_t counter,
                                 int32_t draw_stride, float permute_p, float random_ratio,
                                 const lddl_denoise_params* params) {
  return denoise_launch(
      ContBits{c ? c->d_cont_bits : nullptr, c ? c->vocab_size : 0}, c ? nullptr : "null ctx",
      c && c->d_cont_bits ? nullptr : "the context has no continuation bitmap", stream, d_ids,
      d_sent_off, d_sent_len, d_doc_sent_off, d_rows, batch, seq_len, d_input_ids,
      d_attention_mask, d_decoder_input_ids, d_labels, d_src_lengths, bos_id, eos_id, pad_id,
      mask_id, decoder_start_id, ignore_index, vocab_len, seed, counter, draw_stride, permute_p,
      random_ratio, params);
}

extern "C" int lddl_bart_denoise_bits(const uint32_t* d_cont_bits, int64_t n_ids, void* stream,
                                      const int32_t* d_ids, const int64_t* d_sent_off,
                                      const int32_t* d_sent_len, const int64_t* d_doc_sent_off,
                                      const int64_t* d_rows, int32_t batch, int32_t seq_len,
                                      int64_t* d_input_ids, int64_t* d_attention_mask,
                                      int64_t* d_decoder_input_ids, int64_t* d_labels,
                                      int32_t* d_src_lengths, int64_t bos_id, int64_t eos_id,
                                      int64_t pad_id, int64_t mask_id, int64_t decoder_start_id,
                                      int64_t ignore_index, int64_t vocab_len, uint64_t seed,
                                      uint64_t counter, int32_t draw_stride, float permute_p,
                                      float random_ratio, const lddl_denoise_params* params) {
  const bool ok = d_cont_bits && n_ids >= 1 && n_ids <= INT32_MAX;
  return denoise_launch(
      ContBits{d_cont_bits, (int32_t)(ok ? n_ids : 0)},
      ok ? nullptr : "null continuation bitmap, or n_ids outside [1, 2^31)", nullptr, stream,
      d_ids, d_sent_off, d_sent_len, d_doc_sent_off, d_rows, batch, seq_len, d_input_ids,
      d_attention_mask, d_decoder_input_ids, d_labels, d_src_lengths, bos_id, eos_id, pad_id,
      mask_id, decoder_start_id, ignore_index, vocab_len, seed, counter, draw_stride, permute_p,
      random_ratio, params);
}
