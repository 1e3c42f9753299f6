// BART pretraining chunks on the GPU: the reference's `_aggregate_sentences`
// (lddl/dask/bart/pretrain.py:88-128) over the segmenter's output, for a whole batch of documents.
//
//   for sentence in sentences:            # sent_tokenize + strip() + drop empty (82-86)
//     chunk += " " + sentence
//     num_tokens += len(sentence.split())
//     if num_tokens >= target_length: emit chunk; chunk, num_tokens = "", 0
//   if num_tokens > 0: emit chunk
//
// Input is the layout lddl_segment_fill writes: sentences contiguous, inter-sentence whitespace
// attached to the left sentence, a whitespace-only sentence standing for a dropped one.
//
// Structure used here:
//  * str.strip() / str.split() use str.isspace(), which is bit 0 of the Punkt class table that
//    lddl_punkt_set_params uploaded (tests/test_bart_host.py checks every code point);
//  * every chunk is ' ' + s for its sentences in order, and the chunks follow one another in
//    sentence order, so the output buffer is simply ' ' + strip(s) over all non-empty sentences:
//    a sentence's destination is an exclusive scan of (1 + stripped length) and does not depend
//    on where the chunks are cut. A chunk is then described by the destination at which it ends.
//
// K1 bart_stats_kernel   text tiles of 16 KiB (16-B loads) -> whitespace bitmap in
//                        LDS -> per sentence: leading whitespace, stripped end, word count
//                        (popcounts over the bitmap; a sentence that crosses tiles is combined
//                        with atomics, so a 70-KB sentence is counted by 5 workgroups at once)
//    scan                sentence destinations
// K2 bart_chunk_kernel   one wave per document: wave prefix sums of the word counts, a ballot
//                        finds each cut, chunk ends / word counts go to the document's slots
//    scan                chunk offsets of documents
// K3 bart_compact_kernel slots -> chunk_off / num_tokens
// K4 bart_fill_kernel    output tiles of 16 KiB, 16-byte pieces gathered from the text
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>

#include "common.h"
#include "ctx.h"
#include "device.h"
#include "lddl_amd.h"
#include "punkt_classes.h"
#include "scan.h"

namespace lddl {
namespace {

constexpr int kTile = 16384;     // text / output bytes per workgroup
constexpr int kTileThreads = 256;
constexpr int kPer = kTile / (16 * kTileThreads);  // 16-byte pieces per thread, kTileThreads apart
constexpr int kPad = 16;         // bytes staged on either side of a text tile (4 are needed)

// str.isspace() of a code point >= 0x80
__device__ __forceinline__ bool table_space(const ClassTab& t, uint32_t v) {
  return (class_bits(t, v) & kPSpace) != 0;
}

// Only code points whose UTF-8 form starts with C2, E1, E2 or E3 are whitespace (U+0085 ...
// U+3000; tests/test_bart_host.py checks the table against this), so only those lead bytes pay
// for a table lookup: curly quotes and dashes (E2 80 xx) do, accented letters (C3) and most CJK
// (E4-E9) do not.
__device__ __forceinline__ bool space_lead(uint32_t c) { return c == 0xC2u || (c >= 0xE1u && c <= 0xE3u); }

// the code point of 2 or 3 bytes that starts at the lead byte raw[j]
__device__ __forceinline__ uint32_t decode23(const uint8_t* raw, int j, int* n) {
  const uint32_t c = raw[j];
  *n = c < 0xE0u ? 2 : 3;
  uint32_t v = (c < 0xE0u ? (c & 31u) : (c & 15u)) << 6 | (raw[j + 1] & 63u);
  if (c >= 0xE0u) v = (v << 6) | (raw[j + 2] & 63u);
  return v;
}

// is the code point that contains the non-ASCII byte raw[r] whitespace; raw[r - 3 .. r + 2] exist
// (the bytes at a tile's edge whose lead byte belongs to the tile before)
__device__ inline bool cp_space(const ClassTab& t, const uint8_t* raw, int r) {
  int j = r;
  while (j > r - 3 && (raw[j] & 0xC0u) == 0x80u) --j;
  if (!space_lead(raw[j])) return false;
  int n;
  const uint32_t v = decode23(raw, j, &n);
  return r < j + n && table_space(t, v);
}

// Two partition points at once, by the whole workgroup: the first i in [0, n) with pa(i), and
// with pb(i) (n if none); both predicates are monotone (false ... true). Every round the 256
// threads probe 256 evenly spaced points of each range, so 16M entries take three rounds of one
// load each instead of 24 dependent loads by one thread while the others wait.
template <typename PA, typename PB>
__device__ inline void block_partition_points(int64_t n, PA pa, PB pb, int64_t* ra, int64_t* rb) {
  int64_t lo[2] = {0, 0}, hi[2] = {n, n};
  while (lo[0] < hi[0] || lo[1] < hi[1]) {  // (uniform: every thread holds the same ranges)
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      const int64_t l = lo[w], m = hi[w] - l;
      const int64_t step = (m + kTileThreads - 1) / kTileThreads;
      const int64_t i = l + (int64_t)threadIdx.x * step;
      const bool miss = m > 0 && i < hi[w] && !(w == 0 ? pa(i) : pb(i));
      const int64_t f = __syncthreads_count(miss);  // the probes that miss are the first f
      if (m <= 0) continue;
      if (f == 0) {
        hi[w] = l;
      } else {
        lo[w] = l + (f - 1) * step + 1;
        hi[w] = std::min(hi[w], l + f * step);
      }
    }
  }
  *ra = lo[0];
  *rb = lo[1];
}

// K1. Tile b covers text bytes [t0, t0 + kTile), t0 = b * kTile - (x & 15), so that every
// 16-byte piece is one aligned load (kPer per thread: with 4-KiB tiles the kernel was bound by
// the latency of each workgroup's few dependent loads, not by bandwidth). words[] is zero, lead[] 0x7F7F7F7F and end[] zero on
// entry (relative to the sentence start; a sentence is < 2 GiB).
__global__ void __launch_bounds__(kTileThreads) bart_stats_kernel(
    ClassTab t, const uint8_t* __restrict__ x, int64_t n_bytes, const int64_t* __restrict__ sent_off,
    int64_t n_sent, int32_t* __restrict__ words, int32_t* __restrict__ lead, int32_t* __restrict__ end) {
  __shared__ uint4 raw4[(kTile + 2 * kPad) / 16];
  __shared__ uint64_t ws64[kTile / 64];
  __shared__ uint32_t prev_ws;
  const int tid = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * kTile - (int64_t)((uintptr_t)x & 15u);
  const int64_t t1 = t0 + kTile;
  uint8_t* raw = reinterpret_cast<uint8_t*>(raw4) + kPad;  // raw[r] = x[t0 + r], r in [-kPad, kTile + kPad)
  uint4 v[kPer];
#pragma unroll
  for (int c = 0; c < kPer; ++c) {  // (all loads in flight before the LDS writes)
    const int64_t p = t0 + 16 * (int64_t)(tid + kTileThreads * c);
    v[c] = make_uint4(0, 0, 0, 0);
    if (p >= 0 && p + 16 <= n_bytes) {
      v[c] = *reinterpret_cast<const uint4*>(x + p);
    } else if (p + 16 > 0 && p < n_bytes) {  // the ends of the text buffer
      uint8_t tmp[16] = {};
      for (int k = 0; k < 16; ++k)
        if (p + k >= 0 && p + k < n_bytes) tmp[k] = x[p + k];
      memcpy(&v[c], tmp, 16);
    }
  }
#pragma unroll
  for (int c = 0; c < kPer; ++c) raw4[1 + tid + kTileThreads * c] = v[c];
  if (tid < 8) {  // 4 bytes before and after the tile: the rest of a code point cut by its edge
    const int r = tid < 4 ? tid - 4 : kTile + tid - 4;
    const int64_t q = t0 + r;
    raw[r] = (q >= 0 && q < n_bytes) ? x[q] : (uint8_t)0;
  }
  // sentences that meet the tile: [first s with sent_off[s + 1] > t0, first s with sent_off[s] >= t1)
  int64_t i0, i1;
  block_partition_points(
      n_sent, [&](int64_t i) { return sent_off[i + 1] > t0; }, [&](int64_t i) { return sent_off[i] >= t1; }, &i0,
      &i1);
  __syncthreads();
  // whitespace bitmap of the tile, one bit per byte (every byte of a whitespace code point).
  // ASCII by a bit test; then one table lookup per candidate lead byte (rare), whose bits may
  // run over into the next thread's 16 (or, at the tile's end, into the next tile, which
  // classifies its first continuation bytes itself).
  uint32_t* ws32 = reinterpret_cast<uint32_t*>(ws64);
  uint32_t spill[kPer];
#pragma unroll
  for (int c = 0; c < kPer; ++c) {
    const int piece = tid + kTileThreads * c;
    const uint32_t w[4] = {v[c].x, v[c].y, v[c].z, v[c].w};
    uint32_t m = 0, leads = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const uint32_t ch = (w[k >> 2] >> (8 * (k & 3))) & 255u;
      m |= (ascii_space(ch) ? 1u : 0u) << k;
      leads |= (space_lead(ch) ? 1u : 0u) << k;
    }
    for (; leads; leads &= leads - 1) {
      const int k = __builtin_ctz(leads);
      int n;
      const uint32_t cp = decode23(raw, 16 * piece + k, &n);
      if (table_space(t, cp)) m |= ((1u << n) - 1u) << k;  // (bits 16..17: the next piece's bytes)
    }
    reinterpret_cast<uint16_t*>(ws64)[piece] = (uint16_t)m;
    spill[c] = m >> 16;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < kPer; ++c) {
    const int nxt = tid + kTileThreads * c + 1;
    if (spill[c] && nxt < kTile / 16) atomicOr(&ws32[nxt >> 1], spill[c] << (16 * (nxt & 1)));
  }
  if (tid == 0) {
    uint32_t head = 0;  // continuation bytes at the tile's start
    for (int r = 0; r < 3 && (raw[r] & 0xC0u) == 0x80u; ++r) head |= (cp_space(t, raw, r) ? 1u : 0u) << r;
    if (head) atomicOr(&ws32[0], head);
    const uint32_t c = raw[-1];
    prev_ws = (c < 0x80u ? ascii_space(c) : cp_space(t, raw, -1)) ? 1u : 0u;
  }
  __syncthreads();
  for (int64_t s = i0 + tid; s < i1; s += kTileThreads) {
    const int64_t a = sent_off[s], b = sent_off[s + 1];
    const int64_t lo = std::max(a, t0), hi = std::min(b, t1);
    if (lo >= hi) continue;
    const int rl = (int)(lo - t0), rh = (int)(hi - t0);  // bits [rl, rh) of the tile
    const int k0 = rl >> 6, k1 = (rh - 1) >> 6;
    int cnt = 0, first = -1, last = -1;
    for (int k = k0; k <= k1; ++k) {
      const uint64_t W = ws64[k];
      const uint64_t pv = (W << 1) | (k ? ws64[k - 1] >> 63 : (uint64_t)prev_ws);
      uint64_t mask = ~0ull;
      if (k == k0) mask &= ~0ull << (rl & 63);
      if (k == k1 && (rh & 63)) mask &= (1ull << (rh & 63)) - 1ull;
      const uint64_t N = ~W & mask;  // non-whitespace bytes of the sentence
      uint64_t S = N & pv;           // ... that follow whitespace: word starts
      // the sentence's first byte starts a word whatever precedes it
      if (a >= t0 && k == k0) S |= N & (1ull << (rl & 63));
      cnt += __builtin_popcountll(S);
      if (N) {
        if (first < 0) first = k * 64 + __builtin_ctzll(N);
        last = k * 64 + 64 - __builtin_clzll(N);
      }
    }
    const int32_t fr = (int32_t)(t0 + first - a), er = (int32_t)(t0 + last - a);
    if (a >= t0 && b <= t1) {  // the whole sentence: plain stores
      words[s] = cnt;
      if (first >= 0) {
        lead[s] = fr;
        end[s] = er;
      }
    } else {  // a piece of a sentence that other tiles see too
      if (cnt) atomicAdd(&words[s], cnt);
      if (first >= 0) {
        atomicMin(&lead[s], fr);
        atomicMax(&end[s], er);
      }
    }
  }
}

// bytes of ' ' + strip(sentence s), 0 for a dropped sentence
struct SentBytes {
  const int32_t* lead;
  const int32_t* end;
  __device__ int64_t operator()(int64_t s) const {
    const int32_t l = lead[s], e = end[s];
    return e > l ? (int64_t)(e - l) + 1 : 0;
  }
};

struct Cnt32 {
  const int32_t* cnt;
  __device__ int64_t operator()(int64_t i) const { return cnt[i]; }
};

// K2: one wave per document walks its sentences 64 at a time. acc = words of the open chunk up
// to and including each lane's sentence; the first non-empty lane with acc >= target closes the
// chunk, the later lanes are rebased by its count, and so on. Chunk k of document d goes to slot
// dso[d] + k (a document has no more chunks than sentences): cend = destination offset at which
// the chunk ends, cwords = its word count.
__global__ void __launch_bounds__(256) bart_chunk_kernel(
    const int64_t* __restrict__ dso, int64_t n_doc, const int32_t* __restrict__ words,
    const int32_t* __restrict__ lead, const int32_t* __restrict__ end, const int64_t* __restrict__ sent_dst,
    int32_t target, int64_t* __restrict__ cend, int32_t* __restrict__ cwords, int32_t* __restrict__ nchunk) {
  const int64_t d = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave_id();
  if (d >= n_doc) return;  // wave-uniform
  const int lane = lane_id();
  const int64_t s0 = dso[d], s1 = dso[d + 1];
  int64_t slot = s0;
  int32_t carry = 0;
  for (int64_t base = s0; base < s1; base += 64) {
    const int64_t s = base + lane;
    int32_t w = 0;
    if (s < s1 && end[s] > lead[s]) w = words[s];  // (a non-empty sentence has >= 1 word)
    const int32_t acc = carry + wave_incl_scan(w);
    int32_t sub = 0;
    int from = 0;
    while (true) {
      const uint64_t m = ballot(w > 0 && lane >= from && acc - sub >= target);
      if (!m) break;
      const int c = __builtin_ctzll(m);
      const int32_t n = __shfl(acc, c, 64) - sub;
      if (lane == 0) {
        cwords[slot] = n;
        cend[slot] = sent_dst[base + c + 1];
      }
      ++slot;
      sub += n;
      from = c + 1;
    }
    carry = __shfl(acc, 63, 64) - sub;
  }
  if (carry > 0) {  // the remainder
    if (lane == 0) {
      cwords[slot] = carry;
      cend[slot] = sent_dst[s1];
    }
    ++slot;
  }
  if (lane == 0) nchunk[d] = (int32_t)(slot - s0);
}

// K3: the documents' slots -> chunk_off[n_chunks + 1] / num_tokens[n_chunks]
__global__ void __launch_bounds__(256) bart_compact_kernel(
    const int64_t* __restrict__ dso, const int64_t* __restrict__ dco, int64_t n_doc,
    const int64_t* __restrict__ cend, const int32_t* __restrict__ cwords, int64_t* __restrict__ chunk_off,
    int32_t* __restrict__ num_tokens) {
  const int64_t d = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave_id();
  if (d >= n_doc) return;
  const int64_t s0 = dso[d], c0 = dco[d], n = dco[d + 1] - c0;
  if (d == 0 && lane_id() == 0) chunk_off[0] = 0;
  for (int64_t k = lane_id(); k < n; k += 64) {
    chunk_off[c0 + k + 1] = cend[s0 + k];
    if (num_tokens) num_tokens[c0 + k] = cwords[s0 + k];
  }
}

// K4: output tile b = bytes [b * kTile, ...) of the chunk buffer, kPer pieces of 16 per thread:
// out[sent_dst[s]] = ' ', out[sent_dst[s] + 1 + i] = text[sent_off[s] + lead[s] + i]. The
// destinations and source offsets of the tile's sentences are staged in LDS (about 130 sentences
// of prose; a tile with more than kStage takes them from global memory); a thread finds the
// sentence of its first byte by bisection there and walks on.
constexpr int kStage = 1024;

// (two instantiations rather than a run-time choice of pointer: a select between an LDS and a
// global pointer becomes flat loads)
template <bool kStaged>
struct SentTab {
  const int64_t* sd;  // LDS: sent_dst[i0 + k]
  const int64_t* sb;  // LDS: source offset of sentence i0 + k
  int64_t i0;
  const int64_t* sent_dst;
  const int64_t* sent_off;
  const int32_t* lead;
  __device__ __forceinline__ int64_t dst(int64_t s) const {
    if constexpr (kStaged) return sd[s - i0]; else return sent_dst[s];
  }
  // text index of output byte q of sentence s (q > dst(s)): src(s) + q
  __device__ __forceinline__ int64_t src(int64_t s) const {
    if constexpr (kStaged) return sb[s - i0]; else return sent_off[s] + lead[s] - sent_dst[s] - 1;
  }
};

// the calling thread's 16 output bytes [o, o + 16) of a tile whose sentences are [i0, i1]
template <bool kStaged>
__device__ __forceinline__ void fill16(const SentTab<kStaged>& t, int64_t i1, const uint8_t* __restrict__ x,
                                       int64_t o, int64_t total, uint8_t* __restrict__ out) {
  int64_t lo = t.i0, hi = i1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (t.dst(mid) <= o) lo = mid; else hi = mid - 1;
  }
  int64_t s = lo;
  int64_t dst = t.dst(s), nxt = t.dst(s + 1), src = t.src(s);
  uint8_t b[16];
  if (o > dst && o + 16 <= nxt) {  // inside one sentence (most threads): one 16-byte load
    memcpy(b, x + src + o, 16);
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int64_t q = o + k;
      b[k] = 0;
      if (q >= total) continue;
      while (q >= nxt) {  // (q stays inside the tile, which keeps s <= i1)
        ++s;
        dst = nxt;
        nxt = t.dst(s + 1);
        src = t.src(s);
      }
      b[k] = q == dst ? (uint8_t)' ' : x[src + q];
    }
  }
  if (o + 16 <= total && ((uintptr_t)out & 15u) == 0) {
    uint4 v;
    memcpy(&v, b, 16);
    *reinterpret_cast<uint4*>(out + o) = v;
  } else {
    for (int k = 0; k < 16; ++k)
      if (o + k < total) out[o + k] = b[k];
  }
}

__global__ void __launch_bounds__(kTileThreads) bart_fill_kernel(
    const uint8_t* __restrict__ x, const int64_t* __restrict__ sent_off, int64_t n_sent,
    const int32_t* __restrict__ lead, const int64_t* __restrict__ sent_dst, int64_t total,
    uint8_t* __restrict__ out) {
  __shared__ int64_t sd[kStage + 1];
  __shared__ int64_t sb[kStage];
  const int tid = threadIdx.x;
  const int64_t o0 = (int64_t)blockIdx.x * kTile;
  const int64_t ol = std::min(o0 + kTile, total) - 1;
  // the sentence that holds output byte o is the last s with sent_dst[s] <= o (sent_dst[0] = 0,
  // sent_dst[n_sent] = total > o; of equal destinations the last one is the non-empty one)
  int64_t i0, i1;
  block_partition_points(
      n_sent, [&](int64_t i) { return sent_dst[i] > o0; }, [&](int64_t i) { return sent_dst[i] > ol; }, &i0, &i1);
  --i0;
  --i1;
  const int64_t cnt = i1 - i0 + 1;  // sentences of the tile, dropped ones in between included
  const bool staged = cnt <= kStage;
  if (staged) {
    for (int k = tid; k <= cnt; k += kTileThreads) {
      const int64_t d = sent_dst[i0 + k];
      sd[k] = d;
      if (k < cnt) sb[k] = sent_off[i0 + k] + lead[i0 + k] - d - 1;
    }
  }
  __syncthreads();
  for (int c = 0; c < kPer; ++c) {
    const int64_t o = o0 + 16 * (int64_t)(tid + kTileThreads * c);
    if (o >= total) return;
    if (staged)
      fill16(SentTab<true>{sd, sb, i0, sent_dst, sent_off, lead}, i1, x, o, total, out);
    else
      fill16(SentTab<false>{sd, sb, i0, sent_dst, sent_off, lead}, i1, x, o, total, out);
  }
}

}  // namespace
}  // namespace lddl

using namespace lddl;

// What lddl_bart_count leaves for lddl_bart_fill. The scope owns every block: dropping the
// object gives them back to the arena.
struct PendingBart {
  ArenaScope mem;
  int32_t *words = nullptr, *lead = nullptr, *end = nullptr, *cwords = nullptr, *nchunk = nullptr;
  int64_t *sent_dst = nullptr, *cend = nullptr, *dco = nullptr, *scratch = nullptr;
  const uint8_t* text = nullptr;
  const int64_t *sent_off = nullptr, *dso = nullptr;
  int64_t n_sent = 0, n_doc = 0, n_chunks = 0, n_out = 0;
  PendingBart(DevArena* arena, hipStream_t st) : mem(arena, st) {}
};

struct lddl_bart_state {
  // the aggregation between lddl_bart_count and lddl_bart_fill (null: none pending)
  std::unique_ptr<PendingBart> pending;
};

extern "C" void lddl_bart_release(lddl_ctx* c) {
  delete c->bart;  // (a pending aggregation's blocks go back to the arena)
  c->bart = nullptr;
}

extern "C" int lddl_bart_count(lddl_ctx* c, void* stream, const uint8_t* d_text, int64_t n_bytes,
                               const int64_t* d_sent_off, int64_t n_sent, const int64_t* d_doc_sent_off,
                               int64_t n_doc, int32_t target_words, int64_t* n_chunks, int64_t* n_out_bytes) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  ClassTab t{};
  if (!punkt_class_tab(c, &t))
    LDDL_FAIL(-1, "Punkt parameters not set (lddl_punkt_set_params): lddl_bart_count needs the character classes");
  if (n_bytes < 0 || n_sent < 0 || n_doc < 0 || !n_chunks || !n_out_bytes || !d_sent_off || !d_doc_sent_off)
    LDDL_FAIL(-1, "bad sizes");
  if (n_doc == 0 && n_sent != 0) LDDL_FAIL(-1, "sentences without documents");
  if (!c->bart) c->bart = new lddl_bart_state();
  lddl_bart_state* bs = c->bart;
  if (bs->pending) LDDL_FAIL(-1, "an aggregation is pending: call lddl_bart_fill first");
  hipStream_t st = as_stream(stream);
  // local until the count is complete: an error return gives the blocks back
  auto S = std::make_unique<PendingBart>(&c->arena, st);
  const int64_t ns = n_sent + 1, nd = n_doc + 1;
  int rc;
  if ((rc = S->mem.take(&S->words, ns)) || (rc = S->mem.take(&S->lead, ns)) || (rc = S->mem.take(&S->end, ns)) ||
      (rc = S->mem.take(&S->cwords, ns)) || (rc = S->mem.take(&S->sent_dst, ns)) ||
      (rc = S->mem.take(&S->cend, ns)) || (rc = S->mem.take(&S->nchunk, nd)) || (rc = S->mem.take(&S->dco, nd)) ||
      (rc = S->mem.take(&S->scratch, scan_scratch_elems(std::max(n_sent, n_doc)))))
    return rc;
  LDDL_HIP(hipMemsetAsync(S->words, 0, sizeof(int32_t) * (size_t)ns, st));
  LDDL_HIP(hipMemsetAsync(S->lead, 0x7F, sizeof(int32_t) * (size_t)ns, st));
  LDDL_HIP(hipMemsetAsync(S->end, 0, sizeof(int32_t) * (size_t)ns, st));
  if (n_sent > 0 && n_bytes > 0) {
    const int64_t mis = (int64_t)((uintptr_t)d_text & 15u);
    const int64_t grid = (n_bytes + mis + kTile - 1) / kTile;
    hipLaunchKernelGGL(bart_stats_kernel, dim3((unsigned)grid), dim3(kTileThreads), 0, st, t, d_text, n_bytes,
                       d_sent_off, n_sent, S->words, S->lead, S->end);
    LDDL_HIP(hipGetLastError());
  }
  LDDL_HIP(scan_exclusive(SentBytes{S->lead, S->end}, n_sent, S->sent_dst, S->scratch, st));
  if (n_doc > 0) {
    const int64_t grid = (n_doc + 3) / 4;
    hipLaunchKernelGGL(bart_chunk_kernel, dim3((unsigned)grid), dim3(256), 0, st, d_doc_sent_off, n_doc,
                       (const int32_t*)S->words, (const int32_t*)S->lead, (const int32_t*)S->end,
                       (const int64_t*)S->sent_dst, target_words, S->cend, S->cwords, S->nchunk);
    LDDL_HIP(hipGetLastError());
  }
  LDDL_HIP(scan_exclusive(Cnt32{S->nchunk}, n_doc, S->dco, S->scratch, st));
  int64_t tot[2] = {0, 0};
  LDDL_HIP(hipMemcpyAsync(&tot[0], S->dco + n_doc, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipMemcpyAsync(&tot[1], S->sent_dst + n_sent, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipStreamSynchronize(st));
  S->text = d_text;
  S->sent_off = d_sent_off;
  S->dso = d_doc_sent_off;
  S->n_sent = n_sent;
  S->n_doc = n_doc;
  S->n_chunks = *n_chunks = tot[0];
  S->n_out = *n_out_bytes = tot[1];
  bs->pending = std::move(S);
  return 0;
}

extern "C" int lddl_bart_fill(lddl_ctx* c, void* stream, uint8_t* d_out, int64_t* d_chunk_off,
                              int32_t* d_num_tokens, int64_t* d_doc_chunk_off) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  lddl_bart_state* bs = c->bart;
  if (!bs || !bs->pending) LDDL_FAIL(-1, "no pending aggregation (lddl_bart_count)");
  hipStream_t st = as_stream(stream);
  // the call ends the pending aggregation, whatever it returns (all outputs null: cancel)
  std::unique_ptr<PendingBart> S = std::move(bs->pending);
  const bool cancel = !d_out && !d_chunk_off && !d_num_tokens && !d_doc_chunk_off;
  int rc = 0;
  const char* why = "lddl_bart_fill: HIP launch/copy failed";
  if (!cancel) {
    if (!d_chunk_off || !d_doc_chunk_off || (!d_out && S->n_out > 0)) {
      rc = -1;
      why = "lddl_bart_fill: null output";
    } else {
      const int64_t n_doc = S->n_doc;
      if (n_doc > 0) {
        const int64_t grid = (n_doc + 3) / 4;
        hipLaunchKernelGGL(bart_compact_kernel, dim3((unsigned)grid), dim3(256), 0, st, S->dso,
                           (const int64_t*)S->dco, n_doc, (const int64_t*)S->cend, (const int32_t*)S->cwords,
                           d_chunk_off, d_num_tokens);
      } else if (hipMemsetAsync(d_chunk_off, 0, sizeof(int64_t), st) != hipSuccess) {
        rc = -100;
      }
      if (hipMemcpyAsync(d_doc_chunk_off, S->dco, sizeof(int64_t) * (size_t)(n_doc + 1), hipMemcpyDeviceToDevice,
                         st) != hipSuccess)
        rc = -100;
      if (S->n_out > 0) {
        const int64_t grid = (S->n_out + kTile - 1) / kTile;
        hipLaunchKernelGGL(bart_fill_kernel, dim3((unsigned)grid), dim3(kTileThreads), 0, st, S->text, S->sent_off,
                           S->n_sent, (const int32_t*)S->lead, (const int64_t*)S->sent_dst, S->n_out, d_out);
      }
      if (hipGetLastError() != hipSuccess) rc = -100;
    }
  }
  S->mem.release(st);
  if (rc) LDDL_FAIL(rc, "%s", why);
  return 0;
}
