// The GPT stream: what the plan (stream_plan.hip) and the rows (stream_rows.hip)
// share: the tile of a row, the cap of the rows' LDS table, a document's token count from the
// scan over the sentences, its fill-in-the-middle draw and its cost in the stream.
// include/lddl_amd.h states the semantics. Each translation unit gets its own copy.
#pragma once
#include "device.h"
#include "lddl_amd.h"

namespace lddl {
namespace {

constexpr int kStrTile = LDDL_STREAM_TILE;         // slots of a row per workgroup
constexpr int kStrThreads = 256;
constexpr int kStrItems = kStrTile / kStrThreads;  // consecutive slots per thread
constexpr int kStrLdsDocs = LDDL_STREAM_LDS_DOCS;  // places of a tile staged in LDS
static_assert(kStrItems == 4, "a thread stores two 16-byte vectors per output");
static_assert(kStrLdsDocs >= 2 && kStrLdsDocs <= kStrThreads, "a thread stages one place");

enum { kFimNone = 0, kFimPsm = 1, kFimSpm = 2 };

// The token table under the stream, and the stream's knobs (the plan and the rows take the same)
struct StreamSrc {
  const int64_t* dso;        // doc_sent_off[n_doc + 1]
  const int64_t* doc_order;  // nullable: identity
  const int64_t* sto;        // sent_tok_off[n_sent + 1], the scan of the masked sentence lengths
  int64_t n_sent, n_doc;
  uint32_t fim_q, spm_q;
  uint64_t seed, counter;
};

// One document as the stream sees it: its sentences [s0, s0 + ns), its first token's rank
// base = sto[s0] among all tokens of the table, t tokens, the layout and the cuts a <= b.
struct StreamDoc {
  int64_t s0, base;
  int32_t ns, t, a, b, kind;
  __device__ int32_t cost() const { return t + 1 + (kind != kFimNone ? 3 : 0); }
};

__device__ inline int64_t clamp_to(int64_t v, int64_t n) { return v < 0 ? 0 : (v > n ? n : v); }

// The document at place j. A place's document id outside [0, n_doc) is clamped (the order is
// the caller's to check; nothing is read out of bounds). A document holds fewer than 2^31 - 4
// tokens; a longer one is cut there.
__device__ inline StreamDoc stream_doc(const StreamSrc& S, int64_t j) {
  const int64_t d = clamp_to(S.doc_order ? S.doc_order[j] : j, S.n_doc - 1);
  StreamDoc D;
  D.s0 = clamp_to(S.dso[d], S.n_sent);
  int64_t s1 = clamp_to(S.dso[d + 1], S.n_sent);
  s1 = s1 < D.s0 ? D.s0 : s1;
  D.base = S.sto[D.s0];
  const int64_t t = S.sto[s1] - D.base, ns = s1 - D.s0;
  D.t = (int32_t)(t < INT32_MAX - 4 ? t : INT32_MAX - 4);
  D.ns = (int32_t)(ns < INT32_MAX ? ns : INT32_MAX);
  D.a = D.b = 0;
  D.kind = kFimNone;
  if (S.fim_q == 0 || D.t < 1) return D;
  const uint4 r = Philox::gen(make_uint4((uint32_t)d, (uint32_t)(d >> 32), (uint32_t)S.counter,
                                         (uint32_t)(S.counter >> 32)),
                              make_uint2((uint32_t)S.seed, (uint32_t)(S.seed >> 32)));
  if ((r.x >> 16) >= S.fim_q) return D;
  D.kind = (r.y >> 16) < S.spm_q ? kFimSpm : kFimPsm;
  const uint64_t m = (uint64_t)D.t + 1;
  const int32_t c0 = (int32_t)(((uint64_t)r.z * m) >> 32), c1 = (int32_t)(((uint64_t)r.w * m) >> 32);
  D.a = c0 < c1 ? c0 : c1;
  D.b = c0 < c1 ? c1 : c0;
  return D;
}

// What stands at offset o of a document's cost(d) stream positions
enum { kTokSource = 0, kTokEos = 1, kTokPre = 2, kTokSuf = 3, kTokMid = 4 };

// Offset o in [0, cost) -> the kind of token and, for kTokSource, its index *q in [0, t):
//   plain  the tokens, eos
//   PSM    <pre> [0, a) <suf> [b, t) <mid> [a, b) eos
//   SPM    <pre> <suf> [b, t) <mid> [0, a) [a, b) eos
__device__ inline int stream_map(const StreamDoc& D, int32_t o, int32_t* q) {
  *q = 0;
  if (o >= D.cost() - 1) return kTokEos;
  if (D.kind == kFimNone) {
    *q = o;
    return kTokSource;
  }
  if (o == 0) return kTokPre;
  const int32_t ns = D.t - D.b;  // the suffix
  if (D.kind == kFimPsm) {
    if (o <= D.a) { *q = o - 1; return kTokSource; }
    if (o == D.a + 1) return kTokSuf;
    if (o < D.a + 2 + ns) { *q = D.b + (o - D.a - 2); return kTokSource; }
    if (o == D.a + 2 + ns) return kTokMid;
    *q = D.a + (o - (D.a + 3 + ns));
    return kTokSource;
  }
  if (o == 1) return kTokSuf;
  if (o < 2 + ns) { *q = D.b + (o - 2); return kTokSource; }
  if (o == 2 + ns) return kTokMid;
  *q = o - (3 + ns);  // the prefix and the middle follow each other
  return kTokSource;
}

// cost(doc_order[j]): the functor of the plan's second scan
struct StreamCost {
  StreamSrc S;
  __device__ int64_t operator()(int64_t j) const { return stream_doc(S, j).cost(); }
};

// The largest j in [lo, hi) with Q[j] <= x, given Q[lo] <= x < Q[hi], by the whole wave: each
// step probes 64 points of the range, so a search takes log64 of the range in dependent loads
// where a lane's bisection takes log2. Every lane calls it with the same arguments.
__device__ inline int64_t wave_place(const int64_t* Q, int64_t lo, int64_t hi, int64_t x) {
  const int lane = lane_id();
  while (hi - lo > 1) {
    const int64_t span = hi - lo, step = (span + 63) >> 6;
    int64_t at = (lane + 1) * step;
    at = lo + (at < span ? at : span);  // the probes past the range read Q[hi] > x
    const int c = __popcll(ballot(Q[at] <= x));  // Q rises: the first c probes hold
    const int64_t up = (int64_t)(c + 1) * step, dn = (int64_t)c * step;
    hi = c < 64 && up < span ? lo + up : hi;
    lo = lo + (dn < span ? dn : span - 1);
    // c * step >= span would mean Q[hi] <= x; the clip only keeps a broken Q inside the range
  }
  return lo;
}

// the same by one lane (the rows' path past the LDS table, the offsets of cu_seqlens)
__device__ inline int64_t lane_place(const int64_t* Q, int64_t lo, int64_t hi, int64_t x) {
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (Q[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

}  // namespace
}  // namespace lddl
