// Tokenizer, the lane kernel (unit map: tokenize.hip): one lane per listed sentence, sequential,
// with no bound on a word's length but WordPiece's own 100-char rule. It takes the sentences the
// streaming and wave kernels put on the fallback list, and the whole input with
// LDDL_TOKENIZE_PATH=lane.
#include <algorithm>

#include "tokenize_dev.h"
#include "tokenize_plan.h"

namespace lddl {
namespace {

constexpr int kBlock = 128;       // threads per workgroup
constexpr int kWordStride = 420;  // bytes per lane word buffer: 100 chars * 4 B + pad; 105
                                  // dwords (odd) so lanes hit distinct LDS banks

// Vocab lookup of w[s, s+len) with or without the "##" continuation prefix.
__device__ int32_t lookup(const Tables& T, const uint8_t* w, int s, int len, uint32_t cont) {
  uint64_t k0 = 0;
  uint32_t k1 = 0;
  const int n0 = len < 8 ? len : 8;
  for (int i = 0; i < n0; ++i) k0 |= (uint64_t)w[s + i] << (8 * i);
  for (int i = 8; i < len && i < 12; ++i) k1 |= (uint32_t)w[s + i] << (8 * (i - 8));
  const uint32_t want = kMetaValid | (cont ? kMetaCont : 0u) | (len > 12 ? kMetaLong : 0u) |
                        ((uint32_t)len << 21);
  for (uint32_t slot = (uint32_t)vhash(k0, k1, len, cont) & T.vmask;; slot = (slot + 1) & T.vmask) {
    const VEnt e = T.vhash[slot];
    if (!(e.meta & kMetaValid)) return -1;
    if (e.k0 == k0 && e.k1 == k1 && (e.meta & ~0x1FFFFFu) == want) {
      const int32_t id = meta_id(e.meta);
      if (len <= 12) return id;
      const uint8_t* p = T.vbytes + T.voff[id];
      bool ok = true;
      for (int i = 12; i < len; ++i) ok &= p[i] == w[s + i];
      if (ok) return id;
    }
  }
}

struct Sink {
  int32_t* out;  // sentence region ids[sent_off[s] ...]
  int32_t n;     // pieces emitted so far (may run past max_pieces inside the region)
};

// Greedy longest-match WordPiece of one normalised word (HF tokenizers WordPiece::tokenize).
__device__ void wordpiece(const Tables& T, const uint8_t* w, int nb, int nc, bool overflow,
                          Sink& sk) {
  if (nc == 0) return;
  if (overflow || nc > 100) { sk.out[sk.n++] = T.special_id[kUnk]; return; }
  const int first = sk.n;
  int start = 0;
  while (start < nb) {
    int end = nb < start + T.max_piece_bytes ? nb : start + T.max_piece_bytes;
    int32_t found = -1;
    for (; end > start; --end) {
      if (end < nb && (w[end] & 0xC0) == 0x80) continue;  // not a char boundary
      found = lookup(T, w, start, end - start, start > 0);
      if (found >= 0) break;
    }
    if (found < 0) {
      sk.n = first;
      sk.out[sk.n++] = T.special_id[kUnk];
      return;
    }
    sk.out[sk.n++] = found;
    start = end;
  }
}

__global__ void __launch_bounds__(kBlock) tokenize_lane_kernel(
    Tables T, const uint8_t* __restrict__ text, const int64_t* __restrict__ sent_off,
    int64_t n_sent, int32_t max_pieces, int32_t* __restrict__ ids, int32_t* __restrict__ sent_len,
    const int32_t* __restrict__ list, const uint32_t* __restrict__ list_n) {
  __shared__ uint8_t wbuf_all[kBlock * kWordStride];
  const int64_t n_items = list ? (int64_t)*list_n : n_sent;
  for (int64_t it = (int64_t)blockIdx.x * kBlock + threadIdx.x; it < n_items;
       it += (int64_t)gridDim.x * kBlock) {
  const int64_t s = list ? (int64_t)list[it] : it;
  uint8_t* w = wbuf_all + threadIdx.x * kWordStride;
  const int64_t b0 = sent_off[s], b1 = sent_off[s + 1];
  Sink sk{ids + b0, 0};
  int32_t flags = 0;
  int nb = 0, nc = 0;
  bool ovf = false;
  int64_t i = b0;
  while (i < b1 && sk.n < max_pieces) {
    if (text[i] == '[') {
      int best = -1;
      for (int k = 0; k < kNumSpecial; ++k)
        if (T.special_id[k] >= 0 && match_special(text, i, b1, k)) { best = k; break; }
      if (best >= 0) {
        wordpiece(T, w, nb, nc, ovf, sk);
        nb = nc = 0;
        ovf = false;
        if (sk.n < max_pieces && (best == kCls || best == kSep)) flags = kLenHasClsSep;
        sk.out[sk.n++] = T.special_id[best];
        i += best == kMask ? 6 : 5;
        continue;
      }
    }
    const uint32_t cp = utf8_next(text, b1, i);
    const uint32_t e = tab_entry(T, cp);
    const uint32_t cls = e >> 30;
    if (cls == kDrop) continue;
    if (cls == kSpace) {
      wordpiece(T, w, nb, nc, ovf, sk);
      nb = nc = 0;
      ovf = false;
      continue;
    }
    uint8_t ob[12];
    int olen, ochars = 1;
    if (e & kIdent) olen = put_utf8(ob, cp);
    else if (e & kMulti) {
      const uint8_t* p = T.pool + (e & 0xFFFFFFu);
      olen = p[0];
      ochars = p[1];
      for (int k = 0; k < olen; ++k) ob[k] = p[2 + k];
    } else olen = put_utf8(ob, e & 0x1FFFFFu);
    if (cls == kIso) {
      wordpiece(T, w, nb, nc, ovf, sk);
      for (int k = 0; k < olen; ++k) w[k] = ob[k];
      wordpiece(T, w, olen, 1, false, sk);
      nb = nc = 0;
      ovf = false;
      continue;
    }
    if (ovf || nc + ochars > 100) { ovf = true; nc += ochars; continue; }
    for (int k = 0; k < olen; ++k) w[nb + k] = ob[k];
    nb += olen;
    nc += ochars;
  }
  if (sk.n < max_pieces) wordpiece(T, w, nb, nc, ovf, sk);
  sent_len[s] = (sk.n < max_pieces ? sk.n : max_pieces) | flags;
  }
}

}  // namespace

int launch_lane(const TokCall& T, int64_t s0, int64_t n, int64_t grid_cap, bool whole) {
  const int64_t grid = std::min<int64_t>((n + kBlock - 1) / kBlock, grid_cap);
  hipLaunchKernelGGL(tokenize_lane_kernel, dim3((unsigned)grid), dim3(kBlock), 0, T.st, T.c->tab,
                     T.d_text, T.d_sent_off + s0, n, T.max_pieces, T.d_ids, T.d_sent_len + s0,
                     whole ? nullptr : T.fb + kFbHead,
                     whole ? nullptr : reinterpret_cast<const uint32_t*>(T.fb));
  LDDL_HIP(hipGetLastError());
  return 0;
}

}  // namespace lddl
