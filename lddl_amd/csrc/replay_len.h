// The replay planner's view of the sentence lengths (pairs.hip): a document's lengths through a
// 64-entry register window (LenWin), and the slow path's token read (span_token). Device code of
// one unit (anonymous namespace).
#pragma once
#include "replay_rng.h"  // uni, rdlane

namespace lddl {
namespace {

// Sentence lengths of one document through a 64-entry register window (lane l: sentence
// wbase + l) with their inclusive prefix sum, so a chunk end is one ballot and a span's length
// two readlanes. Lengths are < 2^24 (lddl_tokenize caps max_pieces), so 64 of them fit int32.
struct LenWin {
  const int32_t* len;  // ks_len + first kept sentence of the doc
  int n, wbase;
  int32_t win, pre;
  uint64_t fl;  // lanes whose sentence holds a literal [CLS]/[SEP]
  __device__ void reset(const int32_t* p, int nn) { len = p; n = nn; wbase = -1024; }
  // the first window of a document loaded ahead (issued one document early, so the chain does not
  // wait for it), then taken as the window at sentence 0
  int32_t pfw;
  __device__ void prefetch(const int32_t* p, int nn) {
    const int k = (int)threadIdx.x;
    pfw = k < nn ? p[k] : 0;
  }
  __device__ void reset_prefetched(const int32_t* p, int nn) {
    len = p;
    n = nn;
    wbase = 0;
    win = pfw;
    pre = wave_incl_scan(win & kLenMask);
    fl = ballot((win & kLenHasClsSep) != 0);
  }
  __device__ bool has(int j) const { return (unsigned)(j - wbase) < 64u; }  // (j >= 0)
  __device__ void load(int j) {
    wbase = j;
    const int k = j + (int)threadIdx.x;
    win = k < n ? len[k] : 0;
    pre = wave_incl_scan(win & kLenMask);
    fl = ballot((win & kLenHasClsSep) != 0);
  }
  __device__ int32_t at(int j) {  // raw length word (flags included)
    if (!has(j)) load(j);
    return (int32_t)rdlane((uint32_t)win, j - wbase);
  }
  // total length of sentences [a, b) (a < b); ORs their flags into `flags`
  __device__ int64_t sum(int a, int b, int32_t& flags) {
    if (!has(a)) load(a);
    if (!has(b - 1)) {  // longer than a window: sequential
      int64_t s = 0;
      for (int j = a; j < b; ++j) {
        const int32_t w = at(j);
        s += w & kLenMask;
        flags |= w;
      }
      return s;
    }
    const int32_t hi = (int32_t)rdlane((uint32_t)pre, b - 1 - wbase);
    const int32_t lo = a > wbase ? (int32_t)rdlane((uint32_t)pre, a - 1 - wbase) : 0;
    if (fl) {  // (a window without literal [CLS]/[SEP] skips the span mask: the common case)
      const int cnt = b - a;
      const uint64_t m = fl >> (a - wbase);
      if ((cnt >= 64 ? m : (m & ((1ull << cnt) - 1))) != 0) flags |= kLenHasClsSep;
    }
    return hi - lo;
  }
  // the smallest i in [a, lim) with length(a .. i) >= T, else lim - 1 (a < lim <= n): the end of
  // the reference's accumulate-until-target loops (pretrain.py:276-280, 314-317)
  __device__ int find(int a, int lim, int64_t T) {
    if (!has(a)) load(a);
    // (window sums are < 2^31: 32-bit compares; two ballots combined by one scalar AND)
    const int32_t T32 = T < -1 ? -1 : T > INT32_MAX ? INT32_MAX : (int32_t)T;
    for (int pass = 0; pass < 2; ++pass) {
      const int32_t base = a > wbase ? (int32_t)rdlane((uint32_t)pre, a - 1 - wbase) : 0;
      const int j = wbase + (int)threadIdx.x;
      const uint64_t m = ballot((uint32_t)(j - a) < (uint32_t)(lim - a)) & ballot(pre - base >= T32);
      if (m) return wbase + __ffsll((unsigned long long)m) - 1;
      if (wbase + 64 >= lim) return lim - 1;
      if (pass == 0 && wbase != a) load(a);  // restart the window at a and look again
      else break;
    }
    int64_t s = 0;  // more than 64 sentences: sequential
    for (int i = a;; ++i) {
      s += at(i) & kLenMask;
      if (i == lim - 1 || s >= T) return i;
    }
  }
};

// token j (0-based) of the span that starts at kept sentence k0 (slow path only: a literal
// [CLS]/[SEP] in the pair), read from the tokenizer's layout
__device__ int32_t span_token(const PlanArgs& A, int64_t k0, int64_t j) {
  const int64_t x = A.kscan[k0] + j;
  int64_t k = k0;
  while (A.kscan[k + 1] <= x) ++k;
  return A.ids[A.ks_start[k] + (x - A.kscan[k])];
}

}  // namespace
}  // namespace lddl
