// Device helpers of the Punkt segmenter (segment.hip): the byte classes of nltk's regular
// expressions, UTF-8 and lowercasing, the tokens of a period context with their first- and
// second-pass annotation over the trained parameters, and the decision on one candidate
// (eval_candidate). Each translation unit gets its own copy (anonymous namespace).
#pragma once
#include "punkt_classes.h"
#include "punkt_params.h"

namespace lddl {
namespace {

// nltk _ORTHO_* flags
constexpr uint32_t kOBegUc = 2, kOMidUc = 4, kOUnkUc = 8, kOBegLc = 16, kOMidLc = 32, kOUnkLc = 64;
constexpr uint32_t kOUc = kOBegUc | kOMidUc | kOUnkUc, kOLc = kOBegLc | kOMidLc | kOUnkLc;

// ---- character classes ------------------------------------------------------------------------

__device__ __forceinline__ bool in_mask(uint32_t c, uint64_t lo, uint64_t hi) {
  return c < 64 ? ((lo >> c) & 1ull) : c < 128 ? ((hi >> (c - 64)) & 1ull) : false;
}
__device__ __forceinline__ bool non_word(uint32_t c) {  // [)";}\]*:@'({[?!]
  return in_mask(c, 0x8c00078600000000ull, 0x2800000028000001ull);
}
__device__ __forceinline__ bool word_start_excl(uint32_t c) {  // not in _re_word_start
  return in_mask(c, 0x0c00374c00000000ull, 0x2800000128000001ull);
}
__device__ __forceinline__ bool ortho_punct(uint32_t c) {  // ";:,.!?"
  return in_mask(c, 0x8c00500200000000ull, 0);
}
__device__ __forceinline__ bool sent_end(uint32_t c) { return c == '.' || c == '?' || c == '!'; }
__device__ __forceinline__ bool closing(uint32_t c) {
  return c == '"' || c == '\'' || c == ')' || c == ']' || c == '}';
}

// Text bytes: the wave's LDS slab when the index falls inside it, else global memory.
// (Explicit address spaces: a select between the two pointers would become flat loads, which
// wait on both the vector-memory and the LDS counters.)
typedef const __attribute__((address_space(3))) uint8_t* lds_u8_ptr;
typedef const __attribute__((address_space(1))) uint8_t* glb_u8_ptr;
struct Src {
  glb_u8_ptr x;
  lds_u8_ptr lds;
  int64_t lo, hi;
  __device__ Src(const uint8_t* gx, const void* l, int64_t lo_, int64_t hi_)
      : x((glb_u8_ptr)gx), lds((lds_u8_ptr)l), lo(lo_), hi(hi_) {}
  __device__ __forceinline__ uint32_t operator[](int64_t i) const {
    if (i >= lo && i < hi) return lds[i - lo];
    return x[i];
  }
};

// class bits of an ASCII code point, computed (the table agrees: tests/test_punkt.py)
__device__ __forceinline__ uint32_t ascii_props(uint32_t c) {
  const bool up = c - 'A' < 26u, lo = c - 'a' < 26u;
  return (ascii_space(c) ? kPSpace : 0u) | (up ? kPUpper : 0u) | (lo ? kPLower : 0u) |
         ((up || lo || c == '_') ? kPAlnod : 0u) | (c - '0' < 10u ? kPDigit : 0u);
}

__device__ __forceinline__ uint32_t props(const PunktTab& t, uint32_t cp) {
  if (cp < 128u) return ascii_props(cp);
  return class_bits(t.cls, cp);
}

__device__ __forceinline__ int utf8_len(uint32_t lead) {
  return lead < 0x80 ? 1 : lead < 0xE0 ? 2 : lead < 0xF0 ? 3 : 4;
}

// code point starting at byte i (a lead byte), bounded by e
__device__ inline uint32_t decode(const Src& s, int64_t i, int64_t e, int* len) {
  const uint32_t c = s[i];
  const int n = utf8_len(c);
  *len = n;
  if (n == 1) return c;
  uint32_t v = n == 2 ? (c & 31u) : n == 3 ? (c & 15u) : (c & 7u);
  for (int k = 1; k < n; ++k) v = (v << 6) | (i + k < e ? (s[i + k] & 63u) : 0u);
  return v;
}

// is the code point containing byte i whitespace (Python `\s`)
__device__ inline bool space_at(const PunktTab& t, const Src& s, int64_t i, int64_t b0, int64_t b1) {
  const uint32_t c = s[i];
  if (c < 0x80) return ascii_space(c);
  int64_t j = i;
  while (j > b0 && j > i - 3 && (s[j] & 0xC0u) == 0x80u) --j;
  int len;
  return (props(t, decode(s, j, b1, &len)) & kPSpace) != 0;
}

__device__ inline uint32_t lower_cp(const PunktTab& t, uint32_t cp, uint32_t* second) {
  *second = 0;
  if (cp < 128) return (cp >= 'A' && cp <= 'Z') ? cp + 32 : cp;
  int lo = 0, hi = t.n_lower - 1;
  while (lo <= hi) {
    const int mid = (lo + hi) >> 1;
    const uint32_t k = (uint32_t)t.lower[2 * mid];
    if (k == cp) {
      const int32_t v = t.lower[2 * mid + 1];
      if (v < 0) {  // U+0130 -> U+0069 U+0307
        *second = 0x307;
        return 0x69;
      }
      return (uint32_t)v;
    }
    if (k < cp) lo = mid + 1; else hi = mid - 1;
  }
  return cp;
}

__device__ inline int put_utf8(uint32_t v, uint8_t* o, int k) {
  if (k + 4 > kMaxKey + 1) return kMaxKey + 1;  // too long for any key
  if (v < 0x80) {
    o[k++] = (uint8_t)v;
  } else if (v < 0x800) {
    o[k++] = (uint8_t)(0xC0 | (v >> 6));
    o[k++] = (uint8_t)(0x80 | (v & 63));
  } else if (v < 0x10000) {
    o[k++] = (uint8_t)(0xE0 | (v >> 12));
    o[k++] = (uint8_t)(0x80 | ((v >> 6) & 63));
    o[k++] = (uint8_t)(0x80 | (v & 63));
  } else {
    o[k++] = (uint8_t)(0xF0 | (v >> 18));
    o[k++] = (uint8_t)(0x80 | ((v >> 12) & 63));
    o[k++] = (uint8_t)(0x80 | ((v >> 6) & 63));
    o[k++] = (uint8_t)(0x80 | (v & 63));
  }
  return k;
}

// ---- tokens of a context --------------------------------------------------------------------

struct Tok {
  int64_t s, e;       // bytes
  uint32_t c0;        // first code point
  int c0len;
  bool numeric;       // _RE_NUMERIC on the token -> type "##number##"
  bool period_final, sentbreak, abbr, ellipsis;
};

// type text of [s, e) (lowercased) or "##number##", into o; returns length (> kMaxKey: too long)
__device__ inline int type_text(const PunktTab& t, const Src& x, int64_t s, int64_t e, bool numeric,
                                uint8_t* o) {
  if (numeric) {
    const char* n = "##number##";
    for (int k = 0; k < 10; ++k) o[k] = (uint8_t)n[k];
    return 10;
  }
  int k = 0;
  for (int64_t i = s; i < e && k <= kMaxKey;) {
    int len;
    const uint32_t cp = decode(x, i, e, &len);
    uint32_t sec;
    k = put_utf8(lower_cp(t, cp, &sec), o, k);
    if (sec) k = put_utf8(sec, o, k);
    i += len;
  }
  return k;
}

__device__ inline int lookup(const PunktTab& t, uint32_t kind, const uint8_t* a, int la, const uint8_t* b,
                             int lb) {
  if (t.n_rec == 0 || la > kMaxKey || lb > kMaxKey) return -1;
  return find_param(t.hash, t.hmask, t.keys, kind, a, la, b, lb);
}

__device__ inline bool is_numeric(const PunktTab& t, const Src& x, int64_t s, int64_t e) {
  int64_t i = s;
  if (i < e && x[i] == '-') ++i;
  if (i < e && (x[i] == '.' || x[i] == ',')) ++i;
  int len;
  if (i >= e || !(props(t, decode(x, i, e, &len)) & kPDigit)) return false;
  i += len;
  while (i < e) {
    const uint32_t c = x[i];
    if (c == ',' || c == '.' || c == '-') {
      ++i;
      continue;
    }
    if (!(props(t, decode(x, i, e, &len)) & kPDigit)) return false;
    i += len;
  }
  return true;
}

// the token's type without a final period (PunktToken.type_no_period)
__device__ inline int type_no_period(const PunktTab& t, const Src& x, const Tok& k, uint8_t* o) {
  const bool strip = !k.numeric && k.period_final && k.e - k.s > 1;
  return type_text(t, x, k.s, k.e - (strip ? 1 : 0), k.numeric, o);
}
__device__ inline int type_no_sentperiod(const PunktTab& t, const Src& x, const Tok& k, uint8_t* o) {
  return k.sentbreak ? type_no_period(t, x, k, o) : type_text(t, x, k.s, k.e, k.numeric, o);
}

__device__ inline void make_tok(const PunktTab& t, const Src& x, int64_t s, int64_t e, Tok& k) {
  k.s = s;
  k.e = e;
  k.c0 = decode(x, s, e, &k.c0len);
  k.period_final = x[e - 1] == '.';
  // the type ("##number##" or not) is only consulted for period-final tokens and parameter keys
  k.numeric = (k.period_final || t.n_rec) ? is_numeric(t, x, s, e) : false;
  k.sentbreak = k.abbr = k.ellipsis = false;
  // _first_pass_annotation
  const int64_t n = e - s;
  if (n == 1 && sent_end(x[s])) {
    k.sentbreak = true;
    return;
  }
  bool dots = n >= 2;
  for (int64_t i = s; i < e && dots; ++i) dots = x[i] == '.';
  if (dots) {
    k.ellipsis = true;
    return;
  }
  if (k.period_final && !(n >= 2 && x[e - 2] == '.')) {
    bool hit = false;
    if (t.n_rec) {  // tok[:-1].lower() or its last '-' component in abbrev_types
      uint8_t buf[kMaxKey + 8];
      const int l = type_text(t, x, s, e - 1, false, buf);
      hit = lookup(t, kKAbbrev, buf, l, nullptr, 0) >= 0;
      if (!hit && l <= kMaxKey) {
        int d = l;
        while (d > 0 && buf[d - 1] != '-') --d;
        if (d > 0) hit = lookup(t, kKAbbrev, buf + d, l - d, nullptr, 0) >= 0;
      }
    }
    if (hit) k.abbr = true; else k.sentbreak = true;
  }
}

// _ortho_heuristic: 1 True, 0 False, 2 unknown
__device__ inline int ortho_heuristic(const PunktTab& t, const Src& x, const Tok& k) {
  if (k.e - k.s == 1 && ortho_punct(x[k.s])) return 0;
  uint32_t oc = 0;
  if (t.n_rec) {
    uint8_t buf[kMaxKey + 8];
    const int l = type_no_sentperiod(t, x, k, buf);
    const int v = lookup(t, kKOrtho, buf, l, nullptr, 0);
    oc = v < 0 ? 0u : (uint32_t)v;
  }
  const uint32_t p = props(t, k.c0);
  if ((p & kPUpper) && (oc & kOLc) && !(oc & kOMidUc)) return 1;
  if ((p & kPLower) && ((oc & kOUc) || !(oc & kOBegLc))) return 0;
  return 2;
}

// _second_pass_annotation of a given its successor b
__device__ inline void second_pass(const PunktTab& t, const Src& x, Tok& a, const Tok& b) {
  if (!a.period_final) return;
  const bool initial = a.e - a.s == a.c0len + 1 && (props(t, a.c0) & kPAlnod);
  uint8_t typ[kMaxKey + 8], nxt[kMaxKey + 8];
  int lt = 0, ln = 0;
  if (t.n_rec) {
    lt = type_no_period(t, x, a, typ);
    ln = type_no_sentperiod(t, x, b, nxt);
    if (lookup(t, kKColloc, typ, lt, nxt, ln) >= 0) {
      a.sentbreak = false;
      a.abbr = true;
      return;
    }
  }
  if ((a.abbr || a.ellipsis) && !initial) {
    if (ortho_heuristic(t, x, b) == 1) {
      a.sentbreak = true;
      return;
    }
    if ((props(t, b.c0) & kPUpper) && t.n_rec && lookup(t, kKStarter, nxt, ln, nullptr, 0) >= 0) {
      a.sentbreak = true;
      return;
    }
  }
  if (initial || a.numeric) {  // typ == "##number##" iff the token is numeric
    const int h = ortho_heuristic(t, x, b);
    if (h == 0) {
      a.sentbreak = false;
      a.abbr = true;
      return;
    }
    if (h == 2 && initial && (props(t, b.c0) & kPUpper)) {
      int v = t.n_rec ? lookup(t, kKOrtho, nxt, ln, nullptr, 0) : -1;
      if (!(v >= 0 && ((uint32_t)v & kOLc))) {
        a.sentbreak = false;
        a.abbr = true;
      }
    }
  }
}

// end-of-word lookahead of _word_tokenize_fmt at e inside a whitespace-free segment ending at se
__device__ inline bool word_end(const Src& x, int64_t e, int64_t se) {
  if (e >= se) return true;
  const uint32_t c = x[e];
  const uint32_t d = e + 1 < se ? x[e + 1] : 0u;
  if (non_word(c) || (c == '-' && d == '-') || (c == '.' && d == '.')) return true;
  if (c == ',') {
    if (e + 1 >= se || non_word(d)) return true;
    const uint32_t f = e + 2 < se ? x[e + 2] : 0u;
    return (d == '-' && f == '-') || (d == '.' && f == '.');
  }
  return false;
}

// next token of the whitespace-free segment [p, se); returns its end
__device__ inline int64_t next_word(const Src& x, int64_t p, int64_t se) {
  const uint32_t c = x[p];
  const uint32_t d = p + 1 < se ? x[p + 1] : 0u;
  if ((c == '-' || c == '.') && d == c) {  // MultiChar \-{2,} | \.{2,}
    int64_t e = p;
    while (e < se && x[e] == c) ++e;
    return e;
  }
  if (word_start_excl(c)) return p + 1;  // \S (ASCII)
  int64_t e = p + 1;  // (?=WordStart)\S+? up to the end lookahead
  while (!word_end(x, e, se)) ++e;
  return e;
}

// text_contains_sentbreak over the context: segment [s1, e1) then (if s2 < e2) [s2, e2)
__device__ inline bool contains_sentbreak(const PunktTab& t, const Src& x, int64_t s1, int64_t e1,
                                          int64_t s2, int64_t e2) {
  Tok cur, nxt;
  int64_t p = s1, se = e1;
  bool have = false;
  while (true) {
    if (p >= se) {
      if (se == e1 && s2 < e2) {
        p = s2;
        se = e2;
      } else {
        break;
      }
    }
    const int64_t e = next_word(x, p, se);
    if (!have) {
      make_tok(t, x, p, e, cur);
      have = true;
    } else {
      make_tok(t, x, p, e, nxt);
      second_pass(t, x, cur, nxt);
      if (cur.sentbreak) return true;
      cur = nxt;
    }
    p = e;
  }
  return false;
}

// One qualified sentence ender q: if it is the match of its run (the last qualified ender
// before the next whitespace), evaluate its period context; for a cut, its realigned boundary.
template <bool kParams>
__device__ inline bool eval_candidate(const PunktTab& t, const Src& src, int64_t i, int64_t b0, int64_t b1,
                                      int64_t rs, int64_t* bound) {
  int64_t s2 = 0, e2 = 0, e1 = i + 1, next_start;
  if (non_word(src[i + 1])) {
    // finditer takes the LAST qualified ender of the run: any later one in the run wins
    for (int64_t k = i + 1; k < rs; ++k) {
      if (space_at(t, src, k, b0, b1)) break;
      if (sent_end(src[k]) && k + 1 < rs && (non_word(src[k + 1]) || space_at(t, src, k + 1, b0, b1)))
        return false;
    }
    e1 = i + 2;  // context = match + the NonWord char
    next_start = i + 1;
  } else {
    s2 = i + 1;
    while (space_at(t, src, s2, b0, b1)) ++s2;  // non-whitespace exists before rs
    e2 = s2;
    while (e2 < b1 && !space_at(t, src, e2, b0, b1)) ++e2;
    next_start = s2;
  }
  int64_t run_start = i;  // the match starts at the run's first byte
  while (run_start > b0 && !space_at(t, src, run_start - 1, b0, b1)) --run_start;
  if (!contains_sentbreak(t, src, run_start, e1, s2, e2)) return false;
  // _realign_boundaries: a closing run followed by whitespace, "--" or the end moves left
  int64_t k = next_start;
  while (k < rs && closing(src[k])) ++k;
  const bool ok = k > next_start &&
                  (k >= rs || space_at(t, src, k, b0, b1) || (src[k] == '-' && k + 1 < b1 && src[k + 1] == '-'));
  *bound = ok ? k : next_start;
  return true;
}

}  // namespace
}  // namespace lddl
