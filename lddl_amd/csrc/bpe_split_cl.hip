// Byte-level BPE, the cl100k-style pre-tokenizer (Llama 3, GPT-4, Qwen2, DeepSeek):
//   (?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+
// (digit_group 1: \p{N} for \p{N}{1,3}) with bpe_split.hip's contract: one start bit per byte, one
// ballot per 64-byte tile. Most of the pattern is a function of a few characters each side and is
// decided from LDS codes with a halo, as in bpe_split.hip:
//   other       starts iff the character before is neither "other" nor U+0020 (which opened the
//               token); an apostrophe that starts and has a contraction behind it fires (ASCII in
//               either case, U+017F for s), and the character behind the contraction starts;
//   letter      the first of a run starts unless the character before absorbs it: a starting
//               "other" that did not fire, or white space other than \r and \n;
//   newline     starts iff the character before is a letter, a number or nothing (after "other"
//               it belongs to that token, after white space to the run's token);
//   white space other than a newline: starts after any non-space; after such white space iff a
//               non-space follows it (the last of the run is split off).
// Three decisions depend on a whole run of characters, which can cross any number of tiles:
//   (a) a digit starts iff its index in its run of digits, in characters, is a multiple of
//       digit_group;
//   (b), (c) white space other than a newline right behind a newline starts iff that newline
//       belongs to an "other" token (everything back to the run's start is newline and an
//       "other" stands before it), or no newline follows in its run of white space.
// Inside a tile these come from ballots of the class masks (a continuation byte counts with the
// class of its lead): run starts are mask & ~(mask << 1), an index is a popcount of lead bytes,
// a stop is a count of trailing zeros. Across tiles:
//   pass 1  one wave per tile leaves three bytes: the digits (mod 3) in the run at the tile's
//           tail, whether its tail is a newline run that an "other" owns, whether the white space
//           at its head holds a newline; or, for a tile that is one run all through (all digits,
//           all newlines, all other white space; no document start), that it passes on what
//           reaches it (kOpen, with the tile's digit count);
//   pass 2  lane = tile. A tile with kOpen takes the value of the nearest tile before it without
//           (behind it for (c)), by ballots inside the 64 tiles of a wave; a stretch that leaves
//           the wave's range is walked by that one wave, 64 tiles a step, so every stretch is
//           walked once and nothing waits on the host;
//   pass 3  decodes the tile again (the text is read twice; a tile keeps 3 bytes between the
//           passes, not its masks) with the carries of its two neighbours and writes the mask.
#include "bpe.h"
#include "bpe_split_dev.h"
#include "device.h"

namespace lddl {
namespace {

constexpr int kClThreads = 256, kClHalo = 16, kClWin = kClThreads + 2 * kClHalo;
constexpr uint8_t kNewline = 0x40;  // a code's flag: \r or \n
constexpr uint8_t kOpen = 4;        // a summary's flag: the tile is one run, its value is relative

// the codes and bytes of a workgroup's 256 positions and their halo; every thread calls it
__device__ inline void cl_window(const BpeTables& T, const BpeWork& W, int64_t first, uint8_t* code,
                                 uint8_t* byte) {
  for (int i = threadIdx.x; i < kClWin; i += kClThreads) {
    const int64_t x = first - kClHalo + i;
    uint8_t c = char_code(T, W, x);
    const uint8_t b = x >= 0 && x < W.n_bytes ? W.text[x] : 0;
    if (!(c & kOutside) && (b == 0x0A || b == 0x0D)) c |= kNewline;
    code[i] = c;
    byte[i] = b;
  }
  __syncthreads();
}

// the class of the character that window index i belongs to (its lead is at most 3 back)
__device__ inline int filled_class(const uint8_t* code, int i) {
  int k = 0;
  while (k < 3 && ((code[i - k] >> 2) & 7) == 0) ++k;
  return code[i - k] & 3;
}

// A tile's masks, bit = byte: the bytes of numbers, white space and others, the newlines, the
// document starts, the lead bytes; and the byte before the tile.
struct ClMasks {
  uint64_t num, space, other, nl, doc, lead;
  int prev;      // the class of the byte before the tile, kNone outside the text
  bool prev_nl;  // it is a newline
};

__device__ inline ClMasks cl_masks(const uint8_t* code, int i0) {
  const int i = i0 + lane_id();
  const uint8_t c = code[i];
  const bool in = !(c & kOutside);
  const int f = in ? filled_class(code, i) : kNone;
  ClMasks m;
  m.num = ballot(f == kBpeNumber);
  m.space = ballot(f == kBpeSpace);
  m.other = ballot(f == kBpeOther);
  m.nl = ballot(in && (c & kNewline));
  m.doc = ballot(in && (c & kDocStart));
  m.lead = ballot(in && ((c >> 2) & 7) != 0);
  const uint8_t pc = code[i0 - 1];
  m.prev = (pc & kOutside) ? kNone : filled_class(code, i0 - 1);
  m.prev_nl = !(pc & kOutside) && (pc & kNewline);
  return m;
}

// the starts of the runs of `run` in a tile: a byte of it whose byte before is none of it (bit 0:
// `joined` says that the byte before the tile is) or that starts a document
__device__ inline uint64_t run_starts(uint64_t run, uint64_t doc, bool joined) {
  return run & (~((run << 1) | (joined ? 1ull : 0ull)) | doc);
}

// ---- pass 1: a tile's three summaries, sum[c * n_tiles + tile] ----
__global__ void __launch_bounds__(kClThreads) bpe_cl_summary_kernel(BpeTables T, BpeWork W, uint8_t* sum) {
  __shared__ uint8_t code[kClWin + 8], byte[kClWin + 8];
  const int64_t first = (int64_t)blockIdx.x * kClThreads;
  cl_window(T, W, first, code, byte);
  const int w = wave_id();
  const int64_t tile = (first >> 6) + w;
  if (tile >= W.n_tiles) return;
  const ClMasks m = cl_masks(code, kClHalo + 64 * w);
  // (a) forward: the lead bytes, mod 3, of the run of digits at the tile's tail
  uint32_t sd = 0;
  if (m.num == ~0ull && !m.doc) {
    sd = kOpen | (__popcll(m.lead) % 3);
  } else if (m.num >> 63) {
    const int s = 63 - __builtin_clzll(run_starts(m.num, m.doc, false));
    sd = __popcll(m.lead & (~0ull << s)) % 3;
  }
  // (b) forward: the tile's tail is a run of newlines with an "other" before it. The run may be
  // empty: a tile that ends in an "other" hands 1 to a tile of newlines behind it (pass 3 reads
  // the value only where a run of newlines arrives from the tile before)
  uint32_t sa = (m.other >> 63) & 1;
  if (m.nl == ~0ull && !m.doc) {
    sa = kOpen;
  } else if (m.nl >> 63) {
    const int s = 63 - __builtin_clzll(run_starts(m.nl, m.doc, false));
    sa = s > 0 && !((m.doc >> s) & 1) && ((m.other >> (s - 1)) & 1);
  }
  // (c) backward: the white space that goes on from the tile before holds a newline
  uint32_t sc = 0;
  if ((m.space & 1) && !(m.doc & 1)) {
    const uint64_t stop = (~m.space | m.doc) & ~1ull;
    if (stop) sc = (m.nl & ((1ull << __builtin_ctzll(stop)) - 1)) != 0;
    else sc = m.nl ? 1 : kOpen;
  }
  if (lane_id() == 0) {
    sum[tile] = (uint8_t)sd;
    sum[W.n_tiles + tile] = (uint8_t)sa;
    sum[2 * W.n_tiles + tile] = (uint8_t)sc;
  }
}

// ---- pass 2: s[position] = kOpen | k becomes kOpen | (value of the position before + k) mod 3;
// position p is tile p, or tile n - 1 - p with `back`. One wave, positions p0 .. p0 + 63. A
// position past n counts as closed with value 0; tile 0 and tile n - 1 are never open (the
// text's first byte starts a document, byte n_bytes lies outside).
// The values are rewritten in place while other waves ballot over the same bytes. That is safe
// because every byte has one writer and no reader of what that writer changes: the flag never
// changes, so all waves see the same stretches; a closed tile is never written; an open tile is
// written by the wave whose range holds the closed tile its stretch starts behind, and by no
// other. That wave takes its counts from ballots made before it writes. The owner of a range
// uses only lanes from its first closed tile on (the open lanes below belong to a walker from
// an earlier range), and a walker uses only the lanes below the chunk's first closed tile f
// (the lanes from f on belong to the chunk's owner). ----
__device__ inline void cl_resolve(uint8_t* s, int64_t n, int64_t p0, bool back) {
  const int lane = lane_id();
  auto load = [&](int64_t p) { return p < n ? (uint32_t)s[back ? n - 1 - p : p] : 0u; };
  auto sum3 = [](uint64_t b1, uint64_t b2, uint64_t range) {
    return (uint32_t)(__popcll(b1 & range) + 2 * __popcll(b2 & range)) % 3;
  };
  int64_t p = p0 + lane;
  uint32_t e = load(p);
  uint64_t open = ballot(e & kOpen), b1 = ballot((e & 3) == 1), b2 = ballot((e & 3) == 2);
  const uint64_t closed_below = bpe_upto(~open, lane);
  if ((e & kOpen) && closed_below) {  // from the nearest closed tile of the wave's range
    const uint64_t range = bpe_upto(~0ull, lane) & (~0ull << (63 - __builtin_clzll(closed_below)));
    s[back ? n - 1 - p : p] = (uint8_t)(kOpen | sum3(b1, b2, range));
  }
  if (!(open >> 63) || open == ~0ull) return;  // no stretch leaves the range, or none starts in it
  uint32_t carry = sum3(b1, b2, ~0ull << (63 - __builtin_clzll(~open)));
  for (int64_t q0 = p0 + 64;; q0 += 64) {
    p = q0 + lane;
    e = load(p);
    open = ballot(e & kOpen), b1 = ballot((e & 3) == 1), b2 = ballot((e & 3) == 2);
    const int f = ~open ? __builtin_ctzll(~open) : 64;  // the stretch ends before lane f
    if (lane < f) s[back ? n - 1 - p : p] = (uint8_t)(kOpen | (carry + sum3(b1, b2, bpe_upto(~0ull, lane))) % 3);
    if (f < 64) return;
    carry = (carry + sum3(b1, b2, ~0ull)) % 3;
  }
}

__global__ void __launch_bounds__(256) bpe_cl_carry_kernel(uint8_t* sum, int64_t n_tiles) {
  const int64_t p0 = ((int64_t)blockIdx.x * 4 + wave_id()) * 64;
  if (p0 >= n_tiles) return;
  cl_resolve(sum, n_tiles, p0, false);
  cl_resolve(sum + n_tiles, n_tiles, p0, false);
  cl_resolve(sum + 2 * n_tiles, n_tiles, p0, true);
}

// ---- pass 3: the local rules ----
// the window index of the character before index i, -1 at a document start or the text's
__device__ inline int prev_index(const uint8_t* code, int i) {
  if (code[i] & kDocStart) return -1;
  int k = 1;
  while (k < 4 && ((code[i - k] >> 2) & 7) == 0) ++k;
  return (code[i - k] & kOutside) ? -1 : i - k;
}

// the bytes of the contraction that fires at window index a (2, or 3 for 're 've 'll and for
// ' U+017F), else 0
__device__ inline int cl_fires(const uint8_t* code, const uint8_t* byte, int a) {
  if ((code[a] & kOutside) || byte[a] != 0x27) return 0;
  bool is20;
  const int p = prev_class(code, byte, a, &is20);
  if (p == kBpeOther || is20) return 0;  // the apostrophe is no token start
  if ((code[a + 1] & (kOutside | kDocStart))) return 0;
  const uint8_t b1 = byte[a + 1] | 0x20;  // an ASCII letter in lower case, or no letter of the list
  if (b1 == 's' || b1 == 't' || b1 == 'm' || b1 == 'd') return 2;
  if ((code[a + 2] & (kOutside | kDocStart))) return 0;
  if (byte[a + 1] == 0xC5 && byte[a + 2] == 0xBF && ((code[a + 1] >> 2) & 7) == 2) return 3;
  const uint8_t b2 = byte[a + 2] | 0x20;
  return ((b1 == 'r' && b2 == 'e') || (b1 == 'v' && b2 == 'e') || (b1 == 'l' && b2 == 'l')) ? 3 : 0;
}

__global__ void __launch_bounds__(kClThreads) bpe_cl_split_kernel(BpeTables T, BpeWork W, int digit_group,
                                                                 const uint8_t* sum) {
  __shared__ uint8_t code[kClWin + 8], byte[kClWin + 8];
  const int64_t first = (int64_t)blockIdx.x * kClThreads;
  cl_window(T, W, first, code, byte);
  const int w = wave_id(), lane = lane_id();
  const int64_t tile = (first >> 6) + w;
  if (tile >= W.n_tiles) return;
  const ClMasks m = cl_masks(code, kClHalo + 64 * w);
  const int i = kClHalo + 64 * w + lane;
  const uint8_t c = code[i];
  const uint64_t below = (1ull << lane) - 1;
  bool start;
  if (c & (kOutside | kDocStart)) {
    start = true;
  } else if (((c >> 2) & 7) == 0) {
    start = false;
  } else {
    const int cls = c & 3, len = (c >> 2) & 7;
    const int pi = prev_index(code, i);
    const int p = pi < 0 ? kNone : code[pi] & 3;
    const bool p20 = pi >= 0 && byte[pi] == 0x20, pnl = pi >= 0 && (code[pi] & kNewline);
    if (cls == kBpeNumber) {
      int k = 0;
      if (digit_group > 1) {  // (a): the leads between the run's start and this one
        const uint64_t rs = bpe_upto(run_starts(m.num, m.doc, m.prev == kBpeNumber), lane);
        if (rs) k = __popcll(m.lead & below & (~0ull << (63 - __builtin_clzll(rs))));
        else k = (tile > 0 ? sum[tile - 1] & 3 : 0) + __popcll(m.lead & below);  // the run comes from the tile before
      }
      start = k % digit_group == 0;
    } else if (cls == kBpeOther) {
      start = !(p == kBpeOther || p20);
    } else if (cls == kBpeLetter) {
      const int f1 = cl_fires(code, byte, i - 1), f2 = cl_fires(code, byte, i - 2);
      if (f1 > 0 || f2 == 3) start = false;
      else if (f2 == 2 || cl_fires(code, byte, i - 3) == 3) start = true;
      else if (p == kBpeLetter) start = false;
      else if (p == kBpeSpace) start = pnl;
      else if (p == kBpeOther) {  // a single starting "other" takes the letters with it
        bool pp20;
        const int pp = prev_class(code, byte, pi, &pp20);
        start = pp == kBpeOther || pp20;
      } else start = true;
    } else if (c & kNewline) {
      start = p != kBpeSpace && p != kBpeOther;
    } else if (p != kBpeSpace) {
      start = true;
    } else if (!pnl) {
      const uint8_t nc = code[i + len];
      start = !(nc & (kOutside | kDocStart)) && (nc & 3) != kBpeSpace;
    } else {
      // (b): the run of newlines that ends right before this byte
      const uint64_t rs = lane ? bpe_upto(run_starts(m.nl, m.doc, m.prev_nl), lane - 1) : 0;
      bool owned;
      if (rs) {
        const int s = 63 - __builtin_clzll(rs);
        owned = !((m.doc >> s) & 1) && (s > 0 ? (m.other >> (s - 1)) & 1 : m.prev == kBpeOther);
      } else {
        owned = tile > 0 && (sum[W.n_tiles + tile - 1] & 1);  // it comes from the tile before
      }
      // (c): a newline between this byte and the end of its run of white space
      const uint64_t stop = bpe_above(~m.space | m.doc, lane);
      bool follows;
      if (stop) follows = (bpe_above(m.nl, lane) & ((1ull << __builtin_ctzll(stop)) - 1)) != 0;
      else follows = bpe_above(m.nl, lane) != 0 || (tile + 1 < W.n_tiles && (sum[2 * W.n_tiles + tile + 1] & 1));
      start = owned || !follows;
    }
  }
  const uint64_t M = ballot(start);
  if (lane == 0) W.start_bits[tile] = M;
}

}  // namespace

hipError_t bpe_launch_split_cl(const BpeTables& T, const BpeWork& W, int64_t clear_words,
                               int digit_group, uint8_t* run_tmp, hipStream_t st) {
  const hipError_t e = bpe_launch_docs(W, clear_words, st);
  if (e != hipSuccess) return e;
  const unsigned blocks = (unsigned)((W.n_tiles + 3) / 4);
  hipLaunchKernelGGL(bpe_cl_summary_kernel, dim3(blocks), dim3(kClThreads), 0, st, T, W, run_tmp);
  hipLaunchKernelGGL(bpe_cl_carry_kernel, dim3((unsigned)((W.n_tiles + 255) / 256)), dim3(256), 0, st,
                     run_tmp, W.n_tiles);
  hipLaunchKernelGGL(bpe_cl_split_kernel, dim3(blocks), dim3(kClThreads), 0, st, T, W, digit_group,
                     (const uint8_t*)run_tmp);
  return hipGetLastError();
}

}  // namespace lddl
