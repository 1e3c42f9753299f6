// Byte-level BPE, the pre-tokenizer: GPT-2's pattern
//   's|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+
// as a local function of a few characters each side, lane = byte, one start bit per byte.
//
// A workgroup takes 256 bytes and a halo of 16 each side. Stage A: every position of the window
// decodes its own character (a lead byte with all its continuation bytes inside the document;
// any other byte is a character of class "other" by itself) and leaves one code byte in LDS:
// class, length (0: a continuation byte that a lead claims), document start, outside the text.
// Stage B: a lane reads the codes of the character before it (at most 4 bytes back), of the one
// after it, and of the three bytes that can hold an apostrophe whose contraction covers or ends
// at it, and decides:
//   white space   starts a token iff the character before is none or no white space (the run
//                 starts), or the one after is a non-space (the run's last character is split
//                 off: a U+0020 opens the next token, another one is a token by itself);
//   a non-space   after nothing or after white space other than U+0020 starts; after U+0020 it
//                 never does (the space opened its token); inside a fired contraction it does
//                 not; right after one it does; else it starts iff its class differs from the
//                 class before;
//   a contraction fires at an apostrophe that is at a token start: before it a letter, a
//                 number, white space other than U+0020, or nothing.
// A document's first byte always starts (the match restarts there) and nothing is read across
// it: before it is "none", and the last character of the document before has "none" after it.
// One ballot per wave writes the 64-bit start mask of a tile; every byte from n_bytes on counts
// as a start, so the last pre-token ends at the text's end.
#include "bpe.h"
#include "bpe_split_dev.h"
#include "device.h"

namespace lddl {
namespace {

constexpr int kSplitThreads = 256, kHalo = 16, kWin = kSplitThreads + 2 * kHalo;

__global__ void __launch_bounds__(256) bpe_clear_kernel(uint64_t* p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0;
}

__global__ void __launch_bounds__(256) bpe_mark_docs_kernel(BpeWork W) {
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t n = W.doc_sent_off ? W.n_doc : W.n_sent;
  if (d >= n) return;
  const int64_t s = W.doc_sent_off ? W.doc_sent_off[d] : d;
  if (s < 0 || s > W.n_sent) return;
  const int64_t x = W.sent_off[s];
  if (x >= 0 && x < W.n_bytes)
    atomicOr(reinterpret_cast<unsigned long long*>(W.doc_bits + (x >> 6)), 1ull << (x & 63));
}

// 2 or 3 if a contraction fires at window index a, else 0
__device__ inline int fires(const uint8_t* code, const uint8_t* byte, int a) {
  if ((code[a] & kOutside) || byte[a] != 0x27) return 0;
  bool is20;
  const int p = prev_class(code, byte, a, &is20);
  if (p == kBpeOther || is20) return 0;  // the apostrophe is no token start
  if ((code[a + 1] & (kOutside | kDocStart))) return 0;
  const uint8_t b1 = byte[a + 1];
  if (b1 == 's' || b1 == 't' || b1 == 'm' || b1 == 'd') return 2;
  if ((code[a + 2] & (kOutside | kDocStart))) return 0;
  const uint8_t b2 = byte[a + 2];
  return ((b1 == 'r' && b2 == 'e') || (b1 == 'v' && b2 == 'e') || (b1 == 'l' && b2 == 'l')) ? 3 : 0;
}

__global__ void __launch_bounds__(kSplitThreads) bpe_split_kernel(BpeTables T, BpeWork W) {
  __shared__ uint8_t code[kWin + 8], byte[kWin + 8];
  const int64_t first = (int64_t)blockIdx.x * kSplitThreads;
  for (int i = threadIdx.x; i < kWin; i += kSplitThreads) {
    const int64_t x = first - kHalo + i;
    code[i] = char_code(T, W, x);
    byte[i] = x >= 0 && x < W.n_bytes ? W.text[x] : 0;
  }
  __syncthreads();
  const int i = threadIdx.x + kHalo;
  const uint8_t c = code[i];
  bool start;
  if (c & kOutside) {
    start = true;
  } else if (c & kDocStart) {
    start = true;
  } else if (((c >> 2) & 7) == 0) {
    start = false;
  } else {
    const int cls = c & 3, len = (c >> 2) & 7;
    bool p20;
    const int p = prev_class(code, byte, i, &p20);
    const uint8_t nc = code[i + len];
    const int nx = (nc & (kOutside | kDocStart)) ? kNone : (nc & 3);
    if (cls == kBpeSpace) {
      start = p != kBpeSpace || (nx != kNone && nx != kBpeSpace);
    } else if (p == kNone) {
      start = true;
    } else if (p20) {
      start = false;
    } else if (p == kBpeSpace) {
      start = true;
    } else {
      const int f1 = fires(code, byte, i - 1), f2 = fires(code, byte, i - 2);
      if (f1 > 0 || f2 == 3) start = false;
      else if (f2 == 2 || fires(code, byte, i - 3) == 3) start = true;
      else start = cls != p;
    }
  }
  const uint64_t m = ballot(start);
  const int64_t tile = (first >> 6) + (threadIdx.x >> 6);
  if (lane_id() == 0 && tile < W.n_tiles) W.start_bits[tile] = m;
}

}  // namespace

hipError_t bpe_launch_docs(const BpeWork& W, int64_t clear_words, hipStream_t st) {
  hipLaunchKernelGGL(bpe_clear_kernel, dim3((unsigned)((clear_words + 255) / 256)), dim3(256), 0, st,
                     W.doc_bits, clear_words);
  const int64_t nd = W.doc_sent_off ? W.n_doc : W.n_sent;
  if (nd > 0)
    hipLaunchKernelGGL(bpe_mark_docs_kernel, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, st, W);
  return hipGetLastError();
}

hipError_t bpe_launch_split(const BpeTables& T, const BpeWork& W, int64_t clear_words, hipStream_t st) {
  const hipError_t e = bpe_launch_docs(W, clear_words, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(bpe_split_kernel, dim3((unsigned)((W.n_tiles + 3) / 4)), dim3(kSplitThreads), 0,
                     st, T, W);
  return hipGetLastError();
}

}  // namespace lddl
