// Tokenizer, the wave kernel (unit map: tokenize.hip): the round-1 design, one wavefront per
// sentence with no cross-sentence queue, kept only as the LDDL_TOKENIZE_PATH=wave diagnostic. A
// wave reads its sentence in 64-byte windows, one byte per lane; ballots find the window's
// pre-tokenizer units, each lane resolves one unit (unit_word and wordpiece32, as phase B of the
// streaming kernel), and a scan places the pieces. The next window starts at the first byte of
// the unit the window cut. A unit that does not fit (>= 64 bytes, > kNorm normalised bytes,
// > kPcs pieces) sends its sentence to the fallback list.
#include <algorithm>

#include "tokenize_dev.h"
#include "tokenize_plan.h"

namespace lddl {
namespace {

constexpr int kTW = 4;     // waves per workgroup

struct alignas(16) WaveLds {
  uint8_t us[64], ue[64], uk[64];  // unit k: first byte, last byte (window-relative), kind
  int32_t pcs[kPcs * 64];          // lane l's pieces at pcs[64 q + l]
  alignas(16) uint8_t nrm[64 * kNorm];  // lane l's normalised word (generic path)
};

// Classification of one 64-byte window [pos, pos+64) of a sentence ending at b1 (one byte per
// lane). Returns, in registers, the window's complete units as masks (US: first bytes, UE: last
// bytes; unit k = the k-th bit of each), each start lane's unit kind (0 word run, 1 isolated
// char, 2 + k literal special token k), the start of the next window and the mask of lanes
// holding a byte the register fast path cannot take. The caller stores what it needs.
struct WinResult {
  int n_units;
  int64_t next;  // the next window starts at this byte (b1: the sentence is consumed to its end)
  uint64_t slow;
  uint64_t US, UE;  // unit starts (a trailing incomplete unit included) / complete unit ends
  int ukind;        // this lane's unit kind when its US bit is set
  bool fallback;    // a unit of >= 64 bytes: the sentence goes to the lane kernel
};

// byte = text[pos + lane] (any value at or past b1)
__device__ WinResult classify_window(const Tables& T, const uint32_t* s_ascii,
                                     const uint8_t* __restrict__ text, int64_t pos, int64_t b1,
                                     uint32_t byte) {
  const int lane = lane_id();
  const int64_t i = pos + lane;
  const bool in = i < b1;
  const bool tail_known = pos + 64 >= b1;  // the byte after lane 63 is past the sentence's end
  // ASCII bytes for every lane without a branch (beyond the sentence: a separator); the
  // non-ASCII and '[' lanes are revisited only in windows that have them (wave-uniform tests,
  // so a plain window runs no exec-mask branches here)
  const uint32_t ascii_e = s_ascii[byte & 127u];  // (read by every lane: no branch)
  uint32_t cls = in ? ascii_e >> 30 : kSpace;
  int cplen = 1;          // bytes of the code point starting here (0: covered continuation)
  int spk = -1;           // literal special token starting here
  bool slow = in && cls == kDrop;  // non-ASCII or dropped char: not for the register fast path
  bool cont = false;
  if (ballot(in && byte >= 0x80)) {
    if (in && byte >= 0xC0) {
      int64_t j = i;
      const uint32_t cp = utf8_next(text, b1, j);
      cplen = (int)(j - i);
      cls = tab_entry(T, cp) >> 30;
      slow = true;
    } else if (in && byte >= 0x80) {
      cont = true;  // resolved below: covered by a valid lead, or a lone byte (U+FFFD, drop)
      cls = kDrop;
      slow = true;
    }
  }
  if (ballot(in && byte == '[')) {
    if (in && byte == '[') spk = match_special_at(T, text, i, b1);
  }
  const uint64_t V2 = ballot(cplen == 2), V3 = ballot(cplen == 3), V4 = ballot(cplen == 4);
  bool cp_last = cplen <= 1;
  if (V2 | V3 | V4) {  // multi-byte code points in the window (wave-uniform branch)
    const uint64_t C1 = (V2 | V3 | V4) << 1, C2 = (V3 | V4) << 2, C3 = V4 << 3;
    const bool covered = cont && (((C1 | C2 | C3) >> lane) & 1ull);
    const int dist = !covered ? 0 : ((C1 >> lane) & 1ull) ? 1 : ((C2 >> lane) & 1ull) ? 2 : 3;
    // a covered continuation inherits its lead's class; cp_last marks a code point's last byte
    const int lead_len = __shfl((int)(cls | ((uint32_t)cplen << 4)), lane - dist, 64);
    if (covered) {
      cls = (uint32_t)lead_len & 3u;
      cplen = 0;
    }
    cp_last = covered ? (dist == (lead_len >> 4) - 1) : (cplen <= 1);
  }
  const uint64_t S = ballot(spk >= 0), S6 = ballot(spk == kMask);
  const uint64_t inside = (S << 1) | (S << 2) | (S << 3) | (S << 4) | (S6 << 5);
  const bool in_sp = ((S | inside) >> lane) & 1ull;
  const uint32_t cat = in_sp ? kCatSpecial : cls == kSpace ? kCatSep : cls == kIso ? kCatIso : kCatRun;
  const uint64_t RUN = ballot(cat == kCatRun);
  const uint64_t LEAD = ballot(cplen > 0);
  const uint64_t ISO = ballot(cat == kCatIso);
  const uint64_t CPL = ballot(cp_last);
  WinResult R;
  R.slow = ballot(slow);
  R.fallback = false;
  R.ukind = spk >= 0 ? 2 + spk : cat == kCatIso ? 1 : 0;
  R.next = b1;
  R.US = S | (ISO & LEAD) | (RUN & ~(RUN << 1));
  uint64_t RE = RUN & ~(RUN >> 1);
  if (!tail_known) RE &= ~(1ull << 63);
  R.UE = ((S & ~S6) << 4) | (S6 << 5) | (ISO & CPL & ~inside) | RE;
  R.n_units = __popcll(R.UE);
  if (__popcll(R.US) > R.n_units) {  // the window cuts its last unit: the next one starts there
    const int last = 63 - __clzll(R.US);
    if (last == 0) R.fallback = true;  // a unit of >= 64 bytes
    else R.next = pos + last;
  } else if (!tail_known) {
    // a separator code point straddling the window end restarts the next window at its lead
    const int hl = 63 - __clzll(LEAD);
    const int hc = 63 - __clzll(CPL);
    R.next = pos + (hl > hc ? hl : 64);
  }
  return R;
}

// The window's units as arrays (W.us / W.ue / W.uk, unit k at index k): the kernel gives one
// unit to each lane.
__device__ inline void store_units(const WinResult& R, WaveLds& W) {
  const int lane = lane_id();
  if ((R.US >> lane) & 1ull) {
    const int k = (int)popc_below(R.US);
    W.us[k] = (uint8_t)lane;
    W.uk[k] = (uint8_t)R.ukind;
  }
  if ((R.UE >> lane) & 1ull) W.ue[popc_below(R.UE)] = (uint8_t)lane;
  wave_sync();
}

// Pieces of one pre-tokenizer unit (text[start, start+len), kind as classify_window): written to
// pc[64 * q]; returns the count (0: every char of the unit is dropped), or -1 when the unit needs
// the lane kernel (> kPcs pieces or a normalised word > kNorm bytes). cs_flag: the unit is a
// literal [CLS] / [SEP]. The word goes through the lane's LDS row `w` unless it is ASCII.
__device__ int unit_pieces(const Tables& T, const uint32_t* bloom, const uint32_t* s_ascii,
                           const uint8_t* __restrict__ text, int64_t n_bytes, int64_t start,
                           int len, int kind, bool unit_slow, Pcs& pc, uint8_t* w,
                           bool& cs_flag) {
  cs_flag = false;
  if (kind >= 2) {
    pc.put(0, T.special_id[kind - 2]);
    cs_flag = kind - 2 == kCls || kind - 2 == kSep;
    return 1;
  }
  const UnitWord u = unit_word(T, s_ascii, text, n_bytes, start, len, unit_slow, w, false);
  if (u.status) return u.status < 0 ? -1 : 0;
  return wordpiece32(T, bloom, u.v, u.nb, u.ends, pc);
}

__global__ void __launch_bounds__(64 * kTW) tokenize_wave_kernel(
    Tables T, const uint8_t* __restrict__ text, int64_t n_bytes, const int64_t* __restrict__ sent_off,
    int64_t n_sent, int32_t max_pieces, int32_t* __restrict__ ids, int32_t* __restrict__ sent_len,
    int32_t* __restrict__ fb_list, uint32_t* __restrict__ fb_n) {
  __shared__ uint32_t s_ascii[128];
  __shared__ WaveLds s_w[kTW];
  for (int c = threadIdx.x; c < 128; c += blockDim.x) s_ascii[c] = tab_entry(T, (uint32_t)c);
  __syncthreads();
  const int lane = lane_id();
  WaveLds& W = s_w[threadIdx.x >> 6];
  const int64_t stride = (int64_t)gridDim.x * kTW;
  for (int64_t s = (int64_t)blockIdx.x * kTW + wave_id(); s < n_sent; s += stride) {
    const int64_t b0 = sent_off[s], b1 = sent_off[s + 1];
    int64_t pos = b0;
    int32_t emitted = 0, flags = 0;
    bool fallback = false;
    while (pos < b1 && emitted < max_pieces) {
      const uint32_t byte = pos + lane < b1 ? text[pos + lane] : 0x20u;
      const WinResult R = classify_window(T, s_ascii, text, pos, b1, byte);
      if (R.fallback) { fallback = true; break; }
      store_units(R, W);
      int npc = 0;
      bool cs_flag = false;
      Pcs pc{W.pcs + lane};
      if (lane < R.n_units) {
        const int us = W.us[lane], ue = W.ue[lane], kind = W.uk[lane];
        const int ulen = ue - us + 1;
        const bool unit_slow = ((R.slow >> us) & (ulen >= 64 ? ~0ull : ((1ull << ulen) - 1))) != 0;
        npc = unit_pieces(T, T.bloom, s_ascii, text, n_bytes, pos + us, ulen, kind, unit_slow, pc,
                          W.nrm + lane * kNorm, cs_flag);
      }
      if (ballot(npc < 0)) { fallback = true; break; }
      const int incl = wave_incl_scan(npc);
      const int o = emitted + incl - npc;
      for (int q = 0; q < npc; ++q)
        if (o + q < max_pieces) ids[b0 + o + q] = pc.get(q);
      if (ballot(cs_flag && o < max_pieces)) flags = kLenHasClsSep;
      emitted += __shfl(incl, 63, 64);
      pos = R.next;
      wave_sync();
    }
    if (fallback) {
      if (lane == 0) fb_list[atomicAdd(fb_n, 1u)] = (int32_t)s;
    } else if (lane == 0) {
      sent_len[s] = (emitted < max_pieces ? emitted : max_pieces) | flags;
    }
  }
}

}  // namespace

int tokenize_wave(const TokCall& T) {
  int per_cu = 0;
  LDDL_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, tokenize_wave_kernel, 64 * kTW, 0));
  const int64_t want = (T.n_sent + kTW - 1) / kTW;
  const int64_t grid = std::min<int64_t>(want, T.n_cu * std::max(per_cu, 1));
  hipLaunchKernelGGL(tokenize_wave_kernel, dim3((unsigned)grid), dim3(64 * kTW), 0, T.st, T.c->tab,
                     T.d_text, T.n_bytes, T.d_sent_off, T.n_sent, T.max_pieces, T.d_ids, T.d_sent_len,
                     T.fb + kFbHead, reinterpret_cast<uint32_t*>(T.fb));
  return launch_lane(T, 0, T.n_sent, T.n_cu * 2, false);
}

}  // namespace lddl
