// Sentence -> WordPiece ids on the GPU.
//
// Replaces the per-sentence `tokenizer.tokenize(s, max_length=512, truncation=True)` call of
// lddl/dask/bert/pretrain.py:79-80 (HF BertTokenizerFast: added-token split on raw text,
// BertNormalizer, BertPreTokenizer, WordPiece; see oracle/lddl_oracle.c for the restated
// algorithm and tools/make_norm_tables.py for the per-code-point table).
//
// Output layout (no prefix sum needed): every code point normalises to at most as many chars
// as its UTF-8 bytes and every piece consumes >= 1 char, so a sentence never has more pieces than
// bytes; sentence s writes its pieces to ids[sent_off[s] ...] and its kept count (<= max_pieces)
// to sent_len[s] (bit 30 set if the kept pieces contain a literal [CLS]/[SEP]).
//
// Units (one kernel each, with the host function that launches it):
//   tokenize.hip       this file: tokenize_batch_kernel, the product path. Persistent workgroups
//                      of kBW waves (one per CU, sharing an LDS Bloom filter of the vocab); each
//                      wave streams its sentences (dynamic chunks) in 64-byte banks, one byte per
//                      lane. Lanes classify code points, ballots find the pre-tokenizer units,
//                      which go to an LDS queue spanning sentences; every kSF queued units are
//                      resolved in two phases (A: one vocab probe per unit, B: greedy
//                      longest-match WordPiece of the multi-piece / non-ASCII units only) and
//                      placed in queue order by a segmented scan (details below). A unit that does
//                      not fit (> kNorm normalised bytes, > kPcs pieces) sends its sentence to the
//                      fallback list. With it: the word memo, batch_pass, and the LDDL_STAMPS
//                      diagnostics (their host functions address this unit's __device__ globals).
//   tokenize_lane.hip  tokenize_lane_kernel: one lane per listed sentence, sequential (unbounded
//                      words, 100-char rule); also the whole-corpus path when
//                      LDDL_TOKENIZE_PATH=lane.
//   tokenize_wave.hip  tokenize_wave_kernel: round-1 design, one wavefront per sentence with no
//                      cross-sentence queue; kept only as the LDDL_TOKENIZE_PATH=wave diagnostic.
//   tokenize_api.hip   lddl_tokenize: argument checks, the knobs, the fallback list, the choice
//                      of path, the memo's table and its two passes. Launches no kernel itself.
//   tokenize_dev.h     device code of more than one unit: code-point table and UTF-8, words in
//                      registers (B32), vocab probes, wordpiece32, unit_word / norm_regs.
//   tokenize_plan.h    TokCall (one call's arguments) and the launchers' declarations.
//   tok_knobs.h        the LDDL_TOKENIZE_* knobs and the memo's sample size (host-only).
#include <algorithm>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "tokenize_dev.h"
#include "tokenize_plan.h"

namespace lddl {
namespace {

// ---------------------------------------------------------------------------------------------
// Streaming batched tokenizer (the product path).
//
// A wave claims chunks of kChunk consecutive sentences. Their text is one contiguous byte range
// [A, A + span), which the wave streams in 64-byte banks, one byte per lane, at fixed positions:
// a unit may span banks, so nothing is re-read. Sentence starts inside a bank are break bits
// (BRK); units never cross them. Per bank, ballots give two masks:
//   UNIT  bytes that belong to a pre-tokenizer unit (not a separator, inside the chunk)
//   CONT  bytes that continue the unit of the byte before: the same word run (no break between),
//         a continuation byte of an isolated char, the rest of a literal special token
// Unit starts are UNIT & ~CONT; unit ends are UNIT & ~(CONT >> 1), which needs the next bank's
// first CONT bit, so ends are enqueued one bank late. Starts (chunk-relative byte | kind | slow
// flag) and ends go to two LDS queues in byte order: the k-th start and the k-th end are unit k.
// Banks of plain ASCII (no byte >= 0x80, no control char, no '[', no special token carried in)
// take the short path: one LDS class lookup and three compares per lane. The others take the
// per-code-point classification (UTF-8 leads and continuations, literal specials, the Unicode
// class table) with carries into the next bank.
// Every kSF complete units are resolved in two phases:
//   A (one lane per unit, 64 at a time): literal specials, and one full-length vocab probe of
//     every ASCII word / punctuation unit. ~3/4 of the units are a single piece and are done.
//   B (one lane per unit, 64 at a time): greedy longest-match WordPiece of the remaining "hard"
//     units only (multi-piece words, non-ASCII), deferred across kSF units so that every lane of
//     a phase-B pass has a hard unit.
// Pieces are placed in queue order by a segmented scan over sentences (a unit's sentence by binary
// search of the chunk's sentence starts in LDS). At the end of a chunk the remaining units are
// resolved and every sentence's length (or its fallback) is written.
// Round 2's design re-started a 64-byte window at the last unit start of the window before and
// kept a ring of in-flight sentences; its per-window bookkeeping was ~half of the kernel's
// instructions (profiles/r03l_pmc_tokenizer_variants.txt).
// ---------------------------------------------------------------------------------------------
//
// Word memo (round 6; 19.27 -> 15.25 ms per 2 GB, profiles/r06l_*, r06m_*). Phase B (greedy
// longest match of the multi-piece and non-ASCII words) is
// ~half of the kernel's wave cycles, and its words repeat: in the synthetic corpus 26 % of the
// pre-tokenizer units are multi-piece, and 95 % of those occurrences are words already seen in
// the first 3 % of the text (Zipf). lddl_tokenize therefore runs the kernel twice per call: over
// a leading sample of the sentences (kMemoBuild: every resolved multi-piece word's pieces go to a
// device table, one slot per hash, the first writer claims it by CAS), then over the rest
// (kMemoLookup: a phase-B lane reads its word's slot — one 64-byte entry, normalised bytes as the
// key — and runs the greedy match only on a miss). The table belongs to the call: it is cleared
// before the sample pass, and the two launches order every write before every read, so an entry
// is always one complete (word, pieces) record. The pieces are a function of the normalised word
// alone, so the output is the same with or without the memo (tests run both).
// (WordMemo, kMemoOff / kMemoBuild / kMemoLookup and the table's size: tokenize_plan.h, for
// lddl_tokenize, which owns the table; the sample's size: memo_sample, tok_knobs.h.)
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kMemoReady = 1u << 31, kMemoClaim = 1u << 30;
__device__ inline B32 memo_key(const B32& v, int nb) {
  return B32{keep_bytes(v.w0, nb), keep_bytes(v.w1, nb - 8), keep_bytes(v.w2, nb - 16),
             keep_bytes(v.w3, nb - 24)};
}
__device__ inline uint32_t memo_slot(const B32& k, int nb) {
  uint64_t h = k.w0 * 0x9E3779B97F4A7C15ull ^ (uint64_t)nb;
  h = (h ^ (h >> 29) ^ k.w1) * 0xBF58476D1CE4E5B9ull;
  h = (h ^ (h >> 32) ^ k.w2) * 0x94D049BB133111EBull;
  h = (h ^ (h >> 29) ^ k.w3) * 0x9E3779B97F4A7C15ull;
  return (uint32_t)(h >> 32);
}

constexpr int kSF = 192;   // units resolved per pass (kSF / 64 phase-A rounds)
// queue capacity: before a bank < kSF complete units; a bank adds <= 64 ends and leaves <= 65
// units open (started, end not yet enqueued)
constexpr int kQ = kSF + 128;
constexpr int kBW = 16;   // waves per workgroup (one workgroup per CU shares the Bloom filter)
constexpr int kChunk = 128;  // consecutive sentences claimed at a time
static_assert((kChunk & (kChunk - 1)) == 0, "binary search over the chunk's sentences");
using HIdx = std::conditional_t<(kSF > 256), uint16_t, uint8_t>;
constexpr int32_t kHardBit = INT32_MIN;  // q_res: pieces are in column (res & 63) of pcs
// q_npc of a hard unit between phase A and its phase-B pass: phase A's note
constexpr uint32_t kRowMiss = 1u;   // probed at full length in phase A, not a single piece
constexpr uint32_t kRowValid = 2u;  // its word is in the unit's phase-B row (32 B at pcs byte 32 k)
// q_s entry: chunk-relative start byte (bits 0..27) | kind (28..30: 0 word / isolated char,
// 2 + k literal special k) | kQSlow (the unit holds a byte the register fast path cannot take)
constexpr int32_t kQPos = (1 << 28) - 1;
constexpr int32_t kQSlow = INT32_MIN;
constexpr int64_t kMaxSpan = 1 << 28;  // longer chunks go to the lane kernel
// r_cnt: pieces so far (bits 0..28) | kRFb (the sentence goes to the lane kernel) | kLenHasClsSep
constexpr int32_t kRFb = 1 << 29;
constexpr int32_t kRCnt = kRFb - 1;
static_assert(kLenHasClsSep == (1 << 30), "r_cnt flag layout");
// s_cls: fast-path byte classes
enum : uint32_t { kFRun = 0, kFSep = 1, kFIso = 2, kFSlow = 4 };

struct alignas(16) StreamLds {
  int32_t q_s[kQ];          // unit starts (see kQPos)
  int32_t q_e[kQ];          // unit ends (inclusive, chunk-relative)
  uint8_t q_slot[kQ];       // unit start's sentence slot in the chunk (from the bank loop)
  int32_t q_res[kSF];       // phase A/B result: the single piece id, or kHardBit | column
  uint8_t q_npc[kSF];       // pieces of the unit
  HIdx h_idx[kSF];          // queue positions of the hard units, in order
  int32_t s_off[kChunk + 1];  // chunk-relative sentence starts; s_off[n] = the chunk's length
  int32_t r_cnt[kChunk];    // see kRFb
  // lane l's pieces at pcs[64 q + l]; the same bytes hold lane l's normalised word (32 B at
  // byte 32 l) while phase B loads it into registers, before any piece is written
  alignas(16) int32_t pcs[kPcs * 64];
};
static_assert(kPcs * 64 * 4 >= 64 * kNorm, "normalised-word rows must fit the piece columns");

#ifdef LDDL_STAMPS
__device__ unsigned long long* g_tok_tl;  // diagnostic build: [wave][2] s_memrealtime start / end
// diagnostic build: shader cycles per region, summed over waves (kTokRegions entries)
__device__ unsigned long long* g_tok_reg;
// 0 banks, 1 phase A, 2 phase B (reported as the sum of its sub-regions), 3 place, 4 queue shift,
// 5 chunk; phase B's sub-regions: 6 B0 word fetch and normalise, 7 B1 memo load / compare /
// unpack, 8 B2 greedy match of the misses, 9 B3 the rest of the pass
constexpr int kTokRegions = 10;
constexpr int kTokDiag = kTokRegions + kTokCounters;  // one launch's slice of g_tok_reg
// the launches of one call report separately: slice 0 the memo-build (or only) launch, slice 1
// the memo-lookup launch
constexpr int kTokSlices = 2;
constexpr int kTokTlWgs = 1024;  // workgroups per slice of g_tok_tl (stamps_begin checks the grid)
#define TOK_STAMP(r)                                                     \
  do {                                                                   \
    const unsigned long long _now = __builtin_amdgcn_s_memtime();       \
    reg_acc[r] += _now - reg_last;                                       \
    reg_last = _now;                                                     \
  } while (0)
// a stamp inside phase B's block of the lanes that hold a word: the diagnostic build ends the
// block, stamps where the wave is whole again, and opens it anew; the product keeps one block
// (closing it after the memo lookup or after the greedy match costs 4 more spilled VGPRs,
// DESIGN §4)
#define TOK_STAMP_SPLIT(r) \
  }                        \
  }                        \
  TOK_STAMP(r);            \
  if (lane < hn) {         \
    if (uw.status == 0) {
#else
#define TOK_STAMP(r) \
  do {               \
  } while (0)
#define TOK_STAMP_SPLIT(r)
#endif

template <int kMemo>  // kMemoOff / kMemoBuild / kMemoLookup (word memo above)
__global__ void __launch_bounds__(64 * kBW, 1) tokenize_batch_kernel(
    Tables T_arg, const uint8_t* __restrict__ text, int64_t n_bytes, const int64_t* __restrict__ sent_off,
    int64_t n_sent, int32_t max_pieces, int32_t* __restrict__ ids, int32_t* __restrict__ sent_len_arg,
    int32_t* __restrict__ fb_list_arg, uint32_t* __restrict__ fb_n_arg, int32_t* __restrict__ chunk_ctr_arg,
    WordMemo M, int32_t slow_loop_arg) {
  __shared__ uint32_t s_ascii[128];
  __shared__ uint8_t s_cls[256];
  __shared__ uint32_t s_bloom[kBloomWords];
  __shared__ StreamLds s_w[kBW];
  // the tables' pointers and scalars live in LDS, read where used: as kernel arguments they held
  // ~26 SGPRs for the kernel's whole life and pushed the bank loop's own scalars into spills
  __shared__ Tables s_T;
  // (and the per-chunk / rare output pointers, for the same reason)
  __shared__ int32_t* s_cold[4];
  __shared__ int32_t s_slow_loop;  // LDDL_TOKENIZE_SLOW=loop: slow units take unit_word's loop
  if (threadIdx.x == 0) {
    s_T = T_arg;
    s_slow_loop = slow_loop_arg;
    s_cold[0] = sent_len_arg;
    s_cold[1] = fb_list_arg;
    s_cold[2] = reinterpret_cast<int32_t*>(fb_n_arg);
    s_cold[3] = chunk_ctr_arg;
  }
  __syncthreads();
  const Tables& T = s_T;
  int32_t* const volatile* cold = s_cold;  // read where used (not hoisted into registers)
#ifdef LDDL_STAMPS
  const unsigned long long rt0 = __builtin_amdgcn_s_memrealtime();
  unsigned long long reg_acc[kTokRegions] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long reg_last = __builtin_amdgcn_s_memtime();
  TokStats tstat;
  for (int q = 0; q < kTokCounters; ++q) tstat.c[q] = 0;
  TokStats* tsp = &tstat;
#else
  TokStats* tsp = nullptr;
#endif
  for (int c = threadIdx.x; c < 128; c += blockDim.x) s_ascii[c] = tab_entry(T, (uint32_t)c);
  for (int c = threadIdx.x; c < 256; c += blockDim.x) {
    uint32_t v = kFSlow;  // bytes >= 0x80, '[', and the ASCII chars the normaliser drops
    if (c < 128 && c != '[') {
      const uint32_t cl = tab_entry(T, (uint32_t)c) >> 30;
      v = cl == kSpace ? kFSep : cl == kIso ? kFIso : cl == kWord ? kFRun : kFSlow;
    }
    s_cls[c] = (uint8_t)v;
  }
  for (int c = threadIdx.x; c < kBloomWords; c += blockDim.x) s_bloom[c] = T.bloom[c];
  __syncthreads();
  const int lane = lane_id();
  StreamLds& W = s_w[threadIdx.x >> 6];
  // target of the bank loop's lanes that store nothing (no exec-mask branch): the piece columns,
  // unused outside a flush
  int32_t* const trashp = &W.pcs[lane_id()];
  // sentence indices fit int32 (lddl_tokenize: n_sent < INT32_MAX - 2^22)
  const int32_t n_sent32 = (int32_t)n_sent;
  // Chunks: wave w starts with chunk w, then takes the next unclaimed chunk from chunk_ctr
  // (initialised to the number of waves x kChunk). A static share per wave would leave a long
  // tail: waves of one SIMD are issued oldest first, so the first finishes ~25 % before the last.
  int32_t c0;
  {
    const int64_t w = (int64_t)blockIdx.x * kBW + (threadIdx.x >> 6);
    // (readfirstlane: the compiler cannot see that threadIdx.x >> 6 is wave-uniform, and a
    // divergent c0 made the chunk's span, sentence count and every loop over them exec-masked)
    c0 = __builtin_amdgcn_readfirstlane(w * kChunk < n_sent32 ? (int32_t)(w * kChunk) : n_sent32);
  }
  const uint64_t upto = (2ull << lane) - 1;  // lanes <= this one (lane 63: all)

  while (c0 < n_sent32) {
    const int32_t n = n_sent32 - c0 < kChunk ? n_sent32 - c0 : kChunk;
    const int64_t A = sent_off[c0];
    const int64_t span64 = sent_off[c0 + n] - A;
    if (span64 >= kMaxSpan) {  // pathological chunk (>= 256 MiB of text): the lane kernel
      for (int j = lane; j < n; j += 64)
        cold[1][atomicAdd(reinterpret_cast<uint32_t*>(cold[2]), 1u)] = c0 + j;
    } else {
      for (int j = lane; j <= n; j += 64) W.s_off[j] = (int32_t)(sent_off[c0 + j] - A);
      for (int j = lane; j < n; j += 64) W.r_cnt[j] = 0;
      wave_sync();
      const uint32_t span = (uint32_t)span64;
      const uint8_t* __restrict__ ctext = text + A;

      // the sentence holding chunk-relative byte st (the last one starting at or before it: empty
      // sentences at the same offset are skipped)
      auto sent_of = [&](int32_t st) -> int {
        int j = 0;
#pragma unroll
        for (int step = kChunk / 2; step >= 1; step >>= 1) {
          const int k = j + step;
          j = W.s_off[k < n ? k : n] <= st ? k : j;  // s_off[n] = span > st
        }
        return j;
      };

      int ns = 0, ne = 0;  // queued unit starts / ends

      // drop the processed units [0, m) from the queue: < 128 starts and < 128 ends remain
      // (read all, then write)
      auto drop = [&](int m) {
        const int rs = ns - m, re = ne - m;
        int32_t a0 = 0, a1 = 0, e0 = 0, e1 = 0;
        uint8_t l0 = 0, l1 = 0;
        if (lane < rs) a0 = W.q_s[m + lane], l0 = W.q_slot[m + lane];
        if (lane + 64 < rs) a1 = W.q_s[m + 64 + lane], l1 = W.q_slot[m + 64 + lane];
        if (lane < re) e0 = W.q_e[m + lane];
        if (lane + 64 < re) e1 = W.q_e[m + 64 + lane];
        wave_sync();
        if (lane < rs) W.q_s[lane] = a0, W.q_slot[lane] = l0;
        if (lane + 64 < rs) W.q_s[64 + lane] = a1, W.q_slot[64 + lane] = l1;
        if (lane < re) W.q_e[lane] = e0;
        if (lane + 64 < re) W.q_e[64 + lane] = e1;
        wave_sync();
        ns = rs;
        ne = re;
      };

      // place queue units [u0, u1) (all resolved) in order: segmented scan per sentence
      auto place = [&](int u0, int u1) {
        for (int r0 = u0; r0 < u1; r0 += 64) {
          const int u = r0 + lane;
          const bool act = u < u1;
          const int uc = act ? u : u0;
          const int32_t qs = W.q_s[uc];
          const int npc = act ? W.q_npc[uc] : 0;
          const int slot = act ? (int)W.q_slot[uc] : -1;
          const int incl = wave_incl_scan(npc);
          const int excl = incl - npc;
          const int prev_slot = wave_prev(slot);
          const uint64_t F = ballot(act && (lane == 0 || slot != prev_slot));
          const int s0 = 63 - __clzll(F & upto);
          const int seg_excl = excl - __shfl(excl, s0, 64);
          const int next_slot = wave_next(slot);
          const bool seg_last = act && (lane == 63 || u + 1 >= u1 || next_slot != slot);
          if (act) {
            const int o = (W.r_cnt[slot] & kRCnt) + seg_excl;
            const int64_t bb = A + W.s_off[slot];
            const int32_t res = W.q_res[u];
            if (res & kHardBit) {
              const int col = res & 63;
              for (int q = 0; q < npc; ++q)
                if (o + q < max_pieces) ids[bb + o + q] = W.pcs[64 * q + col];
            } else if (npc && o < max_pieces) {
              ids[bb + o] = res;
              const int kind = (qs >> 28) & 7;
              if (kind - 2 == kCls || kind - 2 == kSep) atomicOr(&W.r_cnt[slot], kLenHasClsSep);
            }
          }
          wave_sync();
          if (seg_last) W.r_cnt[slot] += seg_excl + npc;  // (count bits only: < 2^28 pieces)
          wave_sync();
        }
      };

      // resolve and place the complete units [0, m), then drop them from the queue
      auto flush = [&](int m) {
        TOK_STAMP(0);
        // phase A: specials and single-piece words
        int nh = 0;
        {  // all rounds' text loads, then all first table loads, then the checks: one latency each
          constexpr int kR = kSF / 64;
          static_assert(kSF % 64 == 0, "phase A rounds");
          bool elig[kR], hardr[kR];
          int lenr[kR];
          int32_t resr[kR];
          B32 vv[kR];
          Probe pr[kR];
#pragma unroll
          for (int r = 0; r < kR; ++r) {
            const int u = 64 * r + lane;
            elig[r] = hardr[r] = false;
            lenr[r] = 0;
            resr[r] = 0;
            if (u < m) {
              const int32_t qs = W.q_s[u];
              const int st = qs & kQPos, kind = (qs >> 28) & 7;
              const int len = W.q_e[u] - st + 1;
              lenr[r] = len;
              if (kind >= 2) {
                resr[r] = T.special_id[kind - 2];
              } else if (qs >= 0 && T.ascii_mode != 0 && len <= T.max_piece_bytes && len <= 32) {
                elig[r] = true;
                vv[r] = load32(text, n_bytes, A + st);
              } else {
                hardr[r] = true;
              }
            }
          }
#pragma unroll
          for (int r = 0; r < kR; ++r)
            if (elig[r]) {
              if (T.ascii_mode == 1)
                vv[r] = B32{swar_lower(vv[r].w0), swar_lower(vv[r].w1), swar_lower(vv[r].w2), swar_lower(vv[r].w3)};
              pr[r] = probe_first(T, vv[r], lenr[r], 0);
            }
#pragma unroll
          for (int r = 0; r < kR; ++r) {
            if (elig[r]) {
              resr[r] = probe_finish(T, vv[r], lenr[r], pr[r]);
              hardr[r] = resr[r] < 0;
            }
            const int u = 64 * r + lane;
            if (u < m && !hardr[r]) {
              W.q_res[u] = resr[r];
              W.q_npc[u] = 1;
            }
            const uint64_t H = ballot(hardr[r]);
            if (hardr[r]) {
              const int k = nh + (int)popc_below(H);
              W.h_idx[k] = (HIdx)u;
              // phase B learns from q_npc[u] (its own until phase B writes the piece count) what
              // phase A did with the unit, and so whether row k holds a word
              W.q_npc[u] = (uint8_t)(!elig[r] ? 0u : k < 64 ? kRowMiss | kRowValid : kRowMiss);
              // a probed word that missed: its (lowercased) bytes go to phase-B row k, so the
              // first phase-B pass reads them from LDS instead of loading the text again
              if (elig[r] && k < 64) {
                uint4* row = reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(W.pcs) + 32 * k);
                row[0] = make_uint4((uint32_t)vv[r].w0, (uint32_t)(vv[r].w0 >> 32), (uint32_t)vv[r].w1,
                                    (uint32_t)(vv[r].w1 >> 32));
                row[1] = make_uint4((uint32_t)vv[r].w2, (uint32_t)(vv[r].w2 >> 32), (uint32_t)vv[r].w3,
                                    (uint32_t)(vv[r].w3 >> 32));
              }
            }
            nh += __popcll(H);
          }
        }
        wave_sync();
        TOK_STAMP(1);
        // phase B in chunks of 64 hard units, each chunk placed with the units before the next one
        int placed = 0;
        if (tsp) {
          tsp->wave(8);
          tsp->add(9, lane == 0 ? m : 0);
        }
        for (int h0 = 0; h0 < nh; h0 += 64) {
          const int hn = nh - h0 < 64 ? nh - h0 : 64;
          if (tsp) {
            tsp->wave(0);
            tsp->add(1, lane < hn);
          }
          int u = -1, st = 0;
          UnitWord uw;
          uw.status = 1;
          bool known_miss = false;
          if (lane < hn) {
            u = W.h_idx[h0 + lane];
            const int32_t qs = W.q_s[u];
            st = qs & kQPos;
            const int len = W.q_e[u] - st + 1;
            const bool slow = qs < 0;
            // phase A's note for this unit (kRowMiss: it probed the whole word and missed;
            // kRowValid: it also left the word in row h0 + lane)
            const uint32_t note = W.q_npc[u];
            known_miss = (note & kRowMiss) != 0;
            if (tsp) {
              tsp->add(10, slow);
              if (ballot(slow)) tsp->wave(11);
            }
            if (note & kRowValid) {
              const uint4* row = reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(W.pcs) + 32 * lane);
              const uint4 r0 = row[0], r1 = row[1];
              uw.v = B32{r0.x | (uint64_t)r0.y << 32, r0.z | (uint64_t)r0.w << 32,
                         r1.x | (uint64_t)r1.y << 32, r1.z | (uint64_t)r1.w << 32};
              uw.nb = len;
              uw.ends = ~0ull;
              uw.status = 0;
            } else {
              uw = unit_word(T, s_ascii, text, n_bytes, A + st, len, slow,
                             reinterpret_cast<uint8_t*>(W.pcs) + 32 * lane, !s_slow_loop);
            }
          }
          wave_sync();  // every normalised word is in registers: the rows become piece columns
          TOK_STAMP(6);
          int npc = 0;
          bool hit = false;
          Pcs pc{W.pcs + lane};
          if (lane < hn) {
            if (uw.status == 0) {
              if constexpr (kMemo != kMemoOff) {
                // the memo key is the word with its bytes past nb cleared (don't-care bytes to
                // every later use, so the word's own registers hold it)
                uw.v = memo_key(uw.v, uw.nb);
              }
              if constexpr (kMemo == kMemoLookup) {
                const B32& key = uw.v;
                const uint4* e = M.tab + 4 * (size_t)(memo_slot(key, uw.nb) & M.mask);
                const uint4 k0 = e[0], k1 = e[1], pz = e[2];
                const uint32_t meta = e[3].x;
                hit = (meta & kMemoReady) && (int)(meta & 0xFFu) == uw.nb &&
                      (((k0.x | (uint64_t)k0.y << 32) ^ key.w0) | ((k0.z | (uint64_t)k0.w << 32) ^ key.w1) |
                       ((k1.x | (uint64_t)k1.y << 32) ^ key.w2) | ((k1.z | (uint64_t)k1.w << 32) ^ key.w3)) == 0;
                if (hit) {
                  npc = (int)((meta >> 8) & 0xFu);
                  const uint32_t pw[4] = {pz.x, pz.y, pz.z, pz.w};
#pragma unroll
                  for (int q = 0; q < kPcs; ++q)
                    if (q < npc) pc.put(q, (int32_t)((pw[q >> 1] >> (16 * (q & 1))) & 0xFFFFu));
                }
              }
              TOK_STAMP_SPLIT(7);
              if (!hit) npc = wordpiece32(T, s_bloom, uw.v, uw.nb, uw.ends, pc, known_miss, tsp);
              TOK_STAMP_SPLIT(8);
              if constexpr (kMemo == kMemoBuild) {
                // first writer of the slot in this call claims it; no lane of this launch reads
                const B32& key = uw.v;
                uint4* e = M.tab + 4 * (size_t)(memo_slot(key, uw.nb) & M.mask);
                if (npc >= 1 && atomicCAS(&e[3].x, 0u, kMemoClaim) == 0u) {
                  uint32_t pw[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                  for (int q = 0; q < kPcs; ++q)
                    if (q < npc) pw[q >> 1] |= ((uint32_t)pc.get(q) & 0xFFFFu) << (16 * (q & 1));
                  e[0] = make_uint4((uint32_t)key.w0, (uint32_t)(key.w0 >> 32), (uint32_t)key.w1,
                                    (uint32_t)(key.w1 >> 32));
                  e[1] = make_uint4((uint32_t)key.w2, (uint32_t)(key.w2 >> 32), (uint32_t)key.w3,
                                    (uint32_t)(key.w3 >> 32));
                  e[2] = make_uint4(pw[0], pw[1], pw[2], pw[3]);
                  e[3].x = kMemoReady | (uint32_t)uw.nb | (uint32_t)npc << 8;
                }
              }
            } else if (uw.status < 0) {
              npc = -1;
            }
            if (npc < 0) {  // the sentence goes to the lane kernel
              atomicOr(&W.r_cnt[sent_of(st)], kRFb);
              npc = 0;
            }
            W.q_res[u] = kHardBit | lane;
            W.q_npc[u] = (uint8_t)npc;
          }
          wave_sync();
          const int lim = h0 + 64 < nh ? (int)W.h_idx[h0 + 64] : m;
          TOK_STAMP(9);
          place(placed, lim);
          placed = lim;
          TOK_STAMP(3);
        }
        place(placed, m);
        TOK_STAMP(3);
        drop(m);
        TOK_STAMP(4);
      };

      // ---- the chunk's banks ----
      uint64_t UNITp = 0, CONTp = 0;  // the bank before
      uint64_t cin = 0;               // the byte before the bank is a word-run byte
      // slow-path carries into the next bank: code-point coverage of its first lanes (bit k: lane
      // k continues a lead of the bank before, for leads of 2 / 3 / 4 bytes; <= 3 bits each) and
      // special-token bytes (<= 5 bits), packed k1 | k2 << 8 | k3 << 16 | insc << 24 so that the
      // plain-bank test reads one scalar (as four 64-bit masks they were spilled and reloaded
      // every bank); and the (class | cplen << 4) of the bank's lanes 61..63, one byte each
      uint32_t cpack = 0, plcp = 0;
      int32_t jn = 1;  // the next sentence start to mark
      uint32_t nextS = (uint32_t)__builtin_amdgcn_readfirstlane(W.s_off[1]);
      const uint32_t last = span ? span - 1 : 0;
      // software prefetch three banks ahead (clamped into the chunk; bytes past it are unused)
      uint32_t cur = 0x20u, pf1 = 0x20u, pf2 = 0x20u;
      if (span) {
        cur = ctext[(uint32_t)lane < last ? (uint32_t)lane : last];
        pf1 = ctext[64u + lane < last ? 64u + lane : last];
        pf2 = ctext[128u + lane < last ? 128u + lane : last];
      }
      uint32_t x0 = 0;
      for (; x0 < span; x0 += 64) {
        const uint32_t byte = cur;
        const uint32_t v = s_cls[byte];
        cur = pf1;
        pf1 = pf2;
        {
          const uint32_t xq = x0 + 192u + lane;
          pf2 = ctext[xq < last ? xq : last];
        }
        const uint32_t x = x0 + lane;
        const bool in = x < span;
        uint64_t BRK = 0;
        // this lane's sentence slot (the last sentence starting at or before byte x, as sent_of),
        // stored with its unit start so that placement needs no search
        int32_t lslot = jn - 1;
        while (nextS < x0 + 64) {
          BRK |= 1ull << (nextS - x0);
          lslot += (x0 + lane >= nextS) ? 1 : 0;
          ++jn;
          nextS = jn <= n ? (uint32_t)__builtin_amdgcn_readfirstlane(W.s_off[jn]) : 0xFFFFFFFFu;
        }
        const uint64_t VALID = ballot(in);
        uint64_t RUN, UNIT, CONT, SL = 0;
        // unit start: chunk-relative byte | kind << 28
        int32_t sval = (int32_t)x;
        if (!(ballot(v >= kFSlow) | (uint64_t)cpack)) {  // plain ASCII bank
          RUN = ballot(v == kFRun) & VALID;
          UNIT = VALID & ~ballot(v == kFSep);
          CONT = RUN & ((RUN << 1) | cin) & ~BRK;
        } else {
          const uint64_t k1 = cpack & 0xFFu, k2 = (cpack >> 8) & 0xFFu, k3 = (cpack >> 16) & 0xFFu,
                         insc = cpack >> 24;
          // this lane's sentence end: the next break above the lane, else the first sentence start
          // after the bank
          const uint64_t above = BRK & ~upto;
          const uint32_t se = above ? x0 + (uint32_t)(__ffsll((long long)above) - 1)
                                    : (nextS < span ? nextS : span);
          const int64_t i = A + x, b1 = A + se;
          uint32_t cls = in ? s_ascii[byte & 127u] >> 30 : kSpace;
          int cplen = 1;  // bytes of the code point starting here (0: covered continuation)
          int spk = -1;   // literal special token starting here
          bool slow = in && cls == kDrop;
          bool cont = false;
          if (ballot(in && byte >= 0x80)) {
            if (in && byte >= 0xC0) {
              int64_t j = i;
              const uint32_t cp = utf8_next(text, b1, j);
              cplen = (int)(j - i);
              cls = tab_entry(T, cp) >> 30;
              slow = true;
            } else if (in && byte >= 0x80) {
              cont = true;  // covered by a valid lead, or a lone byte (U+FFFD, dropped)
              cls = kDrop;
              slow = true;
            }
          }
          if (ballot(in && byte == '[')) {
            if (in && byte == '[') spk = match_special_at(T, text, i, b1);
          }
          const int32_t val = (int32_t)(cls | ((uint32_t)cplen << 4));
          const uint64_t V2 = ballot(cplen == 2), V3 = ballot(cplen == 3), V4 = ballot(cplen == 4);
          const uint64_t C1 = ((V2 | V3 | V4) << 1) | k1, C2 = ((V3 | V4) << 2) | k2, C3 = (V4 << 3) | k3;
          if (C1 | C2 | C3) {  // code points of more than one byte (wave-uniform branch)
            const bool covered = cont && (((C1 | C2 | C3) >> lane) & 1ull);
            const int dist = !covered ? 0 : ((C1 >> lane) & 1ull) ? 1 : ((C2 >> lane) & 1ull) ? 2 : 3;
            int lead = __shfl(val, lane - dist, 64);
            if (lane < dist)
              lead = (int)((plcp >> (lane - dist == -1 ? 16 : lane - dist == -2 ? 8 : 0)) & 0xFFu);
            if (covered) {  // a covered continuation takes its lead's class
              cls = (uint32_t)lead & 3u;
              cplen = 0;
            }
          }
          const uint64_t S = ballot(spk >= 0), S6 = ballot(spk == kMask);
          const uint64_t inside = (S << 1) | (S << 2) | (S << 3) | (S << 4) | (S6 << 5) | insc;
          const bool in_sp = ((S | inside) >> lane) & 1ull;
          const uint32_t cat = in_sp ? kCatSpecial : cls == kSpace ? kCatSep : cls == kIso ? kCatIso : kCatRun;
          RUN = ballot(cat == kCatRun);
          const uint64_t ISO = ballot(cat == kCatIso), LEAD = ballot(cplen > 0);
          UNIT = ballot(cat != kCatSep);
          CONT = (RUN & ((RUN << 1) | cin) & ~BRK) | (ISO & ~LEAD) | inside;
          sval = (int32_t)(x | ((uint32_t)(spk >= 0 ? 2 + spk : 0) << 28));
          SL = ballot(slow && cat != kCatSep);
          cpack = (uint32_t)((V2 | V3 | V4) >> 63) | (uint32_t)((V3 | V4) >> 62) << 8 |
                  (uint32_t)(V4 >> 61) << 16 |
                  (uint32_t)((S >> 63) | (S >> 62) | (S >> 61) | (S >> 60) | (S6 >> 59)) << 24;
          plcp = (uint32_t)__builtin_amdgcn_readlane(val, 61) | (uint32_t)__builtin_amdgcn_readlane(val, 62) << 8 |
                 (uint32_t)__builtin_amdgcn_readlane(val, 63) << 16;
        }
        // starts of this bank (lanes without one store to their trash slot)
        const uint64_t US = UNIT & ~CONT;
        {
          const uint32_t r = popc_below(US) + (uint32_t)ns;
          const bool st_here = (US >> lane) & 1ull;
          int32_t* dst = st_here ? &W.q_s[r] : trashp;
          *dst = sval;
          // the unit's sentence slot (placement needs no search)
          uint8_t* sd = st_here ? &W.q_slot[r] : reinterpret_cast<uint8_t*>(trashp);
          *sd = (uint8_t)lslot;
        }
        if (SL) {  // slow bytes flag their unit (started in this bank or before)
          if ((SL >> lane) & 1ull) atomicOr(&W.q_s[ns + (int)__popcll(US & upto) - 1], kQSlow);
        }
        ns += (int)__popcll(US);
        // ends of the bank before
        const uint64_t UEp = UNITp & ~((CONTp >> 1) | (CONT << 63));
        {
          const uint32_t r = popc_below(UEp) + (uint32_t)ne;
          int32_t* dst = ((UEp >> lane) & 1ull) ? &W.q_e[r] : trashp;
          *dst = (int32_t)(x - 64u);
        }
        ne += (int)__popcll(UEp);
        cin = RUN >> 63;
        UNITp = UNIT;
        CONTp = CONT;
        if (ne >= kSF) {
          wave_sync();
          flush(kSF);
        }
      }
      {  // the last bank's ends (nothing continues past the chunk)
        const uint64_t UEp = UNITp & ~(CONTp >> 1);
        const uint32_t r = popc_below(UEp) + (uint32_t)ne;
        int32_t* dst = ((UEp >> lane) & 1ull) ? &W.q_e[r] : trashp;
        *dst = (int32_t)(x0 - 64u + lane);
        ne += (int)__popcll(UEp);
      }
      wave_sync();
      TOK_STAMP(0);
      while (ne > 0) flush(ne < kSF ? ne : kSF);
      // the chunk's sentences
      for (int j = lane; j < n; j += 64) {
        const int32_t rc = W.r_cnt[j];
        if (rc & kRFb) {
          cold[1][atomicAdd(reinterpret_cast<uint32_t*>(cold[2]), 1u)] = c0 + j;
        } else {
          const int32_t cnt = rc & kRCnt;
          cold[0][c0 + j] = (cnt < max_pieces ? cnt : max_pieces) | (rc & kLenHasClsSep);
        }
      }
      wave_sync();  // before the next chunk reuses s_off / r_cnt
    }
    TOK_STAMP(5);
    int32_t nc = 0;
    if (lane == 0) nc = atomicAdd(cold[3], kChunk);
    nc = __builtin_amdgcn_readfirstlane(nc);
    c0 = nc < n_sent32 ? nc : n_sent32;
  }
#ifdef LDDL_STAMPS
  constexpr int slice = kMemo == kMemoLookup ? 1 : 0;
  if (lane == 0 && g_tok_tl) {
    const int64_t wv = ((int64_t)slice * kTokTlWgs + blockIdx.x) * kBW + (threadIdx.x >> 6);
    g_tok_tl[2 * wv] = rt0;
    g_tok_tl[2 * wv + 1] = __builtin_amdgcn_s_memrealtime();
  }
  unsigned long long* const reg = g_tok_reg ? g_tok_reg + slice * kTokDiag : nullptr;
  if (lane == 0 && reg)
    for (int r = 0; r < kTokRegions; ++r) atomicAdd(reg + r, reg_acc[r]);
  if (reg)
    for (int q = 0; q < kTokCounters; ++q) {
      const uint64_t v = wave_sum(tstat.c[q]);
      if (lane == 0) atomicAdd(reg + kTokRegions + q, (unsigned long long)v);
    }
#endif
}

}  // namespace

int batch_grid_max(const TokCall& T, int64_t* grid_max) {
  int per_cu = 0;
  LDDL_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, tokenize_batch_kernel<kMemoOff>, 64 * kBW, 0));
  *grid_max = T.n_cu * std::max(per_cu, 1);
  return 0;
}

// One launch of the streaming kernel over sentences [s0, s0 + n) (the sentence offsets are
// absolute, so a sub-range is a pointer offset), then the lane kernel for its fallback list.
// grid_max: the resident workgroups (grid-stride over sentences with exactly those: a second
// wave of workgroups would start only when the first finished, a 2x tail).
int batch_pass(TokCall& T, int64_t grid_max, int64_t s0, int64_t n, int memo, WordMemo M) {
  const int64_t want = (n + 16 * kBW - 1) / (16 * kBW);
  // (LDDL_TOKENIZE_GRID, tests: a smaller grid makes small inputs take the dynamic chunk claims)
  const int64_t grid = std::max<int64_t>(1, std::min({want, grid_max, T.knobs.grid_cap}));
  T.grid_of[memo == kMemoLookup ? 1 : 0] = grid;
  // the first grid x kBW chunks are taken statically (chunk w by wave w)
  const int64_t first = std::min<int64_t>(grid * kBW * kChunk, (int64_t)INT32_MAX);
  LDDL_HIP(hipMemsetAsync(T.fb, 0, sizeof(int32_t) * kFbHead, T.st));
  LDDL_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(T.chunk_ctr), (int)first, 1, T.st));
  const void* kfn = memo == kMemoBuild ? (const void*)tokenize_batch_kernel<kMemoBuild>
                  : memo == kMemoLookup ? (const void*)tokenize_batch_kernel<kMemoLookup>
                                        : (const void*)tokenize_batch_kernel<kMemoOff>;
  const int64_t* so = T.d_sent_off + s0;
  int32_t* sl = T.d_sent_len + s0;
  int32_t* fl = T.fb + kFbHead;
  uint32_t* fn = reinterpret_cast<uint32_t*>(T.fb);
  void* args[] = {&T.c->tab, (void*)&T.d_text, &T.n_bytes, (void*)&so, &n, &T.max_pieces, &T.d_ids, &sl,
                  &fl, &fn, &T.chunk_ctr, &M, &T.knobs.slow_loop};
  LDDL_HIP(hipLaunchKernel(kfn, dim3((unsigned)grid), dim3(64 * kBW), args, 0, T.st));
  return launch_lane(T, s0, n, T.n_cu * 2, false);
}

#ifdef LDDL_STAMPS
// diagnostic build: the streaming kernel's wave timelines (tl) and region counters (rg), one
// slice per launch of the call
int stamps_begin(ArenaScope& diag, const TokCall& T, int64_t grid_max, unsigned long long** tl,
                 unsigned long long** rg) {
  if (grid_max > kTokTlWgs) LDDL_FAIL(-1, "diagnostic build: %lld workgroups exceed kTokTlWgs", (long long)grid_max);
  const size_t n_tl = (size_t)2 * kTokSlices * kTokTlWgs * kBW, n_rg = (size_t)kTokSlices * kTokDiag;
  int rc;
  if ((rc = diag.take(tl, n_tl)) || (rc = diag.take(rg, n_rg))) return rc;
  LDDL_HIP(hipMemsetAsync(*tl, 0, 8 * n_tl, T.st));
  LDDL_HIP(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_tok_tl), tl, sizeof(*tl), 0, hipMemcpyHostToDevice, T.st));
  LDDL_HIP(hipMemsetAsync(*rg, 0, 8 * n_rg, T.st));
  LDDL_HIP(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_tok_reg), rg, sizeof(*rg), 0, hipMemcpyHostToDevice, T.st));
  return 0;
}

// one launch's slice: `label` names it in every line
static int report_tok_slice(const TokCall& T, const char* label, int64_t grid, const unsigned long long* tl,
                            const unsigned long long* rg) {
  // wave timeline (100 MHz real-time clock)
  const int64_t nw = grid * kBW;
  std::vector<unsigned long long> t(2 * nw);
  LDDL_HIP(hipMemcpyAsync(t.data(), tl, 16 * nw, hipMemcpyDeviceToHost, T.st));
  LDDL_HIP(hipStreamSynchronize(T.st));
  unsigned long long t0 = ~0ull, t1 = 0;
  std::vector<double> e(nw);
  for (int64_t q = 0; q < nw; ++q) {
    t0 = std::min(t0, t[2 * q]);
    t1 = std::max(t1, t[2 * q + 1]);
  }
  for (int64_t q = 0; q < nw; ++q) e[q] = (t[2 * q + 1] - t0) / 1e5;
  std::sort(e.begin(), e.end());
  const double span = (t1 - t0) / 1e5;
  fprintf(stderr, "[tok %s timeline] span %.2f ms, wave end ms: min %.2f p10 %.2f p50 %.2f p90 %.2f max %.2f\n",
          label, span, e[0], e[nw / 10], e[nw / 2], e[nw * 9 / 10], e[nw - 1]);
  const int nb = 40;
  fprintf(stderr, "[tok %s timeline] waves alive per %.2f ms bin:", label, span / nb);
  for (int b = 0; b < nb; ++b) {
    const double te = span * (b + 0.5) / nb;
    int64_t alive = 0;
    for (int64_t q = 0; q < nw; ++q) alive += e[q] > te;
    fprintf(stderr, " %lld", (long long)alive);
  }
  fprintf(stderr, "\n");
  unsigned long long r[kTokDiag];
  LDDL_HIP(hipMemcpy(r, rg, sizeof r, hipMemcpyDeviceToHost));
  const unsigned long long* k = r + kTokRegions;
  fprintf(stderr,
          "[tok %s phaseB] flushes %llu units %llu | passes %llu lanes/pass %.1f | piece-steps: wave %llu "
          "lane %llu (lane util %.2f) | bloom iters: wave %llu lane-useful %llu (util %.2f, per wave "
          "step %.1f) | probe trips: wave %llu lane %llu (util %.2f) | slow lanes %llu (%.2f per pass), "
          "passes with one %llu (%.1f%%)\n",
          label, k[8], k[9], k[0], (double)k[1] / (k[0] ? k[0] : 1), k[2], k[3],
          (double)k[3] / (64.0 * (k[2] ? k[2] : 1)), k[4], k[5], (double)k[5] / (64.0 * (k[4] ? k[4] : 1)),
          (double)k[4] / (k[2] ? k[2] : 1), k[6], k[7], (double)k[7] / (64.0 * (k[6] ? k[6] : 1)), k[10],
          (double)k[10] / (k[0] ? k[0] : 1), k[11], 100.0 * k[11] / (k[0] ? k[0] : 1));
  r[2] = r[6] + r[7] + r[8] + r[9];
  unsigned long long tot = 0;
  for (int q = 0; q < 6; ++q) tot += r[q];
  static const char* names[kTokRegions] = {"banks", "phaseA", "phaseB", "place", "qshift", "chunk",
                                           "B0 fetch+normalise", "B1 memo", "B2 greedy", "B3 rest"};
  fprintf(stderr, "[tok %s regions] wave-cycle shares:", label);
  for (int q = 0; q < 6; ++q) fprintf(stderr, " %s %.1f%%", names[q], 100.0 * r[q] / (tot ? tot : 1));
  fprintf(stderr, "\n[tok %s phaseB split] share of phase B (of the kernel):", label);
  for (int q = 6; q < kTokRegions; ++q)
    fprintf(stderr, " %s %.1f%% (%.1f%%)", names[q], 100.0 * r[q] / (r[2] ? r[2] : 1), 100.0 * r[q] / (tot ? tot : 1));
  fprintf(stderr, " | phase-B wave cycles per pass %.0f\n", (double)r[2] / (k[0] ? k[0] : 1));
  return 0;
}

int report_tok_stamps(const TokCall& T, const unsigned long long* tl, const unsigned long long* rg) {
  static const char* labels[2][kTokSlices] = {{"single", ""}, {"build", "lookup"}};
  const bool two = T.grid_of[1] > 0;
  for (int s = 0; s < kTokSlices; ++s) {
    if (!T.grid_of[s]) continue;
    int rc = report_tok_slice(T, labels[two][s], T.grid_of[s], tl + (size_t)2 * s * kTokTlWgs * kBW,
                              rg + (size_t)s * kTokDiag);
    if (rc) return rc;
  }
  return 0;
}
#endif

}  // namespace lddl
