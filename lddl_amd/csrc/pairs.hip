// NSP pair construction + static MLM masking on the GPU.
//
// Reference: lddl/dask/bert/pretrain.py
//   _get_documents filtering       89-97   -> compact_* kernels (drop empty sentences / documents)
//   _to_partition_pairs           386-402  -> plan kernel (one wave per partition) + final shuffle
//   create_pairs_from_document    241-365  -> plan_document()
//   _truncate_seq_pair            161-176  -> truncation loop in plan_document()
//   create_masked_lm_predictions  182-238  -> mask decisions in plan_document(), applied by gather
//
// Split into a control plane that touches only integers (sentence lengths, RNG draws) and a data
// plane that moves tokens:
//   plan    one wave per partition. Replay mode reproduces CPython's `random` exactly
//           (random.seed(part_seed[p]) then the reference's draw sequence): the wave executes the
//           sequential algorithm wave-uniformly (every lane computes the same scalars, so control
//           flow never diverges), keeps the MT19937 state in LDS and regenerates it with a
//           64-lane cooperative twist. Output: 32-byte pair descriptors (sentence span + truncation
//           window of A and B) and, with masking, the chosen positions + replacement ids.
//   layout  scans of per-partition pair counts and per-pair token / mask counts (final order =
//           the partition shuffle of pretrain.py:401).
//   gather  one wave per pair: coalesced copy of A and B token spans from the tokenizer output,
//           applying the mask decisions and emitting positions + labels.
#include <algorithm>
#include <cstdio>
#include <memory>
#include <vector>

#include <cstdlib>
#include <cstring>

#include "collate_dev.h"  // ContBits, cont_id
#include "common.h"
#include "ctx.h"
#include "device.h"
#include "lddl_amd.h"
#include "plan_split.h"
#include "scan.h"

namespace lddl {
namespace {

struct alignas(16) PairDesc {
  int64_t a_ks;     // kept-sentence index where A's chunk starts
  int64_t b_ks;     // kept-sentence index where B's span starts
  int32_t a_front;  // tokens truncated from the front of A's concatenated sentences
  int32_t na;       // tokens kept in A
  int32_t b_front;
  int32_t nb_rn;    // tokens kept in B | is_random_next << 31
};

// Replay masking, per planner slot: where the pair's decisions (mask pool, entries moff8 * 8 ..)
// and shuffle draws (draw pool, joff16 * 16 ..) are, and how many. One 16-byte record, one store.
struct alignas(16) SlotPool {
  uint32_t moff8;   // mask-pool offset / 8 (regions are 8-entry aligned)
  uint32_t joff16;  // draw-pool offset / 16 (regions are 16-entry aligned)
  int32_t nmask;    // num_to_predict
  int32_t ncand;    // candidates (len(A) + len(B) minus literal [CLS]/[SEP])
};

constexpr int32_t kKeep = -1;  // mask decision "keep the original token" (pretrain.py:215-216)

// Diagnostic build only (-DLDDL_STAMPS): per-region s_memtime sums of the planner.
#ifdef LDDL_STAMPS
constexpr int kStampRegions = 8;
#define STAMP_T() __builtin_amdgcn_s_memtime()
#define STAMP_ADD(r, t0)                   \
  do {                                     \
    const uint64_t t1_ = STAMP_T();        \
    st_acc[r] += t1_ - (t0);               \
    t0 = t1_;                              \
  } while (0)
#else
#define STAMP_T() 0ull
#define STAMP_ADD(r, t0) ((void)0)
#endif

// ---------------------------------------------------------------------------------------------
// Compaction (pretrain.py:89-97): drop sentences with no pieces, then documents with no sentences
// ---------------------------------------------------------------------------------------------
struct KeepSent {
  const int32_t* len;
  __device__ int64_t operator()(int64_t s) const { return (len[s] & kLenMask) > 0; }
};
// both sentence scans in one pass: kept-sentence index and token offset. A dropped sentence has
// no tokens, so the token scan over all sentences, read at the kept ones, is the kept-token scan.
struct SentCounts {
  const int32_t* len;
  __device__ Sum2 operator()(int64_t s) const {
    const int32_t l = len[s] & kLenMask;
    return Sum2{l > 0 ? 1 : 0, l};
  }
};
struct KeepDoc {
  const int64_t* ks_pos;  // exclusive scan of KeepSent, n_sent+1
  const int64_t* doc_sent_off;
  __device__ int64_t operator()(int64_t d) const {
    return ks_pos[doc_sent_off[d + 1]] > ks_pos[doc_sent_off[d]];
  }
};

// kept sentence k = ks_pos[s]: its text start, length and token offset kscan[k] = tok_pos[s]
// (kscan[n_kept] = the total, from thread n_sent)
__global__ void scatter_sentences_kernel(const int64_t* sent_off, const int32_t* sent_len,
                                         int64_t n_sent, const int64_t* ks_pos, const int64_t* tok_pos,
                                         int64_t* ks_start, int32_t* ks_len, int64_t* kscan) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s > n_sent) return;
  if (s == n_sent) {
    kscan[ks_pos[n_sent]] = tok_pos[n_sent];
    return;
  }
  const int32_t l = sent_len[s];
  if ((l & kLenMask) == 0) return;
  const int64_t k = ks_pos[s];
  ks_start[k] = sent_off[s];
  ks_len[k] = l;
  kscan[k] = tok_pos[s];
}

__global__ void scatter_docs_kernel(const int64_t* doc_sent_off, int64_t n_doc, const int64_t* ks_pos,
                                    const int64_t* kd_pos, int64_t* kd_off) {
  const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d > n_doc) return;
  if (d == n_doc) { kd_off[kd_pos[n_doc]] = ks_pos[doc_sent_off[n_doc]]; return; }
  if (kd_pos[d + 1] > kd_pos[d]) kd_off[kd_pos[d]] = ks_pos[doc_sent_off[d]];
}

__global__ void part_offsets_kernel(const int64_t* part_doc_off, int64_t n_part, const int64_t* kd_pos,
                                    int64_t* kp_off, unsigned long long* max_docs) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p <= n_part) kp_off[p] = kd_pos[part_doc_off[p]];
  if (p < n_part)  // kept documents of the largest partition (the planner's LDS table choice)
    atomicMax(max_docs, (unsigned long long)(kd_pos[part_doc_off[p + 1]] - kd_pos[part_doc_off[p]]));
}

// ---------------------------------------------------------------------------------------------
// Wave-uniform CPython MT19937 (Modules/_randommodule.c).
// Raw state and the tempered 624-word block live in LDS; draws are served from a register
// window (lane l holds word wbase+l) through readlane, so a draw costs a few instructions.
// Every lane executes the same sequential algorithm with identical scalars (uniform control
// flow); only parallel phases (twist, temper, speculative shuffle draws) use the lanes.
// ---------------------------------------------------------------------------------------------
constexpr int kN = 624, kM = 397;
constexpr int kLook = 64;  // MT words of look-ahead past the block (WaveRng)
constexpr int64_t kPoolChunk = 4096;  // mask pool entries reserved per atomic

__device__ inline int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ inline uint32_t rdlane(uint32_t v, int idx) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, uni(idx));
}
__device__ inline uint32_t temper(uint32_t y) {
  y ^= (y >> 11);
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= (y >> 18);
  return y;
}

struct WaveRng {
  // LDS: the raw 624-word block followed by kLook words of look-ahead, the next block's first
  // words (next[i] = twist1(cur[i], cur[i+1], cur[i+397]) for i < 227 depends on the current
  // block alone). mti indexes that extended stream: a window starting at mti < 624 may read up to
  // kLook words past it without a block check, and the twist runs when a window or a register
  // refill starts at mti >= 624 (mti -= 624 afterwards).
  uint32_t* mt;
  int mti;       // next word (uniform), < kN + kLook
  int wbase;     // register window base (uniform)
  int wend;      // wbase + 64 while the register window is valid, 0 when stale (uniform)
  uint32_t win;  // this lane's tempered word temper(mt[wbase + lane])
#ifdef LDDL_STAMPS
  uint64_t n_pass = 0, n_win = 0;  // diagnostics: Jacobi passes / Fisher-Yates windows
#endif

  __device__ static uint32_t twist1(uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
    return c ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
  }

  // Regenerate the block in place with all 64 lanes: ten straight-line rounds of 64 consecutive
  // words (no exec-mask loops), then the look-ahead. Word i reads old[i], old[i+1] and old[i+397]
  // (i < 227) or new[i-227], written three rounds earlier; a round reads before it writes, and
  // one wave's LDS operations complete in order, so the rounds need only a compiler fence. Word
  // 623 reads "old[624]" = the look-ahead word 0 = new[0] (seed_i64 sets it for the first block);
  // round 9's lanes past 623 write scratch into the look-ahead, which the last round overwrites.
  __device__ void twist() {
    const int l = threadIdx.x;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
      const int i = 64 * r + l;
      const int ci = r < 3 ? i + kM : r > 3 ? i - (kN - kM) : (l < kN - kM - 192 ? i + kM : i - (kN - kM));
      const uint32_t v = twist1(mt[i], mt[i + 1], mt[ci]);
      mt[i] = v;
      __asm__ volatile("" ::: "memory");
    }
    mt[kN + l] = twist1(mt[l], mt[l + 1], mt[l + kM]);  // look-ahead: next block's words 0..63
    __asm__ volatile("" ::: "memory");
    mti -= kN;
    wbase = -1024;
    wend = 0;
  }
  __device__ void ensure() {
    if (mti >= kN) twist();
  }

  __device__ void seed_i64(int64_t seed) {  // random.seed(int): init_by_array(abs(seed) limbs)
    if (threadIdx.x == 0) {
      const uint64_t a = seed < 0 ? (uint64_t)(-(seed + 1)) + 1 : (uint64_t)seed;
      const uint32_t key[2] = {(uint32_t)a, (uint32_t)(a >> 32)};
      const int klen = key[1] ? 2 : 1;
      uint32_t prev = 19650218u;
      mt[0] = prev;
      for (int i = 1; i < kN; ++i) {
        prev = 1812433253u * (prev ^ (prev >> 30)) + (uint32_t)i;
        mt[i] = prev;
      }
      int i = 1, j = 0;
      prev = mt[0];
      for (int k = kN; k; --k) {
        const uint32_t v = (mt[i] ^ ((prev ^ (prev >> 30)) * 1664525u)) + key[j] + (uint32_t)j;
        mt[i] = v;
        prev = v;
        ++i;
        ++j;
        if (i >= kN) { mt[0] = mt[kN - 1]; prev = mt[0]; i = 1; }
        if (j >= klen) j = 0;
      }
      for (int k = kN - 1; k; --k) {
        const uint32_t v = (mt[i] ^ ((prev ^ (prev >> 30)) * 1566083941u)) - (uint32_t)i;
        mt[i] = v;
        prev = v;
        ++i;
        if (i >= kN) { mt[0] = mt[kN - 1]; prev = mt[0]; i = 1; }
      }
      mt[0] = 0x80000000u;
      mt[kN] = twist1(mt[0], mt[1], mt[kM]);  // look-ahead word 0 (= the first twist's new[0])
    }
    __syncthreads();
    mti = kN;  // CPython leaves index = N after seeding: the first draw twists
    wbase = -1024;
    wend = 0;
  }

  // out of line: runs once per 64 draws (window load) or per 624 draws (twist)
  __device__ void refill() {
    ensure();
    wbase = mti;
    wend = mti + 64;
    win = temper(mt[mti + (int)threadIdx.x]);
  }
  __device__ uint32_t u32() {
    if (mti >= wend) refill();  // one scalar compare per draw
    const uint32_t v = rdlane(win, mti - wbase);
    mti = uni(mti + 1);
    return v;
  }
  // Fisher-Yates draws of random.shuffle over n items: j_i = _randbelow(i+1), i = n-1 .. 1,
  // delivered as sink(off, j) by every lane of every window: off = i for the lane whose word
  // is drawn for step i and accepted, 0 for every other lane (rejected words, words past the
  // end; index 0 of a draw array is never read, so the sink stores unconditionally - no
  // exec-mask branch per window). Wave-parallel over a window of 64 words (lane t holds word t).
  // Word t of the window is drawn for step i_t = s0 - t + R_t (R_t = rejections before t) and
  // rejected iff (w_t >> (32 - bit_length(i_t + 1))) > i_t, i.e. with u = i + 1 (the draw's
  // bound) iff (w_t >> clz(u)) >= u. R is the fixed point of R_t = #{v < t : rejected under
  // R_v}, found by Jacobi iteration on ballots: the recurrence is causal, so every pass fixes at
  // least the first wrong word. Words past the last step (u <= 1) come after every valid word
  // and do not affect their R; they are held "accepted" (a verdict that followed their R would
  // keep changing and cost passes: 11.7 instead of ~5 per window), and the first of them ends
  // the shuffle. The window's bookkeeping is branch-free scalar work (s_ff1 / s_bcnt1).
  template <typename Sink>
  __device__ void fy_draws(int32_t n, Sink sink) {
    const int lane = threadIdx.x;
    int32_t s0 = n - 1;  // next step (uniform); n < 2^30 (host-checked)
    while (s0 >= 1) {
      ensure();
      const uint32_t w = temper(mt[mti + lane]);
      const int32_t u1 = s0 + 1 - lane;
      // Jacobi start: ~0.3 rejections per word (any start converges to the same fixed point,
      // the left-most wrong word being fixed by every pass; simulated: 5.3 -> 4.8 passes per
      // window at target_seq_length 128)
      int32_t R = (lane * 77) >> 8;
      uint32_t x;
      uint64_t rej;
      // Convergence is tested on the rejection masks (one scalar 64-bit compare): from the second
      // pass on, R = popc_below(previous mask), so equal masks give equal R in every lane (bit 63
      // moves no R: at most one extra pass). The loop carries no vector compare and no R copy.
      if (s0 >= 64) {  // every word of the window has a step (u >= 2)
        auto pass = [&]() {
          const int32_t u = u1 + R;
          x = w >> __clz((uint32_t)u);
#ifdef LDDL_STAMPS
          ++n_pass;
#endif
          return ballot(x >= (uint32_t)u);
        };
        uint64_t prev = pass();
        R = (int32_t)popc_below(prev);
        rej = pass();
        while (rej != prev) {
          prev = rej;
          R = (int32_t)popc_below(rej);
          rej = pass();
        }
      } else {  // words past the last step (u <= 1) are held "accepted", so they settle at once
        auto pass = [&]() {
          const int32_t u = u1 + R;
          x = w >> (__clz((uint32_t)u) & 31);
#ifdef LDDL_STAMPS
          ++n_pass;
#endif
          return ballot(x >= (uint32_t)u) & ballot(u > 1);
        };
        uint64_t prev = pass();
        R = (int32_t)popc_below(prev);
        rej = pass();
        while (rej != prev) {
          prev = rej;
          R = (int32_t)popc_below(rej);
          rej = pass();
        }
      }
#ifdef LDDL_STAMPS
      ++n_win;
#endif
      const int32_t i = u1 + R - 1;  // the lane's step (<= 0 past the end)
      // (the verdict is recomputed here rather than carried out of the loop as a lane mask)
      sink(x > (uint32_t)i ? 0 : max(i, 0), x);
      // the shuffle ends at the first word past the last step (E); words < E are consumed. After
      // such a window s0 - (64 - popc(rej)) <= 0, since the held words count as accepted.
      const uint64_t fin = ballot(i < 1);
      mti = uni(mti + (fin ? (int)__ffsll((unsigned long long)fin) - 1 : 64));
      s0 -= 64 - (int32_t)__popcll(rej);
    }
    wbase = -1024;
    wend = 0;  // the register window is stale
  }
  // _truncate_seq_pair draws (pretrain.py:161-176). T = na + nb - max_num trims; trim t hits A
  // iff A is the longer side at that point, which has a closed form: with d = na - nb the first
  // |d| trims hit the longer side, then B and A alternate starting with B (ties trim B). Each
  // trim is from the front iff random() < 0.5, i.e. iff the first of its two words is < 2^31, so
  // 32 trims (64 words, the look-ahead) resolve per wave pass with two ballots.
  __device__ void trunc_draws(int32_t& na, int32_t& nb, int32_t max_num, int32_t& a_front,
                              int32_t& b_front) {
    const int32_t T = na + nb - max_num;
    if (T <= 0) return;
    const int32_t d = na - nb, ad = d < 0 ? -d : d;
    const int lane = threadIdx.x;
    for (int32_t done = 0; done < T;) {
      ensure();
      const int32_t cnt = min(T - done, 32);
      const int32_t t = done + lane;
      // random() < 0.5 <=> the tempered first word's top bit is clear; tempering is linear over
      // GF(2) and that bit is the parity of raw bits 31, 27, 24 and 16
      // (every lane reads: mti + 126 stays inside the LDS block; lanes >= cnt are masked off
      // by the scalar lane mask, not by an exec-mask branch)
      const uint32_t par = __popc(mt[mti + 2 * lane] & 0x89010000u) & 1u;
      const uint64_t F = ballot(par == 0) & ((1ull << cnt) - 1);  // cnt <= 32
      const int32_t x = t - ad;
      const uint64_t S = ballot(t < d) | (ballot(x >= 0) & ballot((x & 1) != 0));
      a_front += __popcll(F & S);
      b_front += __popcll(F & ~S);
      mti = uni(mti + 2 * cnt);
      done += cnt;
    }
    wbase = -1024;
    wend = 0;
    const int32_t nA = (d > 0 ? min(d, T) : 0) + (T > ad ? (T - ad) / 2 : 0);
    na -= nA;
    nb -= T - nA;
  }

  // Decisions of create_masked_lm_predictions (pretrain.py:208-221) for cnt masked tokens:
  // random() < 0.8 -> [MASK]; else random() < 0.5 -> keep; else vocab_words[randint(0, V-1)].
  // Lane t tabulates the decision and word count of a token whose first word is mti + t (only
  // decisions whose words lie in the 64-word look-ahead); the chain of decision starts p_0 = 0,
  // p_{k+1} = p_k + len[p_k] is then resolved for every k at once by pointer doubling
  // (ds_bpermute), so lane k learns where decision k starts (a window holds <= 32 decisions).
  // cnt <= 64; returns decision `lane` in each lane < cnt.
  __device__ int32_t mask_decisions(int cnt, uint64_t lt08, int32_t V, int32_t mask_id) {
    const int lane = threadIdx.x;
    const int kV = 32 - __clz((uint32_t)V);
    int32_t res = 0;
    int c = 0;
    while (c < cnt) {
      ensure();
      // word t + j of the window reaches lane t by j whole-wave DPP shifts (one LDS read and one
      // temper per lane); only words inside the look-ahead are used
      const uint32_t* wp = mt + mti + lane;
      const uint32_t w0 = temper(wp[0]);
      const uint32_t w1 = (uint32_t)wave_next((int)w0), w2 = (uint32_t)wave_next((int)w1),
                     w3 = (uint32_t)wave_next((int)w2), w4 = (uint32_t)wave_next((int)w3);
      (void)w3;
      // random() < 0.8 <=> N = (w0 >> 5) * 2^26 + (w1 >> 6) < lt08 <=> (w0 >> 5) * 2^32 + w1 <
      // lt08 * 64 (w1's low 6 bits cannot carry past a multiple of 64): one shift, one compare
      const uint64_t N64 = ((uint64_t)(w0 >> 5) << 32) | w1;
      // the decision at word t: [MASK] (2 words), else keep (random() < 0.5: w2's top bit clear,
      // 4 words), else a random word (randint's first word w4 accepted: 5 words; rejected: the
      // rare scan below); len 0 when the decision's words run past the look-ahead. Written as
      // selects on three compares and a shift, so that no lane-mask logic runs on the scalar unit.
      const bool mk = N64 < (lt08 << 6);
      const uint32_t top = w2 >> 31;  // 1: not keep
      const uint32_t r4 = w4 >> (32 - kV);
      const bool r4ok = r4 < (uint32_t)V;
      const int need = mk ? 2 : 4 + (int)top;
      int len = lane + need > kLook ? 0 : mk ? 2 : top ? (r4ok ? 5 : 0) : 4;
      int32_t tok = mk ? mask_id : top ? (int32_t)r4 : kKeep;
      if (!mk && top && !r4ok) {  // randint rejected its first word: scan on (rare)
        for (int j = 5; lane + j < kLook; ++j) {
          const uint32_t r = temper(wp[j]) >> (32 - kV);
          if (r < (uint32_t)V) {
            len = j + 1;
            tok = (int32_t)r;
            break;
          }
        }
      }
      // J_b[t] = start after 2^b decisions from t (64: stop, absorbing)
      int Jd[5];
      Jd[0] = len ? min(lane + len, 64) : 64;
#pragma unroll
      for (int b = 1; b < 5; ++b) {
        const int y = __shfl(Jd[b - 1], Jd[b - 1] & 63, 64);
        Jd[b] = Jd[b - 1] >= 64 ? 64 : y;
      }
      int p = 0;  // start of decision `lane` (lanes < 32)
#pragma unroll
      for (int b = 0; b < 5; ++b) {
        const int t = __shfl(Jd[b], p & 63, 64);
        if ((lane >> b) & 1) p = p >= 64 ? 64 : t;
      }
      const int lp = __shfl(len, p & 63, 64);
      const int32_t tp = __shfl(tok, p & 63, 64);
      // a prefix of the lanes (two compares, the scalar unit ANDs their ballots)
      const uint64_t okm = ballot(p < 64) & ballot(lp > 0) & 0xFFFFFFFFull;
      int take = __ffsll((unsigned long long)~okm) - 1;
      if (take > cnt - c) take = cnt - c;
      const int32_t tk = __shfl(tp, (lane - c) & 63, 64);  // decision k goes to lane c + k
      if (lane >= c && lane < c + take) res = tk;
      if (take > 0) {
        mti = uni(mti + (int)rdlane((uint32_t)p, take - 1) + (int)rdlane((uint32_t)lp, take - 1));
        c += take;
      } else {  // the first decision needs words past the look-ahead: draw it word by word
        wbase = -1024;
        wend = 0;
        int32_t t2;
        if (rand53() < lt08) t2 = mask_id;
        else if (below_half()) t2 = kKeep;
        else t2 = (int32_t)randint(0, V - 1);
        if (lane == c) res = t2;
        ++c;
      }
    }
    wbase = -1024;
    wend = 0;
    return res;
  }

  // random() = N / 2^53 with N = (w1 >> 5) * 2^26 + (w2 >> 6). `random() < p` is decided exactly
  // on N: N < ceil(p * 2^53) (see k_short / kLt08), so no floating point is needed.
  // two consecutive words with one window check when both are in the window
  __device__ void u32x2(uint32_t& a, uint32_t& b) {
    if (mti + 1 < wend) {
      a = rdlane(win, mti - wbase);
      b = rdlane(win, mti + 1 - wbase);
      mti = uni(mti + 2);
    } else {
      a = u32();
      b = u32();
    }
  }
  __device__ uint64_t rand53() {
    uint32_t a, b;
    u32x2(a, b);
    return ((uint64_t)(a >> 5) << 26) | (b >> 6);
  }
  __device__ bool below_half() {  // random() < 0.5  <=>  N < 2^52  <=>  w1 < 2^31
    uint32_t a, b;
    u32x2(a, b);
    return a < 0x80000000u;
  }
  __device__ uint32_t randbelow(uint32_t n) {
    const int k = 32 - __clz(n);
    uint32_t r = u32() >> (32 - k);
    while (r >= n) r = u32() >> (32 - k);
    return r;
  }
  __device__ int64_t randint(int64_t a, int64_t b) { return a + randbelow((uint32_t)(b - a + 1)); }
  __device__ int32_t randint32(int32_t a, int32_t b) { return a + (int32_t)randbelow((uint32_t)(b - a + 1)); }

};

// Token ids of the pair tables (the dense kept tokens, the sample tokens and labels): 2 bytes each
// when the vocab fits uint16 (lddl_ctx::id_bytes), else 4. The hot reader (gather_kernel) is
// templated on the type; the rare paths read through this runtime-width view.
struct IdPtr {
  void* p;
  int32_t ib;
  __device__ int32_t ld(int64_t i) const {
    return ib == 2 ? (int32_t)static_cast<const uint16_t*>(p)[i] : static_cast<const int32_t*>(p)[i];
  }
  __device__ void st(int64_t i, int32_t v) const {
    if (ib == 2) static_cast<uint16_t*>(p)[i] = (uint16_t)v;
    else static_cast<int32_t*>(p)[i] = v;
  }
};

struct PlanArgs {
  // kept corpus
  const int64_t* kscan;  // dense token offset of each kept sentence
  const int32_t* ks_len;
  const int64_t* kd_off;
  const int64_t* kp_off;
  const int64_t* ks_start;  // kept sentence k's pieces at ids[ks_start[k] ...]: the tokenizer's
  const int32_t* ids;       // layout (`dense` is filled by this launch's tail workgroups)
  IdPtr dense;              // out: kept tokens, packed (densify_group)
  int64_t n_kept_sent;
  int32_t n_part, n_dense_wg;  // workgroups >= n_part fill `dense`
  // one launch plans partitions [p0, p0 + n_part) (a split plan: a head and a tail launch); its
  // dense workgroups pack kept sentences [*dense_lo, n_kept_sent) (null: from 0)
  int32_t p0;
  const int64_t* dense_lo;
  const int64_t* part_seed;
  // params
  int32_t seq, dup, masking, vocab_size, cls_id, sep_id, mask_id, max_pred;
  double short_seq_prob, ratio;
  uint64_t k_short;  // random() < short_seq_prob  <=>  N < k_short = ceil(short_seq_prob * 2^53)
  int32_t seq_r64;   // seq rounded up to a multiple of 64
  // outputs, slot base of partition p = dup * kd_off[kp_off[p]]
  PairDesc* desc;
  int32_t* jseq;       // per slot: j_i draws of the final partition shuffle
  SlotPool* spool;     // per slot (masking)
  int32_t* mtok;       // mask pool: slot s's decisions at 8 * moff8 .. + nmask (shuffled order)
  void* jpool;         // draw pool: j_i of random.shuffle(cand_indexes) at 16 * joff16 + i
  int32_t jbytes;      // 1 (target_seq_length <= 256: every j_i < 256) or 2 bytes per draw
  unsigned long long* pool_used;  // [0] masks, [1] overflow flag, [2] draws
  int64_t pool_cap, jpool_cap;
  int32_t* overflow;   // set when the pool is too small (the host re-plans with a larger one)
  int64_t* part_npairs;
  uint64_t* stamps;  // diagnostic build: [n_part][8]
  uint64_t* tl;      // diagnostic build: [n_part][2] s_memrealtime at start / end (100 MHz)
  // time-sliced mode (plan_replay_kernel<.., true>; see "The time-sliced mode" below)
  unsigned* sl_ctl;   // [0] tickets claimed, [1] ring entries reserved (= hand-offs),
                      // [2] dense groups claimed, [3] unused; zeroed with the ring on every launch
  unsigned* sl_ring;  // [sl_ring_cap] 0 = not published, partition + 1, or kRingAbandoned
  uint64_t* sl_save;  // [n_part][kSaveU64] a parked partition's state
  int32_t sl_ring_cap;
  int32_t sl_dense;    // 1: the waves that leave the queue pack `dense`
  int32_t sl_quantum;  // documents per slice; 0: 1/kPlanSliceK of the partition's dup * documents
  uint64_t* tls;       // diagnostic build: [n_part + sl_ring_cap][2] slice start / end by ticket
};

constexpr int kDocLds = 512;  // partitions with <= this many documents cache offsets in LDS
constexpr uint64_t kLt08 = 7205759403792794ull;  // ceil(0.8 (binary64) * 2^53): random() < 0.8

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

// Kept tokens packed densely (see densify_kernel below):
// one wave: kept sentences [k0, k0 + 64)
__device__ inline void densify_group(int64_t k0, const int64_t* __restrict__ ks_start,
                                     const int32_t* __restrict__ ks_len,
                                     const int64_t* __restrict__ kscan, int64_t n,
                                     const int32_t* __restrict__ ids, IdPtr dense) {
  const int lane = threadIdx.x & 63;
  const int64_t k = k0 + lane;
  const bool ok = k < n;
  const int32_t len = ok ? ks_len[k] & kLenMask : 0;
  const int64_t st = ok ? ks_start[k] : 0;
  const int32_t incl = wave_incl_scan(len);
  const int32_t total = __builtin_amdgcn_readlane(incl, 63);  // (uniform: scalar loop bounds)
  const int64_t base = kscan[k0];
  // the sentence loop indices are wave-uniform: lane values via readlane, not LDS permutes
  auto rl = [](int32_t v, int i) { return __builtin_amdgcn_readlane(v, i); };
  // kU chunks of 64 tokens per round: their sources first, then all kU loads, then the stores,
  // so a wave has kU loads in flight instead of one dependent load -> store per chunk
  constexpr int kU = 4;  // (8: 6.0 -> 6.3 ms, profiles/r06y)
  int j = 0;
  for (int32_t c0 = 0; c0 < total; c0 += 64 * kU) {
    int64_t src[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int32_t cu = c0 + 64 * u, x = cu + lane, hi = min(cu + 63, total - 1);
      src[u] = 0;
      if (cu < total) {
        while (rl(incl, j) <= cu) ++j;  // first sentence overlapping the chunk
        for (int jj = j;; ++jj) {
          const int32_t e = rl(incl, jj);
          const int32_t b = e - rl(len, jj);
          const int64_t s = ((int64_t)rl((int32_t)(st >> 32), jj) << 32) | (uint32_t)rl((int32_t)st, jj);
          if (x >= b && x < e) src[u] = s + (x - b);
          if (e > hi) break;
        }
      }
    }
    int32_t v[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) v[u] = c0 + 64 * u + lane < total ? ids[src[u]] : 0;
#pragma unroll
    for (int u = 0; u < kU; ++u)
      if (c0 + 64 * u + lane < total) dense.st(base + c0 + 64 * u + lane, v[u]);
  }
}

// waves per SIMD the compiler must keep: 8 caps the kernel at 78 SGPRs (140 spilled to VGPR
// lanes); 6 lets it use all 106 (59 spilled) at 7 waves/SIMD, 176 -> 169.6 ms per 10 GB
// (profiles/r02_plan_minw_ab.txt)
// kDocsLds: every partition's document offsets fit the LDS table (host-checked: <= kDocLds
// documents), so the document lookups carry no global-memory branch; kJB: bytes per shuffle draw
//
// The time-sliced mode (kSliced; a one-range plan of more partitions than the device holds
// waves). The grid is persistent one-wave workgroups, as many as the device holds. A wave plans
// a partition for a quantum of documents, parks it at the document boundary and takes the next
// item of a global FIFO, so every partition gets slice k before any gets slice k + 1 and all
// the chains end together, with every wave slot busy until then.
//   Tickets, all claimed by a returning add on sl_ctl[0], the first one when the wave starts: a
//   workgroup owns no work by its index, so one that becomes resident late (measured with the
//   first tickets bound to the workgroup index: 1,024 of 7,168 started when the others left and
//   planned their partitions alone, 152 ms) finds the queue as it then is. Ticket t < n_part is
//   the fresh partition t (seeded as in the one-shot mode), ticket n_part + r is entry r of a
//   ring that never wraps (the host sizes it from the quantum: plan_slice_ring_entries).
//   Parking. The wave writes the partition's state (the MT block with its look-ahead, mti, the
//   loop position, np and the partition's pool chunks: kSaveU64 granules) to the partition's save
//   area with write-through agent-scope stores, drains them (s_waitcnt vmcnt(0)), reserves a ring
//   index with one returning add on sl_ctl[1] and publishes partition + 1 there by an atomic
//   exchange. Then it claims its next ticket.
//   Claiming. The claimant of ring entry r exchanges kRingAbandoned into it. A partition id
//   coming back is its work item: one agent-scope acquire, then the state is read by vector loads
//   (lane-indexed addresses, through LDS; the uniform words become scalars by readfirstlane). Zero
//   coming back (after kPopTries looks: the entry is reserved but not yet written, or the ring is
//   empty) means the wave leaves the queue for good.
//   No wave waits for another, and nothing is lost: the exchanges on one ring word are totally
//   ordered, so either the claimant sees the partition id and owns the partition, or the
//   publisher sees kRingAbandoned and keeps its partition for another slice (it alone ever held
//   it). Every ticket below the final sl_ctl[0] has exactly one claimant, and the final count
//   covers every published entry: each slice end (a parking that was not handed back, or a
//   finished partition) is followed by one claim, which makes n_part + published - abandoned
//   claims on top of the waves' first ones, and no more entries are ever abandoned than there are
//   waves (a wave abandons one entry, then leaves). So no workgroup's progress depends on another
//   being resident, and the launch ends whatever the dispatch order.
//   The pool chunks belong to the partition here (parked with it), not to the wave: the pools'
//   total use is then the same whichever wave plans which slice, which the exact-size re-plan
//   after a pool overflow relies on.
//   A wave that leaves the queue packs `dense`: groups of kept sentences claimed from sl_ctl[2].
constexpr int kSaveHdr = 16;                            // header words behind the MT block
constexpr int kSaveU64 = (kN + kLook + kSaveHdr) / 2;   // 8-byte granules per parked partition
constexpr int kPopTries = 4;                            // looks at a ring entry that reads zero
constexpr unsigned kRingAbandoned = 0xFFFFFFFFu;
constexpr int kDenseClaim = 4;                          // 64-sentence groups per claim
static_assert((kN + kLook + kSaveHdr) % 2 == 0 && kSaveHdr <= kDocLds, "save area layout");

#define LDDL_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// Claims the wave's next ticket (uniform): -1 = leave the queue, else the ticket, with *part the
// partition to plan (fresh when ticket < n_part, else parked).
__device__ inline int32_t slice_claim(const PlanArgs& A, int32_t* part) {
  int32_t t_out = -1, p_out = 0;
  if (threadIdx.x == 0) {
    const unsigned t = __hip_atomic_fetch_add(&A.sl_ctl[0], 1u, LDDL_RLX_AGENT);
    if (t < (unsigned)A.n_part) {
      t_out = (int32_t)t;
      p_out = (int32_t)t;
    } else if (t - (unsigned)A.n_part < (unsigned)A.sl_ring_cap) {
      unsigned* e = A.sl_ring + (t - (unsigned)A.n_part);
      for (int tries = 1; tries < kPopTries; ++tries) {  // (bounded: then the exchange decides)
        if (__hip_atomic_load(e, LDDL_RLX_AGENT) != 0) break;
        __builtin_amdgcn_s_sleep(4);
      }
      const unsigned v = __hip_atomic_exchange(e, kRingAbandoned, LDDL_RLX_AGENT);
      if (v != 0 && v != kRingAbandoned) {
        t_out = (int32_t)t;
        p_out = (int32_t)(v - 1);
      }
    }
  }
  *part = uni(p_out);
  return uni(t_out);
}

// Publishes the parked partition p (its state is stored and drained). true: handed on; false: the
// entry had been abandoned (or the ring is full), the wave keeps the partition.
__device__ inline bool slice_publish(const PlanArgs& A, int32_t p) {
  int32_t on = 0;
  if (threadIdx.x == 0) {
    const unsigned r = __hip_atomic_fetch_add(&A.sl_ctl[1], 1u, LDDL_RLX_AGENT);
    if (r < (unsigned)A.sl_ring_cap)
      on = __hip_atomic_exchange(A.sl_ring + r, (unsigned)p + 1u, LDDL_RLX_AGENT) == 0;
  }
  // the publish is complete before the wave's own claim reads the queue
  __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
  return uni(on) != 0;
}

template <bool kDocsLds, int kJB, bool kSliced = false>
__global__ void __launch_bounds__(64, 6) plan_replay_kernel(PlanArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint32_t* s_mt = reinterpret_cast<uint32_t*>(smem);
  int32_t* s_doc = reinterpret_cast<int32_t*>(s_mt + kN + kLook);  // [kDocLds + 1]
  const int lane = threadIdx.x;
  const bool leader = lane == 0;
  if (!kSliced && (int)blockIdx.x >= A.n_part) {
    // Workgroups past the partitions pack `dense` (what densify_kernel would do after this
    // launch). Dispatched in order, they start as the last partitions' waves are placed and
    // run in the slots the planner's tail leaves idle (a separate launch before or beside the
    // planner delays its dispatch).
    const int64_t k_lo = A.dense_lo ? *A.dense_lo : 0;
    for (int64_t g = (int)blockIdx.x - A.n_part; k_lo + g * 64 < A.n_kept_sent; g += A.n_dense_wg)
      densify_group(k_lo + g * 64, A.ks_start, A.ks_len, A.kscan, A.n_kept_sent, A.ids, A.dense);
    return;
  }
  // sliced: the wave's current ticket and whether the partition is taken up from its save area
  [[maybe_unused]] int32_t ticket = 0;
  [[maybe_unused]] bool parked = false;
  int p = A.p0 + (int)blockIdx.x;
  if constexpr (kSliced) {
    ticket = slice_claim(A, &p);
    parked = ticket >= A.n_part;
  }
  if (!kSliced || ticket >= 0) do {  // (sliced: one slice per turn; else the body runs once)
#ifdef LDDL_STAMPS
  uint64_t st_acc[kStampRegions] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
  [[maybe_unused]] uint64_t st_t = STAMP_T();
#ifdef LDDL_STAMPS
  const uint64_t rt0 = __builtin_amdgcn_s_memrealtime();
#endif
  WaveRng rng{s_mt, 0, 0, 0, 0u
#ifdef LDDL_STAMPS
              , 0, 0
#endif
  };
  // this wave's current chunks of the mask pool and of the shuffle-draw pool: next entry, entries
  // left (32-bit compares), and whether the chunk lies inside the pool
  int64_t pool_cur = 0, jpool_cur = 0;
  int32_t pool_left = 0, jpool_left = 0;
  bool pool_fits = true, jpool_fits = true;
  int64_t np = 0;
  // sliced: where the slice starts (dp0, di0), and the documents left in it
  [[maybe_unused]] int dp0 = 0;
  [[maybe_unused]] int32_t di0 = 0, slice_left = 0;
  [[maybe_unused]] bool yielded = false;
  if (kSliced && parked) {
    // the one acquire of the hand-off, then the state by vector loads (lane-indexed addresses)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    uint64_t* sv = A.sl_save + (int64_t)p * kSaveU64;
    uint64_t* s64 = reinterpret_cast<uint64_t*>(s_mt);
    for (int i = lane; i < kSaveU64; i += 64) s64[i] = sv[i];
    __syncthreads();
    const int32_t* h = s_doc;  // the header words follow the MT block
    rng.mti = uni(h[0]);
    dp0 = uni(h[1]);
    di0 = uni(h[2]);
    np = ((int64_t)uni(h[11]) << 32) | (uint32_t)uni(h[3]);
    pool_cur = ((int64_t)uni(h[5]) << 32) | (uint32_t)uni(h[4]);
    pool_left = uni(h[6]);
    jpool_cur = ((int64_t)uni(h[8]) << 32) | (uint32_t)uni(h[7]);
    jpool_left = uni(h[9]);
    const int32_t fb = uni(h[10]);
    pool_fits = (fb & 1) != 0;
    jpool_fits = (fb & 2) != 0;
    __syncthreads();  // (before the document table overwrites the header)
  } else {
    rng.seed_i64(A.part_seed[p]);
  }
  const int64_t d0 = A.kp_off[p];
  const int32_t nd = (int32_t)(A.kp_off[p + 1] - d0);  // (partition-local indices are 32-bit)
  const int64_t kbase = A.kd_off[d0];
  if (kDocsLds)
    for (int64_t d = lane; d <= nd; d += 64) s_doc[d] = (int32_t)(A.kd_off[d0 + d] - kbase);
  __syncthreads();
  auto doc_loc = [&](int32_t d) -> int32_t {  // first kept sentence of document d, partition-local
    if constexpr (kDocsLds) return uni(s_doc[d]);
    else return uni((int32_t)(A.kd_off[d0 + d] - kbase));
  };
  const int32_t* ks_len_p = A.ks_len + kbase;
  const int64_t base = (int64_t)A.dup * kbase;
  const int32_t max_num = A.seq - 3;
  LenWin La, Lb;
  constexpr int kPrioLevels = 4;  // priority levels used (s_setprio has 4)
  // issue priority by progress: a SIMD issues its highest-priority (then oldest) wave first, so
  // waves that are behind (e.g. a partition dispatched into a freed slot) catch up and the waves
  // of a SIMD finish together instead of leaving the last ones running alone
  int prio_q = -1;
  const int64_t prio_tot = (int64_t)A.dup * nd;
  // the priority steps at the document counts where progress crosses a quarter (no 64-bit
  // division per document)
  int32_t prio_next = 0, prio_done = 0;
  if constexpr (kSliced) {  // the slice's quantum (plan_slice_quantum, per partition)
    const int64_t q = A.sl_quantum ? (int64_t)A.sl_quantum
                                   : (prio_tot + kPlanSliceK - 1) / kPlanSliceK;
    slice_left = (int32_t)std::min<int64_t>(std::max<int64_t>(q, 1), INT32_MAX);
  }
  if (nd > 0) La.prefetch(ks_len_p + doc_loc(di0), doc_loc(di0 + 1) - doc_loc(di0));
  for (int dp = dp0; dp < A.dup; ++dp) {
    for (int32_t di = di0; di < nd; ++di) {
      if constexpr (kSliced) {
        if (slice_left == 0) {
          // The quantum is used up and document (dp, di) is still to plan: park the partition.
          // The header words go behind the MT block in LDS (over the document table, which the
          // next slice loads again), then the block leaves as 8-byte write-through stores.
          int32_t hw = 0;
          const int32_t hv[12] = {rng.mti, dp, di, (int32_t)np, (int32_t)pool_cur,
                                  (int32_t)(pool_cur >> 32), pool_left, (int32_t)jpool_cur,
                                  (int32_t)(jpool_cur >> 32), jpool_left,
                                  (pool_fits ? 1 : 0) | (jpool_fits ? 2 : 0), (int32_t)(np >> 32)};
#pragma unroll
          for (int k = 0; k < 12; ++k)
            if (lane == k) hw = hv[k];
          __syncthreads();
          if (lane < kSaveHdr) s_doc[lane] = hw;
          __syncthreads();
          uint64_t* sv = A.sl_save + (int64_t)p * kSaveU64;
          const uint64_t* s64 = reinterpret_cast<const uint64_t*>(s_mt);
          for (int i = lane; i < kSaveU64; i += 64) __hip_atomic_store(sv + i, s64[i], LDDL_RLX_AGENT);
          __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");  // drained before the publish
          yielded = true;
          break;
        }
        --slice_left;
      }
      if (!kSliced && prio_done >= prio_next) {
        ++prio_q;
        prio_next = (int32_t)(((int64_t)(prio_q + 1) * prio_tot + kPrioLevels - 1) / kPrioLevels);
        const int lvl = kPrioLevels - 1 - prio_q;
        if (lvl >= 3) __builtin_amdgcn_s_setprio(3);
        else if (lvl == 2) __builtin_amdgcn_s_setprio(2);
        else if (lvl == 1) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
      }
      ++prio_done;
      const int32_t ls0 = doc_loc(di);
      const int64_t s0 = kbase + ls0;
      const int ns = doc_loc(di + 1) - ls0;
      // (the document's first length window was loaded one document ago; 1.5 ms per 10 GB,
      // profiles/r06p2_planner_loop_ab.txt)
      La.reset_prefetched(ks_len_p + ls0, ns);
      {
        const int32_t dn = di + 1 < nd ? di + 1 : 0;  // the next document (of this or the next pass)
        const int32_t nl0 = doc_loc(dn);
        La.prefetch(ks_len_p + nl0, doc_loc(dn + 1) - nl0);
      }
      int32_t target = max_num;
      if (rng.rand53() < A.k_short) target = rng.randint32(2, max_num);
      // chunks: sentences are accumulated until the target length or the document end
      // (pretrain.py:276-280); after a random-next pair the unused sentences are put back
      // (320-321), so the next chunk starts right after A
      for (int chunk0 = 0; chunk0 < ns;) {
        const int i = La.find(chunk0, ns, target);  // the chunk is [chunk0, i]
        const int chunk_n = i - chunk0 + 1;
        const int a_end = chunk_n >= 2 ? rng.randint32(1, chunk_n - 1) : 1;
        int32_t flags = 0;
        const int64_t la = La.sum(chunk0, chunk0 + a_end, flags);
        int64_t lb = 0, b_ks;
        int32_t rn = 0;
        int next0;
        STAMP_ADD(0, st_t);
        if (chunk_n == 1 || rng.below_half()) {
          rn = 1;
          const int64_t target_b = target - la;
          int32_t rd = 0;
          for (int t = 0; t < 10; ++t) {
            rd = rng.randint32(0, nd - 1);
            if (rd != di) break;
          }
          if (rd == di) rn = 0;
          const int32_t r0l = doc_loc(rd);
          const int rns = doc_loc(rd + 1) - r0l;
          const int rstart = rng.randint32(0, rns - 1);
          b_ks = kbase + (r0l + rstart);
          Lb.reset(ks_len_p + r0l, rns);
          const int jb = Lb.find(rstart, rns, target_b);  // B is [rstart, jb] (314-317)
          lb = Lb.sum(rstart, jb + 1, flags);
          next0 = chunk0 + a_end;
        } else {
          b_ks = s0 + chunk0 + a_end;
          lb = La.sum(chunk0 + a_end, i + 1, flags);
          next0 = i + 1;
        }
        STAMP_ADD(3, st_t);
        // _truncate_seq_pair
        int32_t a_front = 0, b_front = 0, na = (int32_t)la, nb = (int32_t)lb;
        rng.trunc_draws(na, nb, max_num, a_front, b_front);
        STAMP_ADD(5, st_t);
        const int64_t slot = base + np;
        // every lane stores the same record: the wave's identical writes merge into one, and no
        // exec-mask branch (3 scalar instructions + a branch) is spent on a leader-only store
        A.desc[slot] = PairDesc{s0 + chunk0, b_ks, a_front, na, b_front,
                                nb | (int32_t)((uint32_t)rn << 31)};
        if (A.masking) {
          // candidates = positions of [CLS] A [SEP] B [SEP] whose token is not [CLS]/[SEP]; only
          // their count matters here (fy_resolve_kernel recovers the positions)
          int32_t nc = na + nb;
          if (flags & kLenHasClsSep) {  // literal [CLS]/[SEP] inside A or B: inspect the tokens
            int32_t c = 0;
            for (int32_t t = 0; t < na + nb; ++t) {
              const int32_t tok = uni(t < na ? span_token(A, s0 + chunk0, a_front + t)
                                             : span_token(A, b_ks, b_front + (t - na)));
              c += tok != A.cls_id && tok != A.sep_id;
            }
            nc = uni(c);
          }
          STAMP_ADD(1, st_t);
          // num_to_predict = round(len(tokens) * masked_lm_ratio) (pretrain.py:197): binary64
          // product, round half to even - the IEEE operations Python performs
          int32_t num = uni((int32_t)__builtin_rint((double)(na + nb + 3) * A.ratio));
          if (num < 1) num = 1;
          if (num > nc) num = nc;
          // pool space for this pair's shuffle draws (nc) and masks (num): bump allocation in
          // per-wave chunks (one atomic per kPoolChunk entries); each slot records its offsets
          if (num > pool_left) {
            const int32_t sz = num > kPoolChunk ? (num + 7) & ~7 : (int32_t)kPoolChunk;
            int64_t nb0 = 0;
            if (leader) nb0 = (int64_t)atomicAdd(&A.pool_used[0], (unsigned long long)sz);
            nb0 = ((int64_t)uni((int)(nb0 >> 32)) << 32) | (uint32_t)uni((int)(uint32_t)nb0);  // lane 0's
            pool_cur = nb0;
            pool_left = sz;
            pool_fits = nb0 + sz <= A.pool_cap;
          }
          if (nc > jpool_left) {
            const int32_t sz = nc > kPoolChunk ? (nc + 15) & ~15 : (int32_t)kPoolChunk;
            int64_t nb0 = 0;
            if (leader) nb0 = (int64_t)atomicAdd(&A.pool_used[2], (unsigned long long)sz);
            nb0 = ((int64_t)uni((int)(nb0 >> 32)) << 32) | (uint32_t)uni((int)(uint32_t)nb0);
            jpool_cur = nb0;
            jpool_left = sz;
            jpool_fits = nb0 + sz <= A.jpool_cap;
          }
          const int64_t mb = pool_cur, jb = jpool_cur;
          // 16-byte aligned regions (fy_resolve_kernel's uint4 I/O; 1-byte draws too); chunk sizes
          // are multiples of the steps, so num <= left implies step <= left
          pool_cur += (num + 7) & ~7;
          pool_left -= (num + 7) & ~7;
          jpool_cur += (nc + 15) & ~15;
          jpool_left -= (nc + 15) & ~15;
          const bool fits = pool_fits && jpool_fits;
          if (!fits) *A.overflow = 1;  // (uniform; every lane stores the same flag)
          // random.shuffle(cand_indexes): draws j_i (i = nc-1 .. 1) to the pool
          // The region's tail [nc, nc rounded up to 16) gets j_i = i: fy_resolve's steps there move
          // an entry onto itself, so its step loop needs no per-step guard. (Entry 0 is not
          // written here: fy_draws' lanes store their rejected words there, and fy_resolve
          // takes j_0 = 0 itself.)
          const int32_t ip = nc + lane;
          if constexpr (kJB == 1) {
            uint8_t* jd = static_cast<uint8_t*>(A.jpool) + jb;
            rng.fy_draws(nc, [&](int32_t i, uint32_t j) {
              if (fits) jd[i] = (uint8_t)j;  // (fits is uniform: a scalar branch)
            });
            if (fits && ip < ((nc + 15) & ~15)) jd[ip] = (uint8_t)ip;
          } else {
            uint16_t* jd = static_cast<uint16_t*>(A.jpool) + jb;
            rng.fy_draws(nc, [&](int32_t i, uint32_t j) {
              if (fits) jd[i] = (uint16_t)j;
            });
            if (fits && ip < ((nc + 15) & ~15)) jd[ip] = (uint16_t)ip;
          }
          STAMP_ADD(2, st_t);
          // decisions of the masked candidates in shuffled order (pretrain.py:208-221)
          for (int32_t c0 = 0; c0 < num; c0 += 64) {
            const int cmax = min(64, num - c0);
            const int32_t mytok = rng.mask_decisions(cmax, kLt08, A.vocab_size, A.mask_id);
            if (fits && lane < cmax) A.mtok[mb + c0 + lane] = mytok;
          }
          STAMP_ADD(4, st_t);
          // (all lanes, as the descriptor above)
          A.spool[slot] = SlotPool{(uint32_t)(mb >> 3), (uint32_t)(jb >> 4), num, nc};
        }
        ++np;
        chunk0 = next0;
      }
    }
    if constexpr (kSliced) {
      if (yielded) break;
      di0 = 0;  // (the later passes start at the partition's first document)
    }
  }
  if (!kSliced || !yielded) {
  // random.shuffle(partition_pairs) (pretrain.py:401): record the draws j_i, i = np-1 .. 1
  // (64 at a time through writelane); shuffle_sort_kernel resolves the swaps.
  STAMP_ADD(0, st_t);
  {
    int32_t* js = A.jseq + base;
    rng.fy_draws(np, [&](int32_t i, uint32_t j) { js[i] = (int32_t)j; });  // (js[0] is never read)
  }
  STAMP_ADD(6, st_t);
  }
#ifdef LDDL_STAMPS
  if constexpr (kSliced) {  // the slices' regions add up per partition; the timeline is per ticket
    if (leader && A.stamps)
      for (int r = 0; r < kStampRegions - 1; ++r)
        atomicAdd(reinterpret_cast<unsigned long long*>(A.stamps) + (int64_t)p * kStampRegions + r,
                  (unsigned long long)st_acc[r]);
    if (leader && A.tl && !parked) A.tl[2 * (int64_t)p] = rt0;
    if (leader && A.tl && !yielded) A.tl[2 * (int64_t)p + 1] = __builtin_amdgcn_s_memrealtime();
    if (leader && A.tls && ticket >= 0) {
      A.tls[2 * (int64_t)ticket] = rt0;
      A.tls[2 * (int64_t)ticket + 1] = __builtin_amdgcn_s_memrealtime();
    }
  } else {
  st_acc[7] = rng.n_pass * 1000000 / (rng.n_win ? rng.n_win : 1);  // passes per window x 1e6
  if (leader && A.stamps)
    for (int r = 0; r < kStampRegions; ++r) A.stamps[(int64_t)p * kStampRegions + r] = st_acc[r];
  if (leader && A.tl) {
    A.tl[2 * (int64_t)p] = rt0;
    A.tl[2 * (int64_t)p + 1] = __builtin_amdgcn_s_memrealtime();
  }
  }
#endif
  if (!kSliced || !yielded) {
    if (leader) A.part_npairs[p] = np;
  }
  if constexpr (kSliced) {
    // a parked partition goes to the ring's end, unless its entry comes back abandoned: then the
    // wave keeps it (ticket -1: no claim) and takes it up from the save area like any other
    parked = yielded && !slice_publish(A, p);
    if (parked) {
      ticket = -1;
    } else {
      ticket = slice_claim(A, &p);
      parked = ticket >= A.n_part;
    }
    if (ticket < 0 && !parked) break;
  }
  } while (kSliced);
  if constexpr (kSliced) {
    // out of the queue: pack `dense` (what the one-shot launch's extra workgroups do)
    const int64_t n_grp = A.sl_dense ? (A.n_kept_sent + 63) / 64 : 0;
    while (n_grp) {
      int32_t g0 = 0;
      if (leader) g0 = (int32_t)__hip_atomic_fetch_add(&A.sl_ctl[2], (unsigned)kDenseClaim, LDDL_RLX_AGENT);
      g0 = uni(g0);
      if ((int64_t)(uint32_t)g0 >= n_grp) break;
      for (int g = 0; g < kDenseClaim && (int64_t)(uint32_t)g0 + g < n_grp; ++g)
        densify_group(((int64_t)(uint32_t)g0 + g) * 64, A.ks_start, A.ks_len, A.kscan, A.n_kept_sent,
                      A.ids, A.dense);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Native RNG mode (LDDL_RNG_NATIVE): the same algorithms (create_pairs_from_document,
// _truncate_seq_pair, create_masked_lm_predictions, the partition shuffle) drawing from
// Philox4x32-10 instead of one sequential MT19937 per partition, so every (duplicate, document)
// walk and every pair's masking runs in its own lane. A stream is keyed by
// (native_seed, part_seed[p]) and counted by the unit's or pair's index inside its partition, so
// a partition's output does not depend on how partitions are batched or sharded.
// Distributions are those of the reference: in the walk, randint / _randbelow by the same
// bit-length rejection and random() < p on the same 53-bit integer, each truncation side a fair
// coin; in the masking, the masked set a uniform num_to_predict-subset of the candidates (Floyd's
// algorithm: the shuffled prefix of pretrain.py:197-207 is a uniform subset) and 80/10/10
// decisions per masked token, both from one 32-bit draw each (exact uniform integers by Lemire's
// multiply-shift with rejection).
// ---------------------------------------------------------------------------------------------
__device__ inline uint64_t mix64(uint64_t x) {  // splitmix64 finaliser
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__device__ inline uint64_t part_key(uint64_t native_seed, int64_t part_seed) {
  return mix64(native_seed ^ mix64((uint64_t)part_seed + 0x9E3779B97F4A7C15ull));
}

enum : uint32_t { kStreamWalk = 1, kStreamMask = 2, kStreamOrder = 3, kStreamDecide = 4 };

struct CtrRng {
  uint2 key;
  uint32_t id0, id1, blk;
  uint4 buf;
  int have;
  __device__ CtrRng(uint64_t k, int64_t index, uint32_t stream)
      : key{(uint32_t)k, (uint32_t)(k >> 32)},
        id0((uint32_t)index),
        id1((uint32_t)((uint64_t)index >> 32) << 4 | stream),
        blk(0),
        have(0) {}
  __device__ uint32_t u32() {
    if (have == 0) {
      buf = Philox::gen(make_uint4(blk++, id0, id1, 0x6C64646Cu), key);
      have = 4;
    }
    --have;
    return have == 3 ? buf.x : have == 2 ? buf.y : have == 1 ? buf.z : buf.w;
  }
  __device__ uint64_t rand53() {  // the 53-bit integer behind random()
    const uint32_t a = u32() >> 5, b = u32() >> 6;
    return ((uint64_t)a << 26) | b;
  }
  __device__ bool coin() { return u32() < 0x80000000u; }
  __device__ uint32_t randbelow(uint32_t n) {  // _randbelow: k-bit draws until < n
    const int k = 32 - __clz(n);
    uint32_t r = u32() >> (32 - k);
    while (r >= n) r = u32() >> (32 - k);
    return r;
  }
  __device__ int64_t randint(int64_t a, int64_t b) { return a + randbelow((uint32_t)(b - a + 1)); }
  __device__ int32_t heads(int32_t n) {  // number of heads in n fair coins
    int32_t h = 0;
    for (; n >= 32; n -= 32) h += __popc(u32());
    if (n > 0) h += __popc(u32() & ((1u << n) - 1u));
    return h;
  }
};

struct NativeArgs {
  const int32_t* ks_len;
  const int64_t* kd_off;
  const int64_t* kp_off;
  const int64_t* kscan;
  IdPtr dense;
  const int64_t* part_seed;
  int64_t n_part, n_units, unit0;  // units dup * (kp_off[0] .. kp_off[n_part])
  uint64_t native_seed, k_short;
  int32_t seq, dup, masking, cls_id, sep_id, mask_id, vocab_size;
  double ratio;
  int64_t* ucnt;        // count pass: pairs of each (duplicate, document) unit
  const int64_t* uoff;  // emit pass: first pair of each unit (exclusive scan of ucnt)
  const int64_t* part_base;
  PairDesc* desc;
  int32_t* nmask;
  int32_t* ncand;
  int32_t* ppart;
  const int64_t* moff;
  uint16_t* mpos;
  int32_t* mtok;
  int64_t* src;
  int64_t n_pairs;
  int32_t words;  // bitmap words per lane (mask kernel)
};

// token t of the window [front, front + n) of the span starting at kept sentence k
__device__ inline int32_t win_token(const NativeArgs& A, int64_t k, int32_t front, int32_t t) {
  return A.dense.ld(A.kscan[k] + front + t);
}

// One partition's walk tables: cumulative kept-sentence lengths and document starts, both
// partition-relative. Staged in LDS when the partition fits (every length sum and search of the
// walk is then an LDS read), else read from the global prefix `g_pre` (int64 over all kept
// sentences) and kd_off. The branch is uniform over the workgroup.
struct WalkTab {
  const int32_t* s_pre;  // [nsp + 1]
  const int32_t* s_doc;  // [nd + 1]
  const int64_t* g_pre;
  const int64_t* g_doc;  // kd_off + d0
  int64_t sb, pre_sb;    // the partition's first kept sentence, g_pre[sb]
  bool lds;
  __device__ int64_t pre(int64_t i) const { return lds ? (int64_t)s_pre[i] : g_pre[sb + i] - pre_sb; }
  __device__ int32_t doc(int64_t d) const { return lds ? s_doc[d] : (int32_t)(g_doc[d] - sb); }
};

// Smallest e in [i, end) whose sentences i..e reach `need` = pre(i) + target (pre(e + 1) >= need),
// else end - 1: the chunk / random-B loops of create_pairs_from_document (pretrain.py:276-280,
// 300-304) as a galloping search over the cumulative lengths (pre(i) < need on entry).
__device__ inline int32_t first_reaching(const WalkTab& W, int32_t i, int32_t end, int64_t need) {
  int32_t a = i, b = i + 1;
  for (int32_t step = 1;; step <<= 1) {
    b = a + step;
    if (b >= end) {
      b = end;
      break;
    }
    if (W.pre(b) >= need) break;
    a = b;
  }
  if (b == end && W.pre(end) < need) return end - 1;
  while (b - a > 1) {  // pre(a) < need <= pre(b)
    const int32_t m = (a + b) >> 1;
    if (W.pre(m) >= need) b = m;
    else a = m;
  }
  return b - 1;
}

// Literal [CLS]/[SEP] among kept sentences [x, y) of the partition (rare: only partitions that
// hold one at all look).
__device__ inline int32_t range_flags(const NativeArgs& A, bool has_flags, int64_t sb, int32_t x,
                                      int32_t y) {
  int32_t f = 0;
  if (has_flags)
    for (int32_t j = x; j < y; ++j) f |= A.ks_len[sb + j];
  return f & kLenHasClsSep;
}

constexpr int kNativeThreads = 256;

// Unit r = (duplicate dp, document dl) of partition p is r = dp * nd + dl (the reference's
// `for _ in range(dup): for doc in docs` order); its global index is dup * (kp_off[p] -
// kp_off[0]) + r. One workgroup per partition: the partition's cumulative sentence lengths and
// document starts are staged in LDS, then every lane walks units, one chunk (pair) per loop
// iteration, taking the partition's next unit from an LDS counter when its unit ends - so a lane
// whose document is short does not idle while another lane's runs on. Chunk ends, A/B lengths and
// the random-next B span are LDS searches over the cumulative lengths (no per-sentence loop).
// EMIT = false counts each unit's pairs; EMIT = true replays the identical draws and writes them
// at uoff[unit].
template <bool EMIT>
__global__ void __launch_bounds__(kNativeThreads) plan_native_kernel(NativeArgs A, const int64_t* g_pre,
                                                                     int32_t lds_words) {
  extern __shared__ int32_t s_tab[];
  __shared__ int32_t s_next;
  const int64_t p = blockIdx.x;
  const int64_t d0 = A.kp_off[p], nd = A.kp_off[p + 1] - d0;
  const int64_t sb = A.kd_off[d0], nsp = A.kd_off[d0 + nd] - sb;
  WalkTab W{s_tab, s_tab + nsp + 1, g_pre, A.kd_off + d0, sb, 0,
            nsp + nd + 2 <= (int64_t)lds_words};
  bool flag_any = false;
  if (W.lds) {
    int32_t* pre = s_tab;
    int32_t* dst = s_tab + nsp + 1;
    for (int64_t i = threadIdx.x; i < nsp; i += kNativeThreads) {
      const int32_t v = A.ks_len[sb + i];
      pre[i + 1] = v & kLenMask;
      flag_any |= (v & kLenHasClsSep) != 0;
    }
    for (int64_t d = threadIdx.x; d <= nd; d += kNativeThreads) dst[d] = (int32_t)(A.kd_off[d0 + d] - sb);
    if (threadIdx.x == 0) {
      pre[0] = 0;
      s_next = kNativeThreads;
    }
    __syncthreads();
    // in-place inclusive scan of pre[1 .. nsp]: a contiguous run per thread, then the runs' sums
    const int32_t per = (int32_t)((nsp + kNativeThreads - 1) / kNativeThreads);
    const int32_t x0 = 1 + (int32_t)threadIdx.x * per;
    const int32_t x1 = min(x0 + per, (int32_t)nsp + 1);
    int32_t run = 0;
    for (int32_t x = x0; x < x1; ++x) run += pre[x];
    __shared__ int32_t s_wsum[kNativeThreads / 64];
    const int32_t inc = wave_incl_scan(run);
    if ((threadIdx.x & 63) == 63) s_wsum[threadIdx.x >> 6] = inc;
    __syncthreads();
    int32_t off = inc - run;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) off += s_wsum[w];
    for (int32_t x = x0; x < x1; ++x) {
      off += pre[x];
      pre[x] = off;
    }
  } else {
    W.pre_sb = g_pre[sb];
    for (int64_t i = threadIdx.x; i < nsp; i += kNativeThreads)
      flag_any |= (A.ks_len[sb + i] & kLenHasClsSep) != 0;
    if (threadIdx.x == 0) s_next = kNativeThreads;
  }
  const bool has_flags = __syncthreads_or(flag_any) != 0;
  const int64_t nu = (int64_t)A.dup * nd;
  const int64_t ug0 = (int64_t)A.dup * (d0 - A.kp_off[0]);  // global index of the partition's unit 0
  const uint64_t key = part_key(A.native_seed, A.part_seed[p]);
  const int32_t max_num = A.seq - 3;
  int64_t r = threadIdx.x;
  bool fresh = true;
  CtrRng rng(key, 0, kStreamWalk);
  int32_t s0 = 0, ns = 0, i = 0, target = 0, dl = 0;
  int64_t np = 0, base = 0;
  while (__builtin_amdgcn_ballot_w64(r < nu)) {
    if (r < nu) {
      if (fresh) {  // a new unit: its document and target length (pretrain.py:259-262)
        fresh = false;
        dl = (int32_t)(r % nd);
        rng = CtrRng(key, r, kStreamWalk);
        s0 = W.doc(dl);
        ns = W.doc(dl + 1) - s0;
        i = 0;
        np = 0;
        if (EMIT) base = A.uoff[ug0 + r];
        target = max_num;
        if (rng.rand53() < A.k_short) target = (int32_t)rng.randint(2, max_num);
      }
      if (i < ns) {  // one chunk -> one pair
        const int64_t c_pre = W.pre(s0 + i);
        const int32_t e = first_reaching(W, s0 + i, s0 + ns, c_pre + target) - s0;
        const int32_t chunk0 = i, chunk_n = e - i + 1;
        const int32_t a_end = chunk_n >= 2 ? (int32_t)rng.randint(1, chunk_n - 1) : 1;
        const int64_t la = W.pre(s0 + chunk0 + a_end) - c_pre;
        int64_t lb, b_ks;
        int32_t rn = 0, flags = 0;
        if (chunk_n == 1 || rng.coin()) {  // random next (pretrain.py:291-321)
          rn = 1;
          const int64_t target_b = target - la;
          int64_t rd = 0;
          for (int t = 0; t < 10; ++t) {
            rd = rng.randint(0, nd - 1);
            if (rd != dl) break;
          }
          if (rd == dl) rn = 0;
          const int32_t r0 = W.doc(rd), rns = W.doc(rd + 1) - r0;
          const int32_t rstart = (int32_t)rng.randint(0, rns - 1);
          const int64_t b_pre = W.pre(r0 + rstart);
          const int32_t be = first_reaching(W, r0 + rstart, r0 + rns, b_pre + target_b);
          lb = W.pre(be + 1) - b_pre;
          b_ks = sb + r0 + rstart;
          if (EMIT && A.masking)
            flags = range_flags(A, has_flags, sb, s0 + chunk0, s0 + chunk0 + a_end) |
                    range_flags(A, has_flags, sb, r0 + rstart, be + 1);
          i = chunk0 + a_end;  // the unused segments are put back (pretrain.py:320-321)
        } else {
          lb = W.pre(s0 + e + 1) - W.pre(s0 + chunk0 + a_end);
          b_ks = sb + s0 + chunk0 + a_end;
          if (EMIT && A.masking) flags = range_flags(A, has_flags, sb, s0 + chunk0, s0 + e + 1);
          i = e + 1;
        }
        // _truncate_seq_pair: which side each trim hits is fixed (see WaveRng::trunc_draws); front
        // or back is a fair coin per trim
        int32_t na = (int32_t)la, nb = (int32_t)lb, a_front = 0, b_front = 0;
        const int32_t T = na + nb - max_num;
        if (T > 0) {
          const int32_t dd = na - nb, ad = dd < 0 ? -dd : dd;
          const int32_t nA = (dd > 0 ? min(dd, T) : 0) + (T > ad ? (T - ad) / 2 : 0);
          a_front = rng.heads(nA);
          b_front = rng.heads(T - nA);
          na -= nA;
          nb -= T - nA;
        }
        if (EMIT) {
          const int64_t q = base + np;
          const int64_t a_ks = sb + s0 + chunk0;
          A.desc[q] = PairDesc{a_ks, b_ks, a_front, na, b_front, nb | (int32_t)((uint32_t)rn << 31)};
          A.ppart[q] = (int32_t)p;
          if (A.masking) {
            int32_t nc = na + nb;
            if (flags) {  // literal [CLS]/[SEP] in the text are not candidates
              nc = 0;
              for (int32_t t = 0; t < na + nb; ++t) {
                const int32_t tok = t < na ? win_token(A, a_ks, a_front, t)
                                           : win_token(A, b_ks, b_front, t - na);
                nc += tok != A.cls_id && tok != A.sep_id;
              }
            }
            int32_t num = (int32_t)rint((double)(na + nb + 3) * A.ratio);
            if (num < 1) num = 1;
            if (num > nc) num = nc;
            A.nmask[q] = num;
            A.ncand[q] = nc;
          }
        }
        ++np;
      }
      if (i >= ns) {  // the unit is done: take the partition's next one
        if (!EMIT) A.ucnt[ug0 + r] = np;
        r = atomicAdd(&s_next, 1);
        fresh = true;
      }
    }
  }
}

// LDS words one partition's walk tables take; the largest over all partitions
__global__ void native_part_need_kernel(const int64_t* kp_off, const int64_t* kd_off, int64_t n_part,
                                        unsigned long long* need_max) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_part) return;
  const int64_t d0 = kp_off[p], d1 = kp_off[p + 1];
  atomicMax(need_max, (unsigned long long)(kd_off[d1] - kd_off[d0] + (d1 - d0) + 2));
}

struct KeptLenOnly {
  const int32_t* v;
  __device__ int64_t operator()(int64_t i) const { return v[i] & kLenMask; }
};

__global__ void native_part_base_kernel(const int64_t* kp_off, int64_t n_part, int32_t dup,
                                        const int64_t* uoff, int64_t* part_base) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p <= n_part) part_base[p] = uoff[(int64_t)dup * (kp_off[p] - kp_off[0])];
}

// Uniform integer in [0, n) from a 32-bit draw: Lemire's multiply-shift with the exact rejection
// (taken with probability < n / 2^32, so the lanes of a wave stay in step).
__device__ inline uint32_t lemire_below(uint32_t x, uint32_t n, CtrRng& rng) {
  uint64_t m = (uint64_t)x * n;
  if ((uint32_t)m < n) {
    const uint32_t t = (0u - n) % n;
    while ((uint32_t)m < t) m = (uint64_t)rng.u32() * n;
  }
  return (uint32_t)(m >> 32);
}

// 80 / 10 / 10 of create_masked_lm_predictions (pretrain.py:214-229) on one 32-bit draw:
// [MASK] below ceil(0.8 * 2^32), the original token below ceil(0.9 * 2^32), else a random token.
constexpr uint32_t kNat80 = 3435973837u, kNat90 = 3865470567u;

// Masked positions of 64 consecutive pairs per wave (one lane per pair), in lock step so that
// every lane's Philox refill comes at the same iteration:
//  1. Floyd's sampling of num candidate indices out of nc (a uniform num-subset: the shuffled
//     prefix of pretrain.py:197-207), one draw per step, into a lane-private LDS bitmap;
//  2. the set bits in ascending order (= sorted(masked_lms, key=index)), each with an 80/10/10
//     decision from its own stream (two draws per mask, whatever the decision), staged in LDS;
//  3. the wave's masks are one contiguous run of the pool (moff is the planner-order scan), copied
//     out with coalesced stores.
// Every draw's stream position depends on the pair alone (the sampling and the decisions use
// separate streams), so a pair's masks do not depend on the pairs that share its wave.
__global__ void __launch_bounds__(256) mask_native_kernel(NativeArgs A, int32_t stage_cap) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_mn[];
  const int w = wave_id(), lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  const int64_t q0 = ((int64_t)blockIdx.x * nw + w) * 64;
  if (q0 >= A.n_pairs) return;
  uint32_t* bm = reinterpret_cast<uint32_t*>(s_mn) + (size_t)w * A.words * 64 + lane;
  int32_t* stok = reinterpret_cast<int32_t*>(s_mn + (size_t)nw * A.words * 64 * 4) + (size_t)w * stage_cap;
  uint16_t* spos = reinterpret_cast<uint16_t*>(s_mn + (size_t)nw * A.words * 64 * 4 +
                                                (size_t)nw * stage_cap * 4) + (size_t)w * stage_cap;
  const int64_t q = q0 + lane;
  const bool valid = q < A.n_pairs;
  const int64_t qv = valid ? q : q0;
  const int64_t qe = q0 + 64 < A.n_pairs ? q0 + 64 : A.n_pairs;
  const int64_t m0 = A.moff[q0];
  const int32_t mend = (int32_t)(A.moff[qe] - m0);
  const int32_t num = valid ? A.nmask[qv] : 0;
  const int32_t nc = A.ncand[qv];
  const int32_t mb = (int32_t)(A.moff[qv] - m0);
  const PairDesc d = A.desc[qv];
  const int32_t na = d.na, nb = d.nb_rn & 0x7FFFFFFF;
  const int64_t p = A.ppart[qv];
  const uint64_t key = part_key(A.native_seed, A.part_seed[p]);
  const int64_t idx = qv - A.part_base[p];
  for (int i = 0; i < A.words; ++i) bm[i * 64] = 0u;
  CtrRng rng(key, idx, kStreamMask);
  for (int32_t s = 0; __builtin_amdgcn_ballot_w64(s < num); ++s) {
    const uint32_t u = rng.u32();
    if (s < num) {
      const uint32_t j = (uint32_t)(nc - num + s);
      const uint32_t t = lemire_below(u, j + 1u, rng);
      const uint32_t wt = bm[(t >> 5) * 64];
      const uint32_t pick = (wt >> (t & 31)) & 1u ? j : t;
      bm[(pick >> 5) * 64] |= 1u << (pick & 31);
    }
  }
  CtrRng drng(key, idx, kStreamDecide);
  const bool fast = nc == na + nb;
  int32_t wi = 0, tcur = 0, ccur = 0;  // bitmap word; slow path: token / candidate cursor
  uint32_t bits = num > 0 ? bm[0] : 0u;
  for (int32_t m = 0; __builtin_amdgcn_ballot_w64(m < num); ++m) {
    const uint32_t x = drng.u32(), y = drng.u32();
    if (m < num) {
      while (bits == 0u) bits = bm[++wi * 64];
      const int32_t ci = wi * 32 + __ffs(bits) - 1;
      bits &= bits - 1u;
      int32_t t = ci;
      if (!fast) {  // walk to the ci-th non-[CLS]/[SEP] token
        while (true) {
          const int32_t tok = tcur < na ? win_token(A, d.a_ks, d.a_front, tcur)
                                        : win_token(A, d.b_ks, d.b_front, tcur - na);
          if (tok != A.cls_id && tok != A.sep_id) {
            if (ccur == ci) break;
            ++ccur;
          }
          ++tcur;
        }
        t = tcur++;
        ++ccur;
      }
      const int32_t tok = x < kNat80 ? A.mask_id
                          : x < kNat90 ? kKeep
                                       : (int32_t)lemire_below(y, (uint32_t)A.vocab_size, drng);
      spos[mb + m] = (uint16_t)(t < na ? t + 1 : t + 2);
      stok[mb + m] = tok;
    }
  }
  wave_sync();
  for (int32_t i = lane; i < mend; i += 64) {
    A.mpos[m0 + i] = spos[i];
    A.mtok[m0 + i] = stok[i];
  }
}

// ---------------------------------------------------------------------------------------------
// Whole-word static masking (lddl_pair_params::whole_word): Google BERT's
// create_masked_lm_predictions with do_whole_word_mask on the native streams. The reference has
// no such mode, so it exists with LDDL_RNG_NATIVE only.
// ---------------------------------------------------------------------------------------------
// streams of the whole-word path (CtrRng keeps 4 bits for the stream id)
enum : uint32_t { kStreamWordKey = 5, kStreamWordDecide = 6 };

// The draws that belong to token t of a pair: Philox blocks (t << 16) + 0, 1, .. of the pair's
// stream (t < 65536: check_plan_args bounds seq), so no two tokens share a block.
__device__ inline CtrRng token_rng(uint64_t key, int64_t pair_index, uint32_t stream, int32_t t) {
  CtrRng r(key, pair_index, stream);
  r.blk = (uint32_t)t << 16;
  return r;
}

// Minimum of v over the 64 lanes (all lanes active), wave-uniform: an inclusive min-scan with the
// DPP steps of wave_incl_scan (a lane without a source keeps its own value), read from lane 63.
template <int kCtrl, int kRowMask>
__device__ inline uint32_t min_step(uint32_t v) {
  const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, kCtrl, kRowMask, 0xF, false);
  return o < v ? o : v;
}
__device__ inline uint32_t wave_min_u32(uint32_t v) {
  v = min_step<0x111, 0xF>(v);  // row_shr:1
  v = min_step<0x112, 0xF>(v);  // row_shr:2
  v = min_step<0x114, 0xF>(v);  // row_shr:4
  v = min_step<0x118, 0xF>(v);  // row_shr:8
  v = min_step<0x142, 0xA>(v);  // row_bcast:15 -> rows 1, 3
  v = min_step<0x143, 0xC>(v);  // row_bcast:31 -> rows 2, 3
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// smallest entry of the lane's column (tokens wi * 64 + lane) among the windows in `cand`
__device__ inline uint64_t column_min(const uint64_t* kk, uint64_t cand, int lane) {
  uint64_t best = ~0ull;
  for (uint64_t c = cand; c; c &= c - 1) {
    const uint64_t v = kk[(__ffsll((unsigned long long)c) - 1) * 64 + lane];
    best = v < best ? v : best;
  }
  return best;
}

// One wave per pair, lane = token of a 64-token window. The budget is the plain path's num
// (nmask[q], from plan_native_kernel<true>); the pool is laid out by it (moff) and the number of
// positions actually masked is written back to nmask[q] (<= the budget, possibly 0), which is what
// pair_prep_kernel and the gather then read.
//  1. tokens loaded coalesced; per window the ballots of literal [CLS]/[SEP] and of word starts
//     (a token that is no continuation; tokens past the pair count as starts), the special flag
//     of a window's last token carried into the next; one Philox key per head, entry
//     key << 32 | token << 16 | word length in the lane's LDS column;
//  2. the greedy walk of the shuffled word order as a repeated wave-wide select-min over the
//     entries not yet visited: every lane keeps its column's smallest entry, a 32-bit DPP minimum
//     of the keys and a ballot name the winner, i.e. the words come in (key, lane, window) order
//     (two of W words share a key in W^2 / 2^33 of the pairs, 1e-5 at seq 512); a word is taken
//     iff it still fits; only the winner's lane rescans its column;
//  3. lane w holds the masked bits of window w: ranks by popcount, sorted positions, and an
//     80/10/10 decision per masked token from the token's own Philox block.
// Every cross-lane step (ballots, DPP minimum) is reached by all 64 lanes: the loops run on
// wave-uniform bounds and tails are predicated.
__global__ void __launch_bounds__(256) mask_ww_native_kernel(NativeArgs A, ContBits C, int32_t seqp) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_ww[];
  const int w = wave_id(), lane = threadIdx.x & 63, nwv = blockDim.x >> 6;
  const int64_t q = (int64_t)blockIdx.x * nwv + w;
  if (q >= A.n_pairs) return;
  const int32_t wcap = seqp >> 6;  // windows of the longest pair
  uint64_t* kk = reinterpret_cast<uint64_t*>(s_ww) + (size_t)w * (seqp + wcap + 1);  // [seqp]
  uint64_t* sbits = kk + seqp;  // [wcap + 1] word-start ballots, then the masked bits, per window
  const PairDesc d = A.desc[q];
  const int32_t na = __builtin_amdgcn_readfirstlane(d.na);
  const int32_t n = __builtin_amdgcn_readfirstlane(min(d.na + (d.nb_rn & 0x7FFFFFFF), seqp));
  const int32_t nwin = (n + 63) >> 6;
  const int32_t budget = __builtin_amdgcn_readfirstlane(A.nmask[q]);
  const int64_t p = A.ppart[q];
  const uint64_t key = part_key(A.native_seed, A.part_seed[p]);
  const int64_t idx = q - A.part_base[p];
  const int64_t a0 = A.kscan[d.a_ks] + d.a_front, b0 = A.kscan[d.b_ks] + d.b_front - na;
  bool carry = false;   // the token before the window is a literal special
  uint64_t cand = 0;    // bit wi: token wi * 64 + lane is a head not yet visited
  for (int32_t wi = 0; wi < nwin; ++wi) {
    const int32_t t = wi * 64 + lane;
    const bool in = t < n;
    const int32_t id = in ? A.dense.ld((t < na ? a0 : b0) + t) : 0;
    const bool special = in && (id == A.cls_id || id == A.sep_id);
    const uint64_t sp = ballot(special);
    const bool prev_special = lane ? ((sp >> (lane - 1)) & 1) != 0 : carry;
    carry = (sp >> 63) != 0;
    const bool cont = in && !special && t != 0 && t != na && !prev_special && cont_id(C, id);
    const uint64_t st = ballot(!cont);
    if (lane == 0) sbits[wi] = st;
    if (in && !special && !cont) {
      CtrRng r = token_rng(key, idx, kStreamWordKey, t);
      kk[t] = ((uint64_t)r.u32() << 32) | ((uint64_t)t << 16);
      cand |= 1ull << wi;
    }
  }
  if (lane == 0) sbits[nwin] = ~0ull;  // (a pair that fills its last window: the word ends there)
  wave_sync();
  // word lengths: the distance to the next start
  for (uint64_t c = cand; c; c &= c - 1) {
    const int32_t wi = __ffsll((unsigned long long)c) - 1;
    uint64_t m = lane < 63 ? sbits[wi] >> (lane + 1) : 0ull;
    int32_t len = __ffsll((unsigned long long)m);
    if (!m) {
      int32_t w2 = wi + 1;
      while (!(m = sbits[w2])) ++w2;  // (ends at sbits[nwin] at the latest)
      len = 64 - lane + 64 * (w2 - wi - 1) + __ffsll((unsigned long long)m) - 1;
    }
    kk[wi * 64 + lane] |= (uint64_t)(uint32_t)len;
  }
  uint64_t best = column_min(kk, cand, lane);
  uint64_t mb = 0;  // lane wi: masked tokens of window wi
  int32_t masked = 0;
  while (masked < budget) {
    // the smallest key; among the lanes that hold it (nearly always one) the lowest wins
    const uint32_t kmin = wave_min_u32((uint32_t)(best >> 32));
    const uint64_t win = ballot(cand != 0 && (uint32_t)(best >> 32) == kmin);
    if (!win) break;  // every word visited
    const int wl = __ffsll((unsigned long long)win) - 1;
    const uint32_t sel = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)best, wl);
    const int32_t h = (int32_t)(sel >> 16), len = (int32_t)(sel & 0xFFFF);
    if (masked + len <= budget) {
      masked += len;
      const int32_t lo = max(h - 64 * lane, 0), hi = min(h + len - 64 * lane, 64);
      if (lo < hi) mb |= (hi - lo == 64 ? ~0ull : (1ull << (hi - lo)) - 1) << lo;
    }
    if (lane == wl) {
      cand &= ~(1ull << (h >> 6));
      best = column_min(kk, cand, lane);
    }
  }
  wave_sync();  // (the start ballots are read; their slots take the masked bits)
  if (lane < nwin) sbits[lane] = mb;
  wave_sync();
  const int64_t m0 = A.moff[q];
  int32_t base = 0;
  for (int32_t wi = 0; wi < nwin; ++wi) {
    const uint64_t m = sbits[wi];
    if ((m >> lane) & 1) {
      const int32_t t = wi * 64 + lane;
      const int64_t at = m0 + base + (int32_t)popc_below(m);
      CtrRng drng = token_rng(key, idx, kStreamWordDecide, t);
      const uint32_t x = drng.u32(), y = drng.u32();
      A.mpos[at] = (uint16_t)(t < na ? t + 1 : t + 2);
      A.mtok[at] = x < kNat80 ? A.mask_id
                   : x < kNat90 ? kKeep
                                : (int32_t)lemire_below(y, (uint32_t)A.vocab_size, drng);
    }
    base += __popcll(m);
  }
  if (lane == 0) A.nmask[q] = base;
}

// random.shuffle(partition_pairs), native: output row k of partition p takes pair perm_p(k), a
// keyed 4-round Feistel bijection on [0, 4^h) >= np restricted to [0, np) by cycle walking.
__global__ void __launch_bounds__(256) order_native_kernel(NativeArgs A) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= A.n_pairs) return;
  const int64_t p = A.ppart[q];
  const int64_t pb = A.part_base[p], np = A.part_base[p + 1] - pb;
  const uint64_t key = mix64(part_key(A.native_seed, A.part_seed[p]) ^ kStreamOrder);
  int bits = 1;
  while ((1ll << bits) < np) ++bits;
  const int h = (bits + 1) >> 1;
  const uint64_t hm = (1ull << h) - 1;
  uint64_t x = (uint64_t)(q - pb);
  do {
    uint64_t L = x >> h, R = x & hm;
    for (uint64_t rd = 0; rd < 4; ++rd) {
      const uint64_t f = mix64(R ^ key ^ (rd << 56)) & hm;
      const uint64_t nl = R;
      R = L ^ f;
      L = nl;
    }
    x = (L << h) | R;
  } while (x >= (uint64_t)np);
  A.src[q] = pb + (int64_t)x;
}


// The final per-partition Fisher-Yates swaps (draws from plan_replay_kernel) for partitions too
// large for shuffle_sort_kernel's LDS tables (more than min_np pairs): one lane swaps in global
// memory.

__global__ void __launch_bounds__(64) apply_shuffle_kernel(const int64_t* kd_off, const int64_t* kp_off,
                                                          int32_t dup, const int64_t* part_npairs,
                                                          const int32_t* jseq, int32_t* order,
                                                          int64_t min_np) {
  const int p = blockIdx.x;
  const int64_t base = (int64_t)dup * kd_off[kp_off[p]];
  const int64_t np = part_npairs[p];
  if (np <= min_np) return;  // (shuffle_sort_kernel's)
  const int32_t* js = jseq + base;
  int32_t* ord = order + base;
  for (int64_t k = threadIdx.x; k < np; k += 64) ord[k] = (int32_t)k;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int64_t i = np - 1; i > 0; --i) {
      const int32_t j = js[i];
      const int32_t t = ord[i];
      ord[i] = ord[j];
      ord[j] = t;
    }
  }
}

// The same permutation with no sequential chain at all (one workgroup of 1024 per partition of at
// most `cap` pairs; larger ones go to apply_shuffle_kernel). The backward Fisher-Yates
// x[i] <-> x[j_i], i = n-1 .. 1, on x = identity leaves, with succ(i) = the next step k > i that
// drew the same j (j_k = j_i) and first(v) = the first step that drew v:
//   x[i] = succ(i) ? R(succ(i)) : j_i  (i >= 1),   x[0] = first(0) ? R(first(0)) : 0,
// where R(k) follows f(k) = (j_k == k ? succ(k) : first(k)) to the end of its chain (the value
// step k moved out of position k is the one the last earlier-executed step wrote there, and so
// on). succ and first come from a bucket sort of the steps by their draw (LDS counters, a block
// scan, a scatter, then each bucket - a few steps on average - sorted by step), R from pointer
// jumping, everything over 1024 threads. LDS: three 16-bit arrays of n (the draws are read from
// global memory once, coalesced, into the one that later holds f and R).
__device__ inline uint32_t lds_add16(uint32_t* words, uint32_t v) {  // 16-bit counters, packed
  const uint32_t sh = 16u * (v & 1u);
  return (atomicAdd(&words[v >> 1], 1u << sh) >> sh) & 0xFFFFu;
}

constexpr int kShufThreads = 1024;  // one block per CU (its LDS): 16 waves hide the latencies
// The pair maps of map_pairs_kernel, written by the partition shuffle's last pass (any may be
// null): src[q] the slot of output pair q, slots[i] the i-th slot in planner order, dstq[i] the
// output position of the i-th pair in planner order; part_base[p] = the partition's first pair.
struct PairMaps {
  const int64_t* part_base;
  int64_t *src, *slots, *dstq;
};

__global__ void __launch_bounds__(kShufThreads) shuffle_sort_kernel(const int64_t* kd_off, const int64_t* kp_off,
                                                          int32_t dup, const int64_t* part_npairs,
                                                          const int32_t* __restrict__ jseq,
                                                          int32_t* __restrict__ order, int32_t cap,
                                                          PairMaps M) {
  extern __shared__ __attribute__((aligned(16))) uint8_t ss_smem[];
  const int p = blockIdx.x;
  const int32_t n = (int32_t)part_npairs[p];
  if (n > cap) return;  // (apply_shuffle_kernel's)
  const int32_t capw = (cap + 2) & ~1;
  uint32_t* cntw = reinterpret_cast<uint32_t*>(ss_smem);        // bucket counters -> ends
  uint16_t* cnt = reinterpret_cast<uint16_t*>(ss_smem);
  uint16_t* srt = reinterpret_cast<uint16_t*>(ss_smem) + capw;  // steps by bucket
  uint16_t* r = srt + capw;                                     // j, then f, then R
  const int64_t base = (int64_t)dup * kd_off[kp_off[p]];
  const int32_t* __restrict__ js = jseq + base;
  // succ(i) (or ~j_i when step i is the last to draw j_i), then the permutation
  int32_t* __restrict__ ord = order + base;
  const int tid = threadIdx.x;
  for (int32_t w = tid; w < capw / 2; w += kShufThreads) cntw[w] = 0u;
  for (int32_t i = tid; i < n; i += kShufThreads) r[i] = (uint16_t)js[i];
  __syncthreads();
  for (int32_t i = 1 + tid; i < n; i += kShufThreads) (void)lds_add16(cntw, r[i]);
  __syncthreads();
  {  // exclusive scan of the counts: a run per thread, then the runs' sums
    __shared__ int32_t s_w[kShufThreads / 64];
    const int32_t per = (n + kShufThreads - 1) / kShufThreads;
    const int32_t x0 = tid * per, x1 = min(x0 + per, n);
    int32_t run = 0;
    for (int32_t x = x0; x < x1; ++x) run += cnt[x];
    const int32_t inc = wave_incl_scan(run);
    if ((tid & 63) == 63) s_w[tid >> 6] = inc;
    __syncthreads();
    int32_t off = inc - run;
    for (int w = 0; w < (tid >> 6); ++w) off += s_w[w];
    for (int32_t x = x0; x < x1; ++x) {
      const int32_t c = cnt[x];
      cnt[x] = (uint16_t)off;
      off += c;
    }
  }
  __syncthreads();
  for (int32_t i = 1 + tid; i < n; i += kShufThreads) srt[lds_add16(cntw, r[i])] = (uint16_t)i;
  __syncthreads();  // cnt[v] = the end of bucket v now
  // each bucket sorted by step (insertion sort: a few entries), succ along it
  for (int32_t v = tid; v < n; v += kShufThreads) {
    const int32_t lo = v ? cnt[v - 1] : 0, hi = cnt[v];
    for (int32_t m = lo + 1; m < hi; ++m) {
      const uint16_t e = srt[m];
      int32_t y = m - 1;
      while (y >= lo && srt[y] > e) {
        srt[y + 1] = srt[y];
        --y;
      }
      srt[y + 1] = e;
    }
    for (int32_t m = lo; m < hi; ++m) ord[srt[m]] = m + 1 < hi ? (int32_t)srt[m + 1] : ~v;
  }
  __syncthreads();
  // f(k) = j_k == k ? succ(k) : first(k); R(k) = k at a chain's end (each thread reads the
  // draws it overwrites)
  for (int32_t k = tid; k < n; k += kShufThreads) {
    int32_t f = -1;
    if (k > 0) {
      if (r[k] == k) {
        f = ord[k];
      } else {
        const int32_t lo = cnt[k - 1], hi = cnt[k];
        f = lo < hi ? (int32_t)srt[lo] : -1;
      }
    }
    r[k] = (uint16_t)(f < 0 ? k : f);
  }
  __syncthreads();
  for (;;) {  // pointer jumping: R(k) = R(R(k)) until every chain is collapsed
    int changed = 0;
    for (int32_t k = tid; k < n; k += kShufThreads) {
      const uint16_t a = r[k], b = r[a];
      if (b != a) {
        r[k] = b;
        changed = 1;
      }
    }
    if (!__syncthreads_or(changed)) break;
  }
  const int32_t first0 = n > 1 && cnt[0] > 0 ? (int32_t)srt[0] : -1;
  const int64_t q0 = M.part_base ? M.part_base[p] : 0;
  for (int32_t k = tid; k < n; k += kShufThreads) {
    const int32_t sc = k == 0 ? first0 : ord[k];
    const int32_t v = sc >= 0 ? (int32_t)r[sc] : (k == 0 ? 0 : ~sc);
    ord[k] = v;
    if (M.src) M.src[q0 + k] = base + v;
    if (M.slots) M.slots[q0 + k] = base + k;
    if (M.dstq) M.dstq[q0 + v] = q0 + k;
  }
}

// ---------------------------------------------------------------------------------------------
// layout + gather
// ---------------------------------------------------------------------------------------------
// src[q]: the planner slot of output pair q (partition shuffle applied); slots[q]: the q-th
// slot in planner order (every partition's slots base .. base + np - 1), so the per-slot passes
// read the slot-indexed arrays front to back instead of in shuffled order.
// (any output may be null)
// dstq[i]: the output position of the i-th pair in planner order (the inverse of src), for the
// mask replay that also writes each pair's gather record.
__global__ void map_pairs_kernel(const int64_t* kd_off, const int64_t* kp_off, int32_t dup,
                                 const int64_t* part_pair_base, const int32_t* order, int64_t* src,
                                 int64_t* slots, int64_t* dstq) {
  const int p = blockIdx.x;
  const int64_t base = (int64_t)dup * kd_off[kp_off[p]];
  const int64_t q0 = part_pair_base[p], n = part_pair_base[p + 1] - q0;
  for (int64_t k = threadIdx.x; k < n; k += blockDim.x) {
    if (src) src[q0 + k] = base + order[base + k];
    if (slots) slots[q0 + k] = base + k;
    if (dstq) dstq[q0 + order[base + k]] = q0 + k;
  }
}

// the largest partition's pair count (the partition shuffle's LDS size)
__global__ void max_pairs_kernel(const int64_t* np, int64_t n, unsigned long long* out) {
  int64_t m = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    m = np[i] > m ? np[i] : m;
  if (m) atomicMax(out, (unsigned long long)m);
}

struct Identity {
  const int64_t* v;
  __device__ int64_t operator()(int64_t i) const { return v[i]; }
};

// Per output pair, everything the gather needs, in output order: the A and B windows in the dense
// token array, the lengths and is_random_next, and the masks' place in the mask pool. Built one
// lane per pair (src -> descriptor -> sentence offsets: every load of a wave in flight at once),
// so the scans and the gather read it front to back instead of chasing src[q] themselves.
struct alignas(16) GatherRec {
  int64_t aoff, boff, moff;
  int32_t na, nb_rn, nm, pad;
};

__global__ void __launch_bounds__(256) pair_prep_kernel(const int64_t* __restrict__ src, int64_t n,
                                                        const PairDesc* __restrict__ desc,
                                                        const int64_t* __restrict__ kscan,
                                                        const int32_t* __restrict__ nmask,
                                                        const int64_t* __restrict__ moff,
                                                        GatherRec* __restrict__ rec,
                                                        int2* __restrict__ cnt) {
  // (XCD-contiguous blocks: a partition's pairs share one L2 for its descriptors and offsets)
  const int64_t q = xcd_block(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
  if (q >= n) return;
  const int64_t slot = src[q];
  const PairDesc d = desc[slot];
  GatherRec r;
  r.aoff = kscan[d.a_ks] + d.a_front;
  r.boff = kscan[d.b_ks] + d.b_front;
  // masks: the native path's arrays (none: no masking; the replay path's records come from
  // fy_resolve_kernel)
  r.moff = nmask ? moff[slot] : 0;
  r.na = d.na;
  r.nb_rn = d.nb_rn;
  r.nm = nmask ? nmask[slot] : 0;
  r.pad = 0;
  rec[q] = r;
  cnt[q] = make_int2(r.na + (r.nb_rn & 0x7FFFFFFF), r.nm);  // compact input of the two scans
}

struct PairTokens {
  const int2* c;
  __device__ int64_t operator()(int64_t q) const { return c[q].x; }
};
struct PairCounts {  // both, for scan_exclusive2
  const int2* c;
  __device__ Sum2 operator()(int64_t q) const {
    const int2 v = c[q];
    return Sum2{v.x, v.y};
  }
};

// Kept tokens packed densely in kept-sentence order: kept sentence k's pieces are
// dense[kscan[k] .. kscan[k+1]). A pair's A (and B) window is then one contiguous run
// dense[kscan[a_ks] + a_front ..+ na), because a span only ever covers consecutive kept
// sentences of one document. One wave per 64 kept sentences; 64-token output chunks are stored
// coalesced, each lane finding its sentence among the few that overlap the chunk.
__global__ void __launch_bounds__(256) densify_kernel(const int64_t* __restrict__ ks_start,
                                                      const int32_t* __restrict__ ks_len,
                                                      const int64_t* __restrict__ kscan, int64_t n,
                                                      const int32_t* __restrict__ ids,
                                                      IdPtr dense) {
  const int64_t k0 = ((int64_t)blockIdx.x * 4 + wave_id()) * 64;
  if (k0 >= n) return;
  densify_group(k0, ks_start, ks_len, kscan, n, ids, dense);
}

// Split plan: the first kept sentence of the tail range's partitions (= the end of the head's)
// and the kept tokens before it. info[0] bounds the two ranges' dense packing, info[1] scales
// the head's counts to the suggested output capacities.
__global__ void split_info_kernel(const int64_t* kp_off, const int64_t* kd_off, const int64_t* kscan,
                                  int64_t s, int64_t* info) {
  const int64_t k = kd_off[kp_off[s]];
  info[0] = k;
  info[1] = kscan[k];
}

// densify_kernel over kept sentences [0, *n_ptr): the head range of a split plan (the launch
// covers all kept sentences; the workgroups past the bound leave at once)
__global__ void __launch_bounds__(256) densify_head_kernel(const int64_t* __restrict__ ks_start,
                                                           const int32_t* __restrict__ ks_len,
                                                           const int64_t* __restrict__ kscan,
                                                           const int64_t* __restrict__ n_ptr,
                                                           const int32_t* __restrict__ ids,
                                                           IdPtr dense) {
  const int64_t n = *n_ptr;
  const int64_t k0 = ((int64_t)blockIdx.x * 4 + wave_id()) * 64;
  if (k0 >= n) return;
  densify_group(k0, ks_start, ks_len, kscan, n, ids, dense);
}

// part_base[s + 1 + i] = head_pairs + rel[i + 1], i in [0, n): the tail range's partitions in
// the plan's one table of first output pairs (part_base[s] = head_pairs came with the head)
__global__ void tail_part_base_kernel(const int64_t* rel, int64_t n, int64_t head_pairs,
                                      int64_t* part_base_s) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) part_base_s[1 + i] = head_pairs + rel[i + 1];
}


struct GatherArgs {
  const void* dense;     // kept tokens, packed (IdT)
  const GatherRec* rec;  // per output pair (pair_prep_kernel)
  // masks: positions + replacements at rec.moff (any order; ranks are taken from the bitmap)
  const uint16_t* mpos;
  const int32_t* mtok;
  int32_t masking;
  // one launch gathers one range of output pairs: q counts from the range's first pair, rec /
  // tok_off / pos_off are the range's tables (offsets relative to its first token / mask) and
  // tok_base / pos_base the tokens / masks of the pairs before it; len_a, is_rn and the offset
  // copies point at the range's first pair
  int64_t n_pairs;
  const int64_t* tok_off;
  const int64_t* pos_off;
  int64_t tok_base, pos_base;
  void* out_tok;  // IdT
  int32_t* len_a;
  uint8_t* is_rn;
  uint16_t* out_pos;
  void* out_lab;  // IdT
  int64_t* out_tok_off;  // the caller's copies of tok_off / pos_off (may be null)
  int64_t* out_pos_off;
};

constexpr int kMaxSeqGather = 4096;
constexpr int kGWaves = 4;

// LDS of the gather per pair in flight: the decision table indexed by output token x (seqp =
// seq rounded up to 128 entries of int32, kNoMask where x is not masked) and the staging rows
// of one pass's masked positions and labels by rank (128 each, then one trash entry per lane).
constexpr int32_t kNoMask = INT32_MIN;
constexpr int kStageRows = 128;  // + 32 trash entries, one per lane of the half-wave
struct GatherLds {
  int32_t seqp;
  int32_t ib;  // bytes per label id (the staging row's width)
  int32_t db;  // bytes per decision-table entry: 4 (int32), 2 in gather16_kernel (16-bit ids)
  __host__ __device__ size_t per_pair() const {
    return (size_t)db * seqp + (size_t)(kStageRows + 32) * (size_t)(2 + ib);
  }
};
// gather16_kernel's 16-bit decision table: a token id, or one of two values no id takes (the
// context uses 2-byte ids only for vocabs of <= 65,534 entries)
constexpr uint16_t kNoMask16 = 0xFFFFu, kKeep16 = 0xFFFEu;

// Replay masks, off the planner's sequential chain: one LANE per pair replays the recorded swaps
// of random.shuffle(cand_indexes) (draws j_i, i = nc-1 .. 1) on a lane-private LDS column and
// writes the candidates that end in slots 0 .. num-1, as positions of [CLS] A [SEP] B [SEP], in
// slot order (= the order of the planner's decisions) over the mask pool. Steps i >= num only
// move x[i] to x[j_i] (slot i is never read again); steps i < num finalise slot i = x[j_i].
// Column layout x[k * 64 + lane] keeps the 64 lanes' accesses in distinct banks.
struct ResolveArgs {
  const int64_t* src;  // slots in planner order (each pair once; mpos is addressed by moff)
  int64_t n_pairs;
  const PairDesc* desc;
  const SlotPool* spool;
  const void* jpool;   // 1- or 2-byte draws (the kernel's D)
  uint16_t* mpos;
  const int64_t* kscan;
  IdPtr dense;
  int32_t cls_id, sep_id;
  // with masking on the replay path, the pair's gather record and scan counts are written here
  // too, at its output position dstq[i] (what pair_prep_kernel does for the other paths: the
  // descriptor and slot record are already in registers, and planner order reads them front to
  // back); null otherwise
  const int64_t* dstq;
  GatherRec* rec;
  int2* cnt;
  int32_t col_rows;  // entries per lane column in LDS (seq rounded up to 16)
};

// A lane's column of LDS entries; 16-bit: x[k * LW + lane]; 8-bit (seq <= 256): dword k/4 of
// lane l at (k/4) * LW + l, so every access of the wave hits distinct banks either way.
template <typename T, int LW>
struct LaneCol;
template <int LW>
struct LaneCol<uint16_t, LW> {
  uint16_t* base;
  int lane;
  __device__ uint32_t get(int k) const { return base[k * LW + lane]; }
  __device__ void set(int k, uint32_t v) { base[k * LW + lane] = (uint16_t)v; }
  __device__ void iota(int n) {
    for (int k = 0; k < n; ++k) set(k, (uint32_t)k);
  }
};
template <int LW>
struct LaneCol<uint8_t, LW> {
  uint8_t* base;
  int lane;
  __device__ int at(int k) const { return ((k >> 2) * (4 * LW)) | (lane << 2) | (k & 3); }
  __device__ uint32_t get(int k) const { return base[at(k)]; }
  __device__ void set(int k, uint32_t v) { base[at(k)] = (uint8_t)v; }
  __device__ void iota(int n) {
    uint32_t* w = reinterpret_cast<uint32_t*>(base);
    for (int k = 0; k < n; k += 4)
      w[(k >> 2) * LW + lane] = (uint32_t)k | (uint32_t)(k + 1) << 8 | (uint32_t)(k + 2) << 16 |
                                (uint32_t)(k + 3) << 24;
  }
};

// D: draw type (uint8_t for target_seq_length <= 256, else uint16_t); a uint4 holds 16 / sizeof(D)
// draws. NG > 0: all of a pair's draws (nc <= NG * 16 / sizeof(D)) are loaded up front, NG uint4
// in flight per lane.
// LW: pairs (lanes) per workgroup of one wave. Long pairs run with LW < 64: a lane's column is
// seq entries, so at seq 512 a full wave holds 64 KB of LDS and only two fit a CU; fewer lanes
// per wave put more waves (more independent step chains) on each SIMD.
template <typename T, typename D, int NG, int LW = 64, bool kBF = false, int kRA = 0, int kPf = 4>
__global__ void __launch_bounds__(64) fy_resolve_kernel(ResolveArgs R) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_xb[];
  constexpr int kPerVec = 16 / (int)sizeof(D);  // draws per uint4
  const int lane = threadIdx.x;
  LaneCol<T, LW> x{reinterpret_cast<T*>(s_xb), lane};
  // (XCD-contiguous blocks: a partition's pairs, their kept-sentence offsets and records meet
  // in one L2)
  const int64_t q = xcd_block(blockIdx.x, gridDim.x) * LW + lane;
  // 16-bit columns, branch-free steps: the workgroup writes the identity into every column at
  // once, 8 rows (one entry per lane and row) per 16-byte store per lane, before any lane leaves
  // (a lane's own per-entry iota was ~20 % of the kernel's LDS instructions and half its scalar
  // ones; C3 profiles/r05n_*). Rows past a lane's nc are only touched by its padding steps.
  constexpr bool kCoopIota = kBF && sizeof(T) == 2 && LW == 16;
  if constexpr (kCoopIota) {
    const int rows = (int)(R.col_rows);
    uint4* base = reinterpret_cast<uint4*>(s_xb);
    for (int k0 = 0; k0 < rows; k0 += 8) {
      const uint32_t k = (uint32_t)(k0 + (lane >> 1)), kk = k | k << 16;
      base[2 * k + (lane & 1)] = make_uint4(kk, kk, kk, kk);  // row k = 32 bytes = 2 uint4
    }
    // lanes wrote rows of other lanes' columns: order the fill before any lane reads its own
    // column (a one-wave workgroup: the barrier is a wait on the LDS stores)
    __syncthreads();
  }
  if (q >= R.n_pairs) return;
  const int64_t slot = R.src[q];
  const int64_t oq = R.dstq ? R.dstq[q] : 0;
  // the whole 16-byte record and the descriptor in one round trip (a member-wise read split the
  // record around the early exit below)
  const uint4 spv = *reinterpret_cast<const uint4*>(R.spool + slot);
  const PairDesc d = R.desc[slot];
  const SlotPool sp{spv.x, spv.y, (int32_t)spv.z, (int32_t)spv.w};
  const int32_t num = sp.nmask;
  const int32_t nc = num > 0 ? sp.ncand : 0;  // (no early exit: it split the loads above)
  const int64_t jb = (int64_t)sp.joff16 << 4, mb = (int64_t)sp.moff8 << 3;
  const int32_t na = d.na, nb = d.nb_rn & 0x7FFFFFFF;
  const bool fast = nc == na + nb;
  const int64_t ao = R.kscan[d.a_ks] + d.a_front, bo = R.kscan[d.b_ks] + d.b_front;
  const uint4* jp = reinterpret_cast<const uint4*>(static_cast<const D*>(R.jpool) + jb);
  uint4* mp = reinterpret_cast<uint4*>(R.mpos + mb);
  uint4 acc = make_uint4(0u, 0u, 0u, 0u);  // slots [8h, 8h+8) collected from the top down
  // steps [8h, 8h+8): swap, or (i < num) finalise slot i; w = the two (1-byte draws) or four
  // (2-byte draws) dwords holding their draws
  auto group = [&](int h, const uint32_t* w) {
#pragma unroll
    for (int u = 7; u >= 0; --u) {
      const int i = 8 * h + u;
      if (i >= nc) continue;
      const int j = sizeof(D) == 1 ? (int)((w[u >> 2] >> (8 * (u & 3))) & 0xFFu)
                                   : (int)((w[u >> 1] >> (16 * (u & 1))) & 0xFFFFu);
      const uint32_t xi = x.get(i);
      if (i >= num) {
        if (i >= 1) x.set(j, xi);
      } else {
        const int y = i >= 1 ? (int)x.get(j) : (int)xi;  // slot 0 keeps x[0]
        if (i >= 1) x.set(j, xi);
        const uint32_t pos = (uint32_t)(fast ? (y < na ? y + 1 : y + 2) : y);
        // 128-bit shift register, newest at slot offset 0 (slots arrive in descending order)
        acc = make_uint4((acc.x << 16) | pos, (acc.y << 16) | (acc.x >> 16),
                         (acc.z << 16) | (acc.y >> 16), (acc.w << 16) | (acc.z >> 16));
      }
    }
    if (8 * h < num) mp[h] = acc;  // slots [8h, 8h+8) complete (the top group zero-padded)
  };
  // kBF: the same steps without exec-mask branches. The planner pads a pair's draw region
  // ([nc, nc rounded up to 16) hold j_i = i) and step 0 takes j = 0 (entry 0 of the region is
  // never a draw), so every step of a loaded vector is x[j] = x[i] unguarded (a padding step
  // rewrites x[i] onto itself); a group in which no
  // lane of the wave finalises a slot is that move alone (read, wait, write: ~2 VALU per
  // step); otherwise each step also reads y = x[j] before the write (i = 0: j = 0, y = x[0])
  // and keeps its position by select. Round 4's guarded steps spent ~10 scalar exec-mask
  // instructions and three branches per step.
  const int32_t padd = fast ? 1 : 0, thr = fast ? na : INT32_MAX;  // pos = y + padd + (y >= thr)
  // draw u of a group (step 8h + u); step 0 has none: j_0 = 0
  auto draw = [&](int h, const uint32_t* w, int u) -> int {
    const int j = sizeof(D) == 1 ? (int)((w[u >> 2] >> (8 * (u & 3))) & 0xFFu)
                                 : (int)((w[u >> 1] >> (16 * (u & 1))) & 0xFFFFu);
    return u == 0 && h == 0 ? 0 : j;
  };
  auto group_bf = [&](int h, const uint32_t* w) {
    if (__any(8 * h < num)) {
      uint32_t pos[8];
#pragma unroll
      for (int u = 7; u >= 0; --u) {
        const int i = 8 * h + u;
        const int j = draw(h, w, u);
        const uint32_t xi = x.get(i);
        const int y = (int)x.get(j);
        x.set(j, xi);
        pos[u] = i < num ? (uint32_t)(y + padd + (y >= thr ? 1 : 0)) : 0u;
      }
      if (8 * h < num)
        mp[h] = make_uint4(pos[0] | pos[1] << 16, pos[2] | pos[3] << 16, pos[4] | pos[5] << 16,
                           pos[6] | pos[7] << 16);
    } else if (kRA == 0) {
#pragma unroll
      for (int u = 7; u >= 0; --u) x.set(draw(h, w, u), x.get(8 * h + u));
    } else {
      // kRA reads ahead: x[i - kRA] is read before step i's write (the group's top kRA entries
      // at its start), so step u's read misses the writes of steps u + 1 .. min(u + kRA, 7),
      // which are forwarded from registers (the most recent wins)
      int jr[8];  // j - 8h: compared with the step offset u
      uint32_t r[8], v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) jr[u] = draw(h, w, u) - 8 * h;
#pragma unroll
      for (int u = 7; u >= 8 - kRA; --u) r[u] = x.get(8 * h + u);
#pragma unroll
      for (int u = 7; u >= 0; --u) {
        if (u - kRA >= 0) r[u - kRA] = x.get(8 * h + u - kRA);
        uint32_t val = r[u];
#pragma unroll
        for (int t = kRA; t >= 1; --t)  // oldest first
          if (u + t <= 7) val = jr[u + t] == u ? v[u + t] : val;
        v[u] = val;
        x.set(jr[u] + 8 * h, val);
      }
    }
  };
  // one uint4 of draws = kPerVec / 8 groups of 8 steps, processed top down
  auto vec = [&](int g, const uint4& v) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    if (kBF) {
      if (sizeof(D) == 1) group_bf(2 * g + 1, w + 2);
      group_bf(sizeof(D) == 1 ? 2 * g : g, w);
    } else if (sizeof(D) == 1) {
      if (16 * g + 8 < nc) group(2 * g + 1, w + 2);
      group(2 * g, w);
    } else {
      group(g, w);
    }
  };
  const int nvec = (nc + kPerVec - 1) / kPerVec;
  if (NG > 0) {
    uint4 jv[NG > 0 ? NG : 1];
#pragma unroll
    for (int g = 0; g < NG; ++g)
      if (g < nvec) jv[g] = jp[g];
    if (!kCoopIota) x.iota(nc);  // (after the draws' loads are issued)
#pragma unroll
    for (int g = NG - 1; g >= 0; --g)
      if (g < nvec) vec(g, jv[g]);
  } else if (nvec > 0) {  // (a pair without masks has no draws to read)
    // four vectors of draws in flight: one vector ahead left each vector's global load latency
    // exposed every 8 steps (C3, seq 512: 93 -> 77.7 ms; eight ahead 80.1 ms, profiles/r04zj_*,
    // r04zk_*)
    auto ld = [&](int g) { return jp[g < 0 ? 0 : g]; };
    const int top = nvec - 1;
    uint4 rv[kPf];
#pragma unroll
    for (int u = 0; u < kPf; ++u) rv[u] = ld(top - u);
    if (!kCoopIota) x.iota(nc);
    for (int g = top; g >= 0; g -= kPf) {
#pragma unroll
      for (int u = 0; u < kPf; ++u) {
        if (g >= u) vec(g - u, rv[u]);
        rv[u] = ld(g - u - kPf);
      }
    }
  }
  if (R.rec) {
    GatherRec r;
    r.aoff = ao;
    r.boff = bo;
    r.moff = mb;
    r.na = na;
    r.nb_rn = d.nb_rn;
    r.nm = num;
    r.pad = 0;
    R.rec[oq] = r;
    R.cnt[oq] = make_int2(na + nb, num);
  }
  if (!fast && num > 0) {  // literal [CLS]/[SEP] in the pair: candidate index -> position via the tokens
    int k = 0;
    for (int t = 0; t < na + nb; ++t) {
      const int32_t tok = t < na ? R.dense.ld(ao + t) : R.dense.ld(bo + (t - na));
      if (tok != R.cls_id && tok != R.sep_id) x.set(k++, (uint32_t)(t < na ? t + 1 : t + 2));
    }
    uint16_t* m16 = R.mpos + mb;
    for (int c = 0; c < num; ++c) m16[c] = (uint16_t)x.get(m16[c]);
  }
}

// Gather: each half-wave emits K output pairs, 4 consecutive tokens per lane (128 per pass), so
// a wave has 2K pairs in flight with all their parameters in vector registers. Per pair:
// A = dense[kscan[a_ks] + a_front ..+ na), B likewise; output token x < na + nb comes from A
// (x < na, position x + 1) or B (position x + 2); a lane's 4 tokens are one 8- or 16-byte load
// and one non-temporal store except where they straddle A/B or the end. The pair's masks (pool,
// any order) fill a per-pair LDS decision table indexed by x (one plain LDS store per mask);
// each lane reads its 4 entries with one 16-byte LDS load. A masked token's rank (its place in
// the position-sorted masked_lm_positions / labels) is the half-wave's exclusive scan of the
// lanes' masked counts (one DPP scan for all K pairs, counts packed 16 bits apart) plus the
// masked elements before it in the lane; (position, label) go to an LDS staging row by rank and
// leave as two coalesced stores per pass (round 3 issued eight lane-masked 2-byte stores per
// pass from four ballots per element: that mask path was half the kernel, profiles/r04t_*).
// The caller's tok_off / pos_off are written here too (no device-to-device copies).
// 4 consecutive token ids (one lane's share of a pass): 16 bytes of int32 ids, 8 of uint16 ids
template <typename IdT>
struct Tok4;
template <>
struct Tok4<int32_t> {
  typedef int32_t type __attribute__((ext_vector_type(4), aligned(4)));
};
template <>
struct Tok4<uint16_t> {
  typedef uint16_t type __attribute__((ext_vector_type(4), aligned(2)));
};
// The raw load of 4 ids, and the blend "element e from A iff e < ra" (ra = A elements left)
__device__ inline uint2 blend4(uint2 a, uint2 b, int32_t ra) {
  const int32_t bits = ra <= 0 ? 0 : ra >= 4 ? 64 : 16 * ra;
  const uint32_t mlo = bits >= 32 ? ~0u : (1u << bits) - 1u;
  const uint32_t mhi = bits >= 64 ? ~0u : bits <= 32 ? 0u : (1u << (bits - 32)) - 1u;
  return make_uint2((a.x & mlo) | (b.x & ~mlo), (a.y & mhi) | (b.y & ~mhi));
}
__device__ inline int4 blend4(int4 a, int4 b, int32_t ra) {
  return make_int4(0 < ra ? a.x : b.x, 1 < ra ? a.y : b.y, 2 < ra ? a.z : b.z, 3 < ra ? a.w : b.w);
}
template <typename IdT>
using Raw4 = std::conditional_t<sizeof(IdT) == 2, uint2, int4>;

template <int K, typename IdT>
__global__ void __launch_bounds__(64 * kGWaves, 1) gather_kernel(GatherArgs G, GatherLds Lg) {
  static_assert(K == 1 || K == 2, "masked counts of K pairs are packed 16 bits apart");
  using tok4_t = typename Tok4<IdT>::type;
  const IdT* __restrict__ dense = static_cast<const IdT*>(G.dense);
  extern __shared__ __attribute__((aligned(16))) uint8_t g_smem[];
  const int w = wave_id(), lane = threadIdx.x & 63, h = lane >> 5, sl = lane & 31;
  // XCD-contiguous blocks: the pairs of one partition (which read its dense tokens dup times over)
  // and their mask pool lines meet in one L2
  const int64_t wg = xcd_block((int64_t)blockIdx.y * gridDim.x + blockIdx.x, (int64_t)gridDim.x * gridDim.y);
  const int64_t q0 = (wg * kGWaves + w) * 2 * K;  // pairs q0 + 2k + h

  int64_t tof[K], aoff[K], boff[K], po[K], mb[K];
  int32_t na[K], nb[K], rk[K], nm[K];
  int32_t* dec[K];
  uint16_t* spos[K];
  IdT* slab[K];
  GatherRec rc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {  // every pair's loads in flight before any is used
    const int64_t q = q0 + 2 * k + h;
    const bool act = q < G.n_pairs;
    rc[k] = act ? G.rec[q] : GatherRec{0, 0, 0, 0, 0, 0, 0};
    tof[k] = act ? G.tok_base + G.tok_off[q] : 0;
    po[k] = (G.masking && act) ? G.pos_base + G.pos_off[q] : 0;
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int64_t q = q0 + 2 * k + h;
    const GatherRec& r = rc[k];
    na[k] = r.na;
    nb[k] = r.nb_rn & 0x7FFFFFFF;
    aoff[k] = r.aoff;
    boff[k] = r.boff;
    mb[k] = r.moff;
    nm[k] = G.masking ? r.nm : 0;
    rk[k] = 0;
    uint8_t* pb = g_smem + (((size_t)w * K + k) * 2 + h) * Lg.per_pair();
    dec[k] = reinterpret_cast<int32_t*>(pb);
    spos[k] = reinterpret_cast<uint16_t*>(pb + 4 * (size_t)Lg.seqp);
    slab[k] = reinterpret_cast<IdT*>(pb + 4 * (size_t)Lg.seqp + 2 * (kStageRows + 32));
    if (sl == 0 && q < G.n_pairs) {
      G.len_a[q] = na[k];
      G.is_rn[q] = (uint8_t)((uint32_t)r.nb_rn >> 31);
      if (G.out_tok_off) {
        G.out_tok_off[q] = tof[k];
        if (q + 1 == G.n_pairs) G.out_tok_off[q + 1] = tof[k] + na[k] + nb[k];
      }
      if (G.out_pos_off && G.masking) {
        G.out_pos_off[q] = po[k];
        if (q + 1 == G.n_pairs) G.out_pos_off[q + 1] = po[k] + nm[k];
      }
    }
  }
  // a lane's 4 tokens: one load from A and one from B, each at the offset of token x in that
  // window (dense is padded by 4 tokens on both sides, so a load overhanging its window stays in
  // bounds); element e comes from A iff x + e < na. Both loads are issued unconditionally (an
  // unneeded one reads the window start) and blended only when the pass needs the tokens: a
  // conditional load made the compiler wait for it inside its branch, before the next pair's
  // loads were issued.
  using raw_t = Raw4<IdT>;
  raw_t ta[K], tb[K];
  auto issue_tokens = [&](int32_t x) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int32_t n = na[k] + nb[k], bx = x - na[k];
      ta[k] = *reinterpret_cast<const raw_t*>(dense + aoff[k] + (x < na[k] ? x : 0));
      tb[k] = *reinterpret_cast<const raw_t*>(dense + boff[k] + (bx >= -3 && x < n ? bx : 0));
    }
  };
  auto finish_tokens = [&](int32_t x, tok4_t* v) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = __builtin_bit_cast(tok4_t, blend4(ta[k], tb[k], na[k] - x));
  };
  tok4_t v[K];
  issue_tokens(4 * sl);  // the first pass's tokens are in flight while the tables fill
  if (G.masking) {
#pragma unroll
    for (int k = 0; k < K; ++k)
      for (int i = 4 * sl; i < Lg.seqp; i += 128)
        *reinterpret_cast<int4*>(dec[k] + i) = make_int4(kNoMask, kNoMask, kNoMask, kNoMask);
    wave_sync();
#pragma unroll
    for (int k = 0; k < K; ++k)
      for (int j = sl; j < nm[k]; j += 32) {
        const int p = G.mpos[mb[k] + j];  // position in [CLS] A [SEP] B [SEP]: never a literal
        dec[k][p <= na[k] ? p - 1 : p - 2] = G.mtok[mb[k] + j];
      }
    wave_sync();
  }
  for (int32_t cb = 0;; cb += 128) {
    const int32_t x = cb + 4 * sl;
    if (cb > 0) issue_tokens(x);
    finish_tokens(x, v);
    bool more = false;
    if (G.masking) {
      int4 d4[K];
      uint32_t m4[K], packed = 0;
#pragma unroll
      for (int k = 0; k < K; ++k) {  // (x < seqp: every pass starts below the longest pair)
        d4[k] = *reinterpret_cast<const int4*>(dec[k] + x);
        m4[k] = (d4[k].x != kNoMask ? 1u : 0u) | (d4[k].y != kNoMask ? 2u : 0u) |
                (d4[k].z != kNoMask ? 4u : 0u) | (d4[k].w != kNoMask ? 8u : 0u);
        packed |= (uint32_t)__popc(m4[k]) << (16 * k);
      }
      // per half-wave exclusive scan of the packed counts (<= 128 per pair and pass)
      const uint32_t inc = wave_incl_scan(packed);
      const uint32_t lo_tot = (uint32_t)__builtin_amdgcn_readlane((int)inc, 31);
      const uint32_t all_tot = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
      const uint32_t excl = inc - packed - (h ? lo_tot : 0u);
      const uint32_t tots = h ? all_tot - lo_tot : lo_tot;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        int32_t r = (int32_t)((excl >> (16 * k)) & 0xFFFFu);
        const int32_t dd[4] = {d4[k].x, d4[k].y, d4[k].z, d4[k].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {  // branch-free: an unmasked element writes the lane's trash entry
          const bool mk = (m4[k] >> e) & 1u;
          const int32_t xe = x + e, at = mk ? r : kStageRows + sl;
          spos[k][at] = (uint16_t)(xe < na[k] ? xe + 1 : xe + 2);
          slab[k][at] = v[k][e];
          v[k][e] = mk && dd[e] != kKeep ? (IdT)dd[e] : v[k][e];
          r += mk ? 1 : 0;
        }
      }
      wave_sync();
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int32_t tot = (int32_t)((tots >> (16 * k)) & 0xFFFFu);
        for (int32_t i = sl; i < tot; i += 32) {
          G.out_pos[po[k] + rk[k] + i] = spos[k][i];
          static_cast<IdT*>(G.out_lab)[po[k] + rk[k] + i] = slab[k][i];
        }
        rk[k] += tot;
      }
      wave_sync();  // (the staging rows are rewritten by the next pass)
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int32_t n = na[k] + nb[k];
      // non-temporal: the output is streamed, never re-read by this step
      IdT* out = static_cast<IdT*>(G.out_tok) + tof[k];
      if (x + 3 < n) {
        __builtin_nontemporal_store(v[k], reinterpret_cast<tok4_t*>(out + x));
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (x + e < n) __builtin_nontemporal_store(v[k][e], out + x + e);
      }
      more |= n > cb + 128;
    }
    if (!ballot(more)) break;
  }
}

typedef uint16_t Tok8 __attribute__((ext_vector_type(8), aligned(2)));
__device__ inline uint4 blend8(uint4 a, uint4 b, int32_t ra) {  // element e from A iff e < ra
  const int32_t bits = ra <= 0 ? 0 : ra >= 8 ? 128 : 16 * ra;
  auto m = [&](int d) -> uint32_t {
    const int32_t t = bits - 32 * d;
    return t >= 32 ? ~0u : t <= 0 ? 0u : (1u << t) - 1u;
  };
  const uint32_t m0 = m(0), m1 = m(1), m2 = m(2), m3 = m(3);
  return make_uint4((a.x & m0) | (b.x & ~m0), (a.y & m1) | (b.y & ~m1), (a.z & m2) | (b.z & ~m2),
                    (a.w & m3) | (b.w & ~m3));
}

// The gather for 16-bit ids: LP = 16 or 8 lanes per output pair (4 or 8 pairs per wave), 128 / LP
// consecutive tokens per lane (16-byte loads from A and B, 16-byte non-temporal stores). Against
// gather_kernel<2, uint16_t> (a half-wave per pair, 4 tokens per lane, two pairs per lane) a pair
// costs fewer lanes and a lane holds one pair's registers, so more pairs are in flight per SIMD
// while the per-wave load chain (record -> tokens and masks -> stores) stays the same: 33.3 ->
// 29.5 ms per 10 GB step at LP = 16 (profiles/r04zd_*); LP = 8 needs 95 VGPRs and 37 KB of LDS
// per 4-wave block, runs at 4 waves/SIMD and took 35.3 ms (r04ze). The mask path is the same
// decision table by output token (16-byte LDS reads), ranks from an LP-lane DPP scan of the
// lanes' masked counts, and staged coalesced stores.
template <int LP>
struct G16 {
  static constexpr int kNT = 128 / LP;  // tokens per lane per pass
  static constexpr int kNV = kNT / 8;   // 16-byte vectors per lane
};

// inclusive scan of v over LP-lane segments (LP = 8 or 16) and the segment's total
template <int LP>
__device__ inline uint32_t seg_scan(uint32_t v, int lane, uint32_t* tot) {
  uint32_t inc = v;  // 16-lane row scan (row_shr 1, 2, 4, 8)
  inc = scan_step<0x111, 0xF, true>(inc);
  inc = scan_step<0x112, 0xF, true>(inc);
  inc = scan_step<0x114, 0xF, true>(inc);
  inc = scan_step<0x118, 0xF, true>(inc);
  const uint32_t r15 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x15F, 0xF, 0xF, false);  // row_share:15
  if (LP == 16) {
    *tot = r15;
    return inc;
  }
  const uint32_t r7 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x157, 0xF, 0xF, false);  // row_share:7
  const bool hi = (lane & 8) != 0;
  *tot = hi ? r15 - r7 : r7;
  return hi ? inc - r7 : inc;
}

template <int LP>
__global__ void __launch_bounds__(64 * kGWaves, 1) gather16_kernel(GatherArgs G, GatherLds Lg) {
  constexpr int NT = G16<LP>::kNT, NV = G16<LP>::kNV, PW = 64 / LP;  // PW pairs per wave
  const uint16_t* __restrict__ dense = static_cast<const uint16_t*>(G.dense);
  uint16_t* __restrict__ out_tok = static_cast<uint16_t*>(G.out_tok);
  uint16_t* __restrict__ out_lab = static_cast<uint16_t*>(G.out_lab);
  extern __shared__ __attribute__((aligned(16))) uint8_t g_smem[];
  const int w = wave_id(), lane = threadIdx.x & 63, qw = lane / LP, ql = lane % LP;
  // XCD-contiguous blocks (see gather_kernel)
  const int64_t wg = xcd_block((int64_t)blockIdx.y * gridDim.x + blockIdx.x, (int64_t)gridDim.x * gridDim.y);
  const int64_t q = (wg * kGWaves + w) * PW + qw;
  const bool act = q < G.n_pairs;
  const GatherRec r = act ? G.rec[q] : GatherRec{0, 0, 0, 0, 0, 0, 0};
  const int64_t tof = act ? G.tok_base + G.tok_off[q] : 0;
  const int64_t po = (G.masking && act) ? G.pos_base + G.pos_off[q] : 0;
  const int32_t na = r.na, nb = r.nb_rn & 0x7FFFFFFF, n = na + nb;
  const int32_t nm = G.masking ? r.nm : 0;
  const int64_t mb = r.moff;
  uint8_t* pb = g_smem + ((size_t)w * PW + qw) * Lg.per_pair();
  uint16_t* dec = reinterpret_cast<uint16_t*>(pb);
  uint16_t* spos = reinterpret_cast<uint16_t*>(pb + 2 * (size_t)Lg.seqp);
  uint16_t* slab = reinterpret_cast<uint16_t*>(pb + 2 * (size_t)Lg.seqp + 2 * (kStageRows + 32));
  if (ql == 0 && act) {
    G.len_a[q] = na;
    G.is_rn[q] = (uint8_t)((uint32_t)r.nb_rn >> 31);
    if (G.out_tok_off) {
      G.out_tok_off[q] = tof;
      if (q + 1 == G.n_pairs) G.out_tok_off[q + 1] = tof + n;
    }
    if (G.out_pos_off && G.masking) {
      G.out_pos_off[q] = po;
      if (q + 1 == G.n_pairs) G.out_pos_off[q + 1] = po + nm;
    }
  }
  // both NT-token loads unconditional (an unneeded one reads the window start; dense is padded
  // by 8 tokens on both sides and a B load starts at most 7 tokens before its window, an A load
  // overhangs only by the tokens a shorter A leaves, which the next 8-token vector's select
  // drops), blended when the pass needs them
  uint4 ta[NV], tb[NV];
  auto issue = [&](int32_t x) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int32_t xk = x + 8 * k, bx = xk - na;
      ta[k] = *reinterpret_cast<const uint4*>(dense + r.aoff + (xk < na ? xk : 0));
      tb[k] = *reinterpret_cast<const uint4*>(dense + r.boff + (bx >= -7 && xk < n ? bx : 0));
    }
  };
  issue(NT * ql);
  int32_t rk = 0;
  if (G.masking) {
    for (int i = 8 * ql; i < Lg.seqp; i += 8 * LP)
      *reinterpret_cast<uint4*>(dec + i) = make_uint4(~0u, ~0u, ~0u, ~0u);  // kNoMask16
    wave_sync();
    for (int j = ql; j < nm; j += LP) {
      const int p = G.mpos[mb + j];  // position in [CLS] A [SEP] B [SEP]: never a literal
      const int32_t t = G.mtok[mb + j];
      dec[p <= na ? p - 1 : p - 2] = t == kKeep ? kKeep16 : (uint16_t)t;
    }
    wave_sync();
  }
  for (int32_t cb = 0;; cb += 128) {
    const int32_t x = cb + NT * ql;
    if (cb > 0) issue(x);
    Tok8 v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = __builtin_bit_cast(Tok8, blend8(ta[k], tb[k], na - x - 8 * k));
    if (G.masking) {
      uint32_t dd[NT];
#pragma unroll
      for (int k = 0; k < NT / 8; ++k) {  // (x < seqp, as in gather_kernel)
        const uint4 d = *reinterpret_cast<const uint4*>(dec + x + 8 * k);
        const uint32_t dw[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) dd[8 * k + e] = (dw[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
      }
      uint32_t mk = 0;
#pragma unroll
      for (int e = 0; e < NT; ++e) mk |= dd[e] != kNoMask16 ? 1u << e : 0u;
      const uint32_t c = (uint32_t)__popc(mk);
      uint32_t tot;
      const uint32_t inc = seg_scan<LP>(c, lane, &tot);
      int32_t rr = (int32_t)(inc - c);
#pragma unroll
      for (int e = 0; e < NT; ++e) {
        // only masked elements write their staging entries (exec-masked stores). Writing every
        // element, the unmasked ones to a per-lane trash entry, was 70 % of the kernel's LDS bank
        // conflicts (two lanes per dword, four pairs per wave on the same banks) at the same time
        // per launch (profiles/r06w_gather_lds_attribution.txt)
        const bool m = (mk >> e) & 1u;
        const int32_t xe = x + e;
        if (m) {
          spos[rr] = (uint16_t)(xe < na ? xe + 1 : xe + 2);
          slab[rr] = v[e >> 3][e & 7];
        }
        v[e >> 3][e & 7] = m && dd[e] != kKeep16 ? (uint16_t)dd[e] : v[e >> 3][e & 7];
        rr += m ? 1 : 0;
      }
      wave_sync();
      for (int32_t i = ql; i < (int32_t)tot; i += LP) {
        G.out_pos[po + rk + i] = spos[i];
        out_lab[po + rk + i] = slab[i];
      }
      rk += (int32_t)tot;
      wave_sync();  // (the staging rows are rewritten by the next pass)
    }
    uint16_t* out = out_tok + tof;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int32_t xk = x + 8 * k;
      if (xk + 7 < n) {
        __builtin_nontemporal_store(v[k], reinterpret_cast<Tok8*>(out + xk));
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (xk + e < n) __builtin_nontemporal_store(v[k][e], out + xk + e);
      }
    }
    if (!ballot(n > cb + 128)) break;
  }
}

}  // namespace
}  // namespace lddl

using namespace lddl;

// A/B knobs of the mask replay, LDDL_FY_MODE / LW / RA / PF (what they select: resolve_masks)
struct FyKnobs {
  int mode, lw, ra, pf;
};

// What one planning stage hands to the next: the inputs of the call, host values read back, and
// device temporaries that no later call on the plan reads. The temporaries come from `tmp`,
// today the plan's own scope (they live until lddl_pairs_destroy); a scope local to
// lddl_pairs_plan would return them when planning ends.
// (A split plan keeps it between its head and tail calls, lddl_pairs::work.)
struct PlanWork {
  lddl_ctx* c;
  const lddl_pair_params* prm;  // the plan's own copy (lddl_pairs::prm)
  const int32_t* d_ids;
  const int64_t* d_part_seed;
  int64_t n_sent, n_part;
  hipStream_t st;
  ArenaScope& tmp;
  FyKnobs fy;
  int64_t split_knob = -1;  // LDDL_PLAN_SPLIT
  int64_t slice_knob = -1;  // LDDL_PLAN_SLICE
  int64_t waves_knob = -1;  // LDDL_PLAN_WAVES
  // compact_inputs
  int64_t* scratch = nullptr;  // scan scratch of the compaction and of the re-plan loop
  int64_t n_kept_tok = 0;
  unsigned long long max_docs = 0;  // kept documents of the largest partition
  // plan_replay
  int32_t* jseq = nullptr;
  int64_t* part_npairs = nullptr;
  SlotPool* spool = nullptr;
  void* jpool = nullptr;
  int64_t max_np = 1;  // pairs of the largest partition
  // the planner launch and its pools, kept for the tail call and the re-plan
  PlanArgs A{};
  unsigned long long* pool_ctl = nullptr;  // [0] masks used, [1] overflow flag, [2] draws used, [3] max pairs
  int64_t cap = 0, jcap = 0;
  int32_t* mtok_try = nullptr;  // this attempt's pools
  uint8_t* jpool_try = nullptr;
  int64_t split = 0;            // partitions of the head range (0: one range)
  int64_t* split_info = nullptr;  // split_info_kernel's two values, and their host copies
  int64_t h_split_info[2] = {0, 0};
  int64_t* tail_rel = nullptr;  // the tail partitions' first pairs, relative to the range
  // the time-sliced plan (one range): the queue block (4 control words + the ring, zeroed before
  // every launch), the partitions' save areas and the persistent grid
  bool sliced = false;
  unsigned* sl_queue = nullptr;
  int64_t sl_ring_cap = 0, sl_grid = 0;
  int sl_dense = 1;  // LDDL_PLAN_SLICE_DENSE (A/B): who packs `dense`, see launch_planner
  // shuffle_partitions
  PairMaps M{nullptr, nullptr, nullptr, nullptr};
  // layout
  int2* pcnt = nullptr;
  int64_t* scr2 = nullptr;
#ifdef LDDL_STAMPS
  uint64_t *d_stamps = nullptr, *d_tl = nullptr, *d_tls = nullptr;
#endif
};

// Output pairs of partitions [p0, p1) of a plan: pair q of the range is output pair pair0 + q,
// its tokens start at tok0 + tok_off[q] and its masks at pos0 + pos_off[q].
struct PairRange {
  int64_t p0 = 0, p1 = 0;
  int64_t n_pairs = 0, n_tokens = 0, n_masked = 0;
  int64_t pair0 = 0, tok0 = 0, pos0 = 0;
  GatherRec* rec = nullptr;  // per output pair (pair_prep_kernel / fy_resolve_kernel)
  int64_t *tok_off = nullptr, *pos_off = nullptr;  // [n_pairs + 1]
};

// Device-resident plan of one batch of partitions (library-owned temporaries).
struct lddl_pairs {
  int32_t masking = 0, max_pred = 0, seq = 0, cls_id = -1, sep_id = -1;
  int64_t n_part = 0, n_pairs = 0, n_tokens = 0, n_masked = 0, n_kept_sent = 0, n_kept_doc = 0;
  int64_t n_slices = 0;  // hand-offs of a time-sliced plan (0: not sliced, or no partition parked)
  // every device block of the plan, from the context's arena (the context outlives its plans);
  // lddl_pairs_destroy gives them back on its stream, a plan dropped while planning on the
  // planning stream
  ArenaScope mem;
  // views
  int64_t *ks_start = nullptr, *kd_off = nullptr, *kp_off = nullptr, *kscan = nullptr;
  int32_t* ks_len = nullptr;
  IdPtr dense{nullptr, 4};  // kept tokens, packed in kept-sentence order (id_bytes each)
  PairDesc* desc = nullptr;
  int32_t *order = nullptr, *nmask = nullptr, *mtok = nullptr;
  uint16_t* mpos = nullptr;
  int64_t* moff = nullptr;
  int64_t* src = nullptr;
  // The output pairs' tables. One range covers the plan; a split replay plan has two, the head
  // and the tail partitions' pairs, each with blocks sized by its own pair count.
  PairRange rg[2];
  int n_rg = 1;
  int64_t* part_base = nullptr;  // [n_part + 1] first output pair of each partition
  // first planner launch .. last planner range complete (on the planning stream, after the join)
  hipEvent_t ev[2] = {nullptr, nullptr};
  // split plan: the tail launch runs on the context's side stream between ev_fork (recorded on
  // the planning stream) and ev_join; until the planning stream has waited for ev_join
  // (tail_pending) no block of the plan may go back
  hipStream_t st;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool tail_pending = false;
  bool head_valid = false;  // the head range's tables (and what was gathered from them) stand
  lddl_pair_params prm{};
  std::unique_ptr<PlanWork> work;  // between the head and the tail call

  lddl_pairs(DevArena* arena, hipStream_t stream) : mem(arena, stream), st(stream) {}
  // order `on` after the tail launch (before the plan's blocks go back on it)
  void join(hipStream_t on) {
    if (tail_pending) (void)hipStreamWaitEvent(on, ev_join, 0);
    tail_pending = false;
  }
  ~lddl_pairs() {
    join(st);  // (then `mem` gives the blocks back on st)
    for (hipEvent_t e : {ev[0], ev[1], ev_fork, ev_join})
      if (e) (void)hipEventDestroy(e);
  }
};

static int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// the A/B knobs take only the values a test runs (unsupported values and
// combinations were ignored without notice)
static int read_fy_knobs(FyKnobs* k) {
  *k = FyKnobs{env_int("LDDL_FY_MODE", -1), env_int("LDDL_FY_LW", 16), env_int("LDDL_FY_RA", 1),
               env_int("LDDL_FY_PF", 4)};
  if (k->mode < -1 || k->mode > 1) LDDL_FAIL(-1, "LDDL_FY_MODE must be -1 (auto), 0 or 1");
  if (k->lw != 16 && k->lw != 32) LDDL_FAIL(-1, "LDDL_FY_LW must be 16 or 32");
  if (k->ra < 0 || k->ra > 3) LDDL_FAIL(-1, "LDDL_FY_RA must be 0 .. 3");
  if (k->pf != 2 && k->pf != 4 && k->pf != 8) LDDL_FAIL(-1, "LDDL_FY_PF must be 2, 4 or 8");
  if (k->pf != 4 && k->ra != 1) LDDL_FAIL(-1, "LDDL_FY_PF applies with LDDL_FY_RA=1 only");
  if ((k->ra != 1 || k->pf != 4) && (k->mode == 0 || k->lw == 32))
    LDDL_FAIL(-1, "LDDL_FY_RA / PF select 16-lane branch-free variants (not with LDDL_FY_MODE=0 "
                  "or LDDL_FY_LW=32)");
  return 0;
}

// A/B knob of the split replay plan, LDDL_PLAN_SPLIT: unset or -1 = automatic
// (plan_split_point), 0 = one range, k > 0 = a head range of exactly min(k, n_part) partitions
static int read_split_knob(int64_t* k) {
  *k = -1;
  const char* e = getenv("LDDL_PLAN_SPLIT");
  if (!e) return 0;
  char* end = nullptr;
  const long long v = strtoll(e, &end, 10);
  if (end == e || *end || v < -1) LDDL_FAIL(-1, "LDDL_PLAN_SPLIT must be -1 (auto), 0 or a partition count");
  *k = v;
  return 0;
}

// A/B knob of the time-sliced replay plan, LDDL_PLAN_SLICE: unset or -1 = automatic
// (plan_slice_on), 0 = never, k > 0 = always, with a quantum of k documents. LDDL_PLAN_WAVES
// (tests and A/B): the persistent grid of a sliced plan, g >= 1 workgroups (unset or -1: what the
// device holds at once).
static int read_slice_knobs(int64_t split_knob, int64_t* slice, int64_t* waves) {
  *slice = *waves = -1;
  if (const char* e = getenv("LDDL_PLAN_SLICE")) {
    char* end = nullptr;
    const long long v = strtoll(e, &end, 10);
    if (end == e || *end || v < -1)
      LDDL_FAIL(-1, "LDDL_PLAN_SLICE must be -1 (auto), 0 or a quantum of documents");
    *slice = v;
  }
  if (const char* e = getenv("LDDL_PLAN_WAVES")) {
    char* end = nullptr;
    const long long v = strtoll(e, &end, 10);
    if (end == e || *end || v < -1 || v == 0 || v > (1 << 20))
      LDDL_FAIL(-1, "LDDL_PLAN_WAVES must be -1 (auto) or a workgroup count up to 2^20");
    *waves = v;
  }
  if (split_knob > 0 && *slice > 0)
    LDDL_FAIL(-1, "LDDL_PLAN_SPLIT and LDDL_PLAN_SLICE are both forced: a split plan is not sliced");
  return 0;
}

static int check_plan_args(const lddl_ctx* c, const lddl_pair_params* prm, FyKnobs* fy, int64_t* split_knob,
                           int64_t* slice_knob, int64_t* waves_knob) {
  if (!c || !prm) LDDL_FAIL(-1, "null argument");
  if (prm->seq < 5 || prm->seq > 65535) LDDL_FAIL(-1, "target_seq_length %d out of range", prm->seq);
  if (prm->dup < 1) LDDL_FAIL(-1, "duplicate_factor must be >= 1");
  if (prm->rng != LDDL_RNG_REPLAY && prm->rng != LDDL_RNG_NATIVE)
    LDDL_FAIL(-1, "unknown rng mode %d", prm->rng);
  if (prm->masking && prm->seq > kMaxSeqGather)
    LDDL_FAIL(-1, "static masking supports target_seq_length <= %d", kMaxSeqGather);
  if (prm->masking && (c->tab.special_id[kCls] < 0 || c->tab.special_id[kSep] < 0 ||
                       c->tab.special_id[kMask] < 0))
    LDDL_FAIL(-1, "static masking needs [CLS] [SEP] [MASK] in the vocab");
  if (prm->whole_word && !prm->masking) LDDL_FAIL(-1, "whole_word needs static masking (masking = 1)");
  if (prm->whole_word && prm->rng != LDDL_RNG_NATIVE)
    LDDL_FAIL(-1, "whole_word needs rng = LDDL_RNG_NATIVE (the replay mode reproduces the "
                  "reference, which has no whole-word masking)");
  int rc;
  if ((rc = read_split_knob(split_knob)) || (rc = read_slice_knobs(*split_knob, slice_knob, waves_knob)))
    return rc;
  return read_fy_knobs(fy);
}

// replay mode: the planner launch's tail workgroups pack `dense` (plan_replay_kernel)
static bool dense_in_plan(const PlanWork& W) { return W.prm->rng == LDDL_RNG_REPLAY && W.n_part > 0; }

// ceil(p * 2^53): random() < p  <=>  N < this (N = 53-bit integer behind random())
static uint64_t short_threshold(double p) {
  if (!(p > 0)) return 0;
  if (p >= 1) return 1ull << 53;
  return (uint64_t)ceil(ldexp(p, 53));
}

struct I32 {
  const int32_t* v;
  __device__ int64_t operator()(int64_t i) const { return v[i]; }
};

// Drop empty sentences and documents: the kept-sentence tables, the partitions' kept-document
// offsets and the dense token buffer.
static int compact_inputs(lddl_pairs* P, PlanWork& W, const int64_t* d_sent_off,
                          const int32_t* d_sent_len, const int64_t* d_doc_sent_off, int64_t n_doc,
                          const int64_t* d_part_doc_off) {
  const int64_t n_sent = W.n_sent, n_part = W.n_part;
  hipStream_t st = W.st;
  int rc;
  int64_t *ks_pos, *tok_pos, *kd_pos;
  const int64_t nscr = 2 * scan_scratch_elems(std::max(n_sent, n_doc) + n_part + 1);  // (dual scans)
  // kept-sentence index and token offset of every sentence in one scan
  if ((rc = W.tmp.take(&W.scratch, nscr)) || (rc = W.tmp.take(&ks_pos, n_sent + 1)) ||
      (rc = W.tmp.take(&tok_pos, n_sent + 1)))
    return rc;
  LDDL_HIP(scan_exclusive2(SentCounts{d_sent_len}, n_sent, ks_pos, tok_pos, W.scratch, st));
  if ((rc = W.tmp.take(&kd_pos, n_doc + 1))) return rc;
  LDDL_HIP(scan_exclusive(KeepDoc{ks_pos, d_doc_sent_off}, n_doc, kd_pos, W.scratch, st));
  int64_t h_counts[3];
  LDDL_HIP(hipMemcpyAsync(&h_counts[0], ks_pos + n_sent, 8, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipMemcpyAsync(&h_counts[1], kd_pos + n_doc, 8, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipMemcpyAsync(&h_counts[2], tok_pos + n_sent, 8, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipStreamSynchronize(st));
  P->n_kept_sent = h_counts[0];
  P->n_kept_doc = h_counts[1];
  W.n_kept_tok = h_counts[2];  // (dropped sentences have no tokens)
  unsigned long long* d_max_docs;
  if ((rc = P->mem.take(&P->ks_start, P->n_kept_sent)) || (rc = P->mem.take(&P->ks_len, P->n_kept_sent)) ||
      (rc = P->mem.take(&P->kscan, P->n_kept_sent + 1)) || (rc = P->mem.take(&P->kd_off, P->n_kept_doc + 1)) ||
      (rc = P->mem.take(&P->kp_off, n_part + 1)) || (rc = W.tmp.take(&d_max_docs, 1)))
    return rc;
  hipLaunchKernelGGL(scatter_sentences_kernel, dim3((unsigned)((n_sent + 256) / 256)), dim3(256), 0,
                     st, d_sent_off, d_sent_len, n_sent, ks_pos, tok_pos, P->ks_start, P->ks_len,
                     P->kscan);
  hipLaunchKernelGGL(scatter_docs_kernel, dim3((unsigned)((n_doc + 256) / 256)), dim3(256), 0, st,
                     d_doc_sent_off, n_doc, ks_pos, kd_pos, P->kd_off);
  LDDL_HIP(hipMemsetAsync(d_max_docs, 0, 8, st));
  hipLaunchKernelGGL(part_offsets_kernel, dim3((unsigned)((n_part + 256) / 256)), dim3(256), 0, st,
                     d_part_doc_off, n_part, kd_pos, P->kp_off, d_max_docs);
  LDDL_HIP(hipGetLastError());
  LDDL_HIP(hipMemcpyAsync(&W.max_docs, d_max_docs, 8, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipStreamSynchronize(st));
  // dense kept tokens, 8 tokens of padding on both sides: the gather's 4- and 8-token loads may
  // overhang a window
  const int32_t ib = W.c->id_bytes();
  uint8_t* raw;
  if ((rc = P->mem.take(&raw, (W.n_kept_tok + 16) * ib))) return rc;
  P->dense = IdPtr{raw + 8 * ib, ib};
  if (P->n_kept_sent && !dense_in_plan(W))
    hipLaunchKernelGGL(densify_kernel, dim3((unsigned)((P->n_kept_sent + 255) / 256)), dim3(256), 0,
                       st, P->ks_start, P->ks_len, P->kscan, P->n_kept_sent, W.d_ids, P->dense);
  LDDL_HIP(hipGetLastError());
  return 0;
}

// The gather records + output-order scans (tok_off, pos_off) of the plan's pairs.
// (of one range; W.pcnt / W.scr2 are the range's temporaries)
static int layout_alloc(lddl_pairs* P, PlanWork& W, PairRange& r) {
  const int64_t npairs = r.n_pairs;
  int rc;
  if ((rc = P->mem.take(&r.tok_off, npairs + 1)) || (rc = P->mem.take(&r.rec, npairs)) ||
      (rc = W.tmp.take(&W.pcnt, npairs)) || (rc = W.tmp.take(&W.scr2, 2 * scan_scratch_elems(npairs))))
    return rc;
  if (P->masking && (rc = P->mem.take(&r.pos_off, npairs + 1))) return rc;
  return 0;
}

// tok_off (and pos_off) from the counts, then the range's totals (read with the caller's sync)
static int layout_scan(lddl_pairs* P, PlanWork& W, PairRange& r) {
  if (P->masking)
    LDDL_HIP(scan_exclusive2(PairCounts{W.pcnt}, r.n_pairs, r.tok_off, r.pos_off, W.scr2, W.st));
  else
    LDDL_HIP(scan_exclusive(PairTokens{W.pcnt}, r.n_pairs, r.tok_off, W.scr2, W.st));
  LDDL_HIP(hipMemcpyAsync(&r.n_tokens, r.tok_off + r.n_pairs, 8, hipMemcpyDeviceToHost, W.st));
  if (P->masking)
    LDDL_HIP(hipMemcpyAsync(&r.n_masked, r.pos_off + r.n_pairs, 8, hipMemcpyDeviceToHost, W.st));
  return 0;
}

// gather records from the output order (src): the native path, and replay without masking
static int layout_pairs(lddl_pairs* P, PlanWork& W) {
  int rc;
  PairRange& r = P->rg[0];  // (always one range)
  r.p1 = P->n_part;
  r.n_pairs = P->n_pairs;
  if ((rc = layout_alloc(P, W, r))) return rc;
  const int64_t npairs = P->n_pairs;
  if (npairs)
    hipLaunchKernelGGL(pair_prep_kernel, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, W.st,
                       P->src, npairs, P->desc, P->kscan, P->masking ? P->nmask : nullptr,
                       P->moff, r.rec, W.pcnt);
  LDDL_HIP(hipGetLastError());
  return layout_scan(P, W, r);
}

// the kept corpus and the call's parameters, as both planners' kernels take them
template <typename Args>
static void fill_plan_args(Args& A, const lddl_pairs* P, const PlanWork& W) {
  A.kscan = P->kscan;
  A.ks_len = P->ks_len;
  A.kd_off = P->kd_off;
  A.kp_off = P->kp_off;
  A.dense = P->dense;
  A.part_seed = W.d_part_seed;
  A.n_part = (decltype(A.n_part))W.n_part;
  A.seq = W.prm->seq;
  A.dup = W.prm->dup;
  A.masking = W.prm->masking;
  A.vocab_size = W.c->vocab_size;
  A.cls_id = P->cls_id;
  A.sep_id = P->sep_id;
  A.mask_id = W.c->tab.special_id[kMask];
  A.ratio = W.prm->masked_lm_ratio;
  A.k_short = short_threshold(W.prm->short_seq_prob);
}

// LDDL_RNG_NATIVE control plane: count pass, unit scan, emit pass, mask offsets + masks, order,
// layout.
static int plan_native(lddl_pairs* P, PlanWork& W) {
  const lddl_pair_params* prm = W.prm;
  const int64_t n_part = W.n_part;
  hipStream_t st = W.st;
  NativeArgs A{};
  fill_plan_args(A, P, W);
  int64_t kp_ends[2] = {0, 0};  // kept documents covered by the partitions
  unsigned long long need_max = 0, *d_need;
  int rc;
  if ((rc = W.tmp.take(&d_need, 1))) return rc;
  LDDL_HIP(hipMemsetAsync(d_need, 0, 8, st));
  if (n_part)
    hipLaunchKernelGGL(native_part_need_kernel, dim3((unsigned)((n_part + 255) / 256)), dim3(256), 0, st,
                       P->kp_off, P->kd_off, n_part, d_need);
  LDDL_HIP(hipMemcpyAsync(&kp_ends[0], P->kp_off, 8, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipMemcpyAsync(&kp_ends[1], P->kp_off + n_part, 8, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipMemcpyAsync(&need_max, d_need, 8, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipStreamSynchronize(st));
  A.unit0 = (int64_t)prm->dup * kp_ends[0];
  A.n_units = (int64_t)prm->dup * (kp_ends[1] - kp_ends[0]);
  A.native_seed = prm->native_seed;
  const int64_t nu = A.n_units;
  // walk tables in LDS up to 96 KB per workgroup; larger partitions read a global prefix
  int64_t kLdsWordsCap = 24576;
  if (const char* e = getenv("LDDL_NATIVE_LDS_WORDS")) kLdsWordsCap = atoll(e);  // tests: global path
  const int32_t lds_words = (int32_t)std::max<int64_t>(
      1, std::min<int64_t>((int64_t)need_max, kLdsWordsCap));
  int64_t *uoff, *scr, *g_pre = nullptr;
  if ((rc = W.tmp.take(&A.ucnt, nu)) || (rc = W.tmp.take(&uoff, nu + 1)) ||
      (rc = W.tmp.take(&scr, scan_scratch_elems(std::max(nu, P->n_kept_sent) + 1))))
    return rc;
  if ((int64_t)need_max > kLdsWordsCap) {
    if ((rc = W.tmp.take(&g_pre, P->n_kept_sent + 1))) return rc;
    LDDL_HIP(scan_exclusive(KeptLenOnly{P->ks_len}, P->n_kept_sent, g_pre, scr, st));
  }
  LDDL_HIP(hipEventRecord(P->ev[0], st));
  const size_t lds_bytes = (size_t)4 * lds_words;
  if (n_part && nu)
    hipLaunchKernelGGL(plan_native_kernel<false>, dim3((unsigned)n_part), dim3(kNativeThreads), lds_bytes,
                       st, A, g_pre, lds_words);
  LDDL_HIP(hipGetLastError());
  LDDL_HIP(scan_exclusive(Identity{A.ucnt}, nu, uoff, scr, st));
  LDDL_HIP(hipMemcpyAsync(&P->n_pairs, uoff + nu, 8, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipStreamSynchronize(st));
  const int64_t n = P->n_pairs;
  A.uoff = uoff;
  A.n_pairs = n;
  if ((rc = P->mem.take(&P->part_base, n_part + 1)) || (rc = P->mem.take(&P->desc, n)) ||
      (rc = W.tmp.take(&A.ppart, n)) || (rc = P->mem.take(&P->src, n)))
    return rc;
  if (prm->masking &&
      ((rc = P->mem.take(&P->nmask, n)) || (rc = W.tmp.take(&A.ncand, n)) ||
       (rc = P->mem.take(&P->moff, n + 1)) || (rc = W.tmp.take(&scr, scan_scratch_elems(n + 1)))))
    return rc;
  hipLaunchKernelGGL(native_part_base_kernel, dim3((unsigned)((n_part + 256) / 256)), dim3(256), 0,
                     st, P->kp_off, n_part, prm->dup, uoff, P->part_base);
  A.part_base = P->part_base;
  A.desc = P->desc;
  A.nmask = P->nmask;
  if (n_part && nu)
    hipLaunchKernelGGL(plan_native_kernel<true>, dim3((unsigned)n_part), dim3(kNativeThreads), lds_bytes,
                       st, A, g_pre, lds_words);
  LDDL_HIP(hipGetLastError());
  const unsigned gp = (unsigned)((n + 255) / 256);
  if (prm->masking) {
    LDDL_HIP(scan_exclusive(I32{P->nmask}, n, P->moff, scr, st));
    LDDL_HIP(hipMemcpyAsync(&P->n_masked, P->moff + n, 8, hipMemcpyDeviceToHost, st));
    LDDL_HIP(hipStreamSynchronize(st));
    if ((rc = P->mem.take(&P->mpos, P->n_masked)) || (rc = P->mem.take(&P->mtok, P->n_masked)))
      return rc;
    A.moff = P->moff;
    A.mpos = P->mpos;
    A.mtok = P->mtok;
    A.words = (prm->seq + 31) / 32;
    // per wave: the 64 lanes' bitmaps + the staged masks of its 64 pairs (<= max_pred each);
    // up to 4 waves per workgroup within 64 KB of LDS
    const int32_t stage_cap = 64 * std::max(P->max_pred, 1);
    const size_t per_wave = (size_t)A.words * 64 * 4 + (size_t)stage_cap * 6;
    const int nwv = (int)std::max<size_t>(1, std::min<size_t>(4, 65536 / per_wave));
    if (n && !prm->whole_word)
      hipLaunchKernelGGL(mask_native_kernel, dim3((unsigned)((n + 64 * nwv - 1) / (64 * nwv))),
                         dim3(64 * nwv), per_wave * nwv, st, A, stage_cap);
    if (n && prm->whole_word) {
      // one wave per pair; per wave an 8-byte entry per token of the longest pair (seq - 3,
      // rounded up to whole windows) and a ballot per window + 1; up to 4 waves within 64 KB
      const int32_t seqp = (prm->seq - 3 + 63) / 64 * 64;
      const size_t ww_wave = (size_t)8 * (seqp + seqp / 64 + 1);
      const int wwv = (int)std::max<size_t>(1, std::min<size_t>(4, 65536 / ww_wave));
      hipLaunchKernelGGL(mask_ww_native_kernel, dim3((unsigned)((n + wwv - 1) / wwv)), dim3(64 * wwv),
                         ww_wave * wwv, st, A, ContBits{W.c->d_cont_bits, W.c->vocab_size}, seqp);
    }
    LDDL_HIP(hipGetLastError());
  }
  A.src = P->src;
  if (n) hipLaunchKernelGGL(order_native_kernel, dim3(gp), dim3(256), 0, st, A);
  LDDL_HIP(hipGetLastError());
  LDDL_HIP(hipEventRecord(P->ev[1], st));
  return layout_pairs(P, W);
}

// LDDL_RNG_REPLAY planner, set-up: the slot tables, the planner's arguments (W.A) and the sizes
// of the mask pools; decides whether the launch is split into a head and a tail range.
static int plan_replay_setup(lddl_pairs* P, PlanWork& W) {
  const lddl_pair_params* prm = W.prm;
  const int64_t n_part = W.n_part;
  if (prm->seq > 512) LDDL_FAIL(-1, "replay planner supports target_seq_length <= 512");
  const int64_t slots = (int64_t)prm->dup * P->n_kept_sent;
  int rc;
  if ((rc = P->mem.take(&P->desc, slots)) || (rc = P->mem.take(&P->order, slots)) ||
      (rc = W.tmp.take(&W.jseq, slots)) || (rc = W.tmp.take(&W.part_npairs, n_part + 1)))
    return rc;
  if (prm->masking && (rc = W.tmp.take(&W.spool, slots))) return rc;
  PlanArgs& A = W.A;
  fill_plan_args(A, P, W);
  A.ks_start = P->ks_start;
  A.ids = W.d_ids;
  A.n_kept_sent = dense_in_plan(W) ? P->n_kept_sent : 0;
  A.n_dense_wg = 4096;
  A.max_pred = P->max_pred;
  A.short_seq_prob = prm->short_seq_prob;
  A.seq_r64 = ((prm->seq + 63) / 64) * 64;
  A.desc = P->desc;
  A.jseq = W.jseq;
  A.spool = W.spool;
  A.part_npairs = W.part_npairs;
#ifdef LDDL_STAMPS
  if ((rc = W.tmp.take(&W.d_stamps, n_part * kStampRegions)) || (rc = W.tmp.take(&W.d_tl, n_part * 2)))
    return rc;
  LDDL_HIP(hipMemsetAsync(W.d_stamps, 0, 8 * n_part * kStampRegions, W.st));
  LDDL_HIP(hipMemsetAsync(W.d_tl, 0, 16 * n_part, W.st));
  A.stamps = W.d_stamps;
  A.tl = W.d_tl;
#endif
  // pools: decisions (int32, shuffled order) and shuffle draws (uint16), sized from the kept
  // tokens (expected use ~0.15 * 1.5 and ~1.5 times dup * tokens); a plan that outgrows them
  // reports the exact sizes and is planned again (deterministic replay)
  if ((rc = W.tmp.take(&W.pool_ctl, 4)) || (rc = P->mem.take(&P->part_base, n_part + 1))) return rc;
  W.cap = W.jcap = 0;
  A.jbytes = prm->seq <= 256 ? 1 : 2;  // every draw j_i < nc <= seq - 3
  if (prm->masking && W.n_sent) {
    W.cap = (int64_t)(2.0 * prm->masked_lm_ratio * prm->dup * (double)W.n_kept_tok) +
            (int64_t)prm->dup * P->n_kept_sent / 2 + kPoolChunk * (n_part + 16);
    W.jcap = (int64_t)(1.6 * prm->dup * (double)W.n_kept_tok) + 8 * slots +
             kPoolChunk * (n_part + 16);  // + the 16-entry alignment of every pair's draws
    if (const char* e = getenv("LDDL_AMD_MASK_POOL")) W.cap = atoll(e);  // tests: force a re-plan
  }
  // SlotPool keeps pool offsets as 32-bit multiples of 8 / 16 entries
  if (W.cap / 8 >= (int64_t)UINT32_MAX || W.jcap / 16 >= (int64_t)UINT32_MAX)
    LDDL_FAIL(-1, "batch too large for the mask pools (split it into smaller GPU batches)");
  A.pool_used = W.pool_ctl;
  A.overflow = reinterpret_cast<int32_t*>(W.pool_ctl + 1);
  return 0;
}

typedef void (*PlanKernel)(PlanArgs);
static PlanKernel planner_kernel(const PlanWork& W) {
  const bool docs_lds = W.max_docs + 1 <= (unsigned long long)kDocLds;  // document table in LDS
  if (W.sliced)
    return docs_lds ? (W.A.jbytes == 1 ? plan_replay_kernel<true, 1, true> : plan_replay_kernel<true, 2, true>)
                    : (W.A.jbytes == 1 ? plan_replay_kernel<false, 1, true> : plan_replay_kernel<false, 2, true>);
  return docs_lds ? (W.A.jbytes == 1 ? plan_replay_kernel<true, 1> : plan_replay_kernel<true, 2>)
                  : (W.A.jbytes == 1 ? plan_replay_kernel<false, 1> : plan_replay_kernel<false, 2>);
}
constexpr size_t kPlanLds = 4 * (kN + kLook) + 4 * (kDocLds + 4) + 16;  // ~4.8 KB: 7 waves/SIMD fit

// The head range of a split replay plan with static masking (0: one range): what the device
// holds of the planner's one-wave workgroups at once, see plan_split_point.
// planner workgroups (one wave each) the device holds at once, for the instantiation W selects
static int planner_capacity(const PlanWork& W, int64_t* capacity) {
  int per_cu = 0, n_cu = 0;
  LDDL_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, planner_kernel(W), 64, kPlanLds));
  LDDL_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, W.c->device));
  *capacity = (int64_t)per_cu * n_cu;
  return 0;
}

static int choose_split(const PlanWork& W, int64_t* s) {
  *s = 0;
  if (W.sliced || !W.prm->masking || W.n_part <= 0 || W.split_knob == 0) return 0;
  int64_t capacity = 0;
  int rc;
  if (W.split_knob < 0 && (rc = planner_capacity(W, &capacity))) return rc;
  *s = plan_split_point(W.n_part, capacity, W.split_knob);
  return 0;
}

// Whether the plan runs time-sliced in one range (plan_slice_on; with or without masking; a
// forced split keeps the split path), and then its grid, ring and save areas.
static int choose_slice(const lddl_pairs* P, PlanWork& W) {
  W.sliced = false;
  if (W.n_part <= 0 || W.split_knob > 0 || W.slice_knob == 0) return 0;
  if (W.slice_knob < 0 && !kPlanSliceAuto) return 0;
  int64_t capacity = 0;
  int rc;
  W.sliced = true;  // (the capacity of the sliced instantiation)
  rc = planner_capacity(W, &capacity);
  W.sliced = !rc && plan_slice_on(W.n_part, capacity, W.slice_knob);
  if (rc || !W.sliced) return rc;
  W.sl_grid = std::min<int64_t>(W.n_part, W.waves_knob > 0 ? W.waves_knob : std::max<int64_t>(capacity, 1));
  W.sl_dense = env_int("LDDL_PLAN_SLICE_DENSE", 1);
  if (W.sl_dense < 0 || W.sl_dense > 2) LDDL_FAIL(-1, "LDDL_PLAN_SLICE_DENSE must be 0, 1 or 2");
  const unsigned __int128 units = (unsigned __int128)(uint64_t)W.prm->dup * (uint64_t)P->n_kept_doc;
  W.sl_ring_cap = plan_slice_ring_entries(
      W.n_part, units > (unsigned __int128)INT64_MAX ? INT64_MAX : (int64_t)units, W.slice_knob);
  // tickets and dense-group claims are 32-bit counters
  if (W.sl_ring_cap >= INT32_MAX - W.n_part || P->n_kept_sent / 64 >= INT32_MAX - (int64_t)(1 << 24))
    LDDL_FAIL(-1, "batch too large for the time-sliced plan (LDDL_PLAN_SLICE=0, or smaller GPU batches)");
  uint64_t* save;
  if ((rc = W.tmp.take(&W.sl_queue, 4 + ((W.sl_ring_cap + 3) & ~(int64_t)3))) ||
      (rc = W.tmp.take(&save, W.n_part * kSaveU64)))
    return rc;
  PlanArgs& A = W.A;
  A.sl_ctl = W.sl_queue;
  A.sl_ring = W.sl_queue + 4;
  A.sl_save = save;
  A.sl_ring_cap = (int32_t)W.sl_ring_cap;
  A.sl_dense = W.sl_dense == 1;
  A.sl_quantum = (int32_t)std::min<int64_t>(std::max<int64_t>(W.slice_knob, 0), INT32_MAX);
#ifdef LDDL_STAMPS
  if ((rc = W.tmp.take(&W.d_tls, 2 * (W.n_part + W.sl_ring_cap)))) return rc;
  LDDL_HIP(hipMemsetAsync(W.d_tls, 0, 16 * (W.n_part + W.sl_ring_cap), W.st));
  A.tls = W.d_tls;
#endif
  return 0;
}

// The pools of one planning attempt (the counters cleared on the stream first). A split plan also
// takes `mpos` here, at the pool's capacity: mpos shares the mask pool's index space, and the
// head's mask replay fills it while the tail range still allocates from the pool.
static int take_pools(lddl_pairs* P, PlanWork& W, bool split) {
  W.mtok_try = nullptr;
  W.jpool_try = nullptr;
  int rc;
  if (W.prm->masking) {
    LDDL_HIP(hipMemsetAsync(W.pool_ctl, 0, 32, W.st));
    if ((rc = P->mem.take(&W.mtok_try, W.cap + 4)) ||
        (rc = W.tmp.take(&W.jpool_try, W.A.jbytes * (W.jcap + 16))))
      return rc;
    if (split && (rc = P->mem.take(&P->mpos, W.cap + 4))) return rc;
  }
  W.A.mtok = W.mtok_try;
  W.A.jpool = W.jpool_try;
  W.A.pool_cap = W.cap;
  W.A.jpool_cap = W.jcap;
  return 0;
}

// One plan_replay_kernel launch over partitions [p0, p0 + n) on `st`. with_dense: its extra
// workgroups pack the kept sentences from *dense_lo on (null: all of them).
static int launch_planner(const PlanWork& W, int64_t p0, int64_t n, hipStream_t st, bool with_dense,
                          const int64_t* dense_lo) {
  PlanArgs A = W.A;
  A.p0 = (int32_t)p0;
  A.n_part = (int32_t)n;
  A.dense_lo = dense_lo;
  if (!with_dense) A.n_kept_sent = 0;
  if (W.sliced) {
    // The whole plan by the persistent grid. `dense` is packed by the waves that leave the queue
    // (the default), or by densify_kernel behind (LDDL_PLAN_SLICE_DENSE=0) or ahead of the
    // planner (2): the one-shot launch's tail, which hides that work, no longer exists.
    auto densify = [&]() {
      if (A.n_kept_sent)
        hipLaunchKernelGGL(densify_kernel, dim3((unsigned)((A.n_kept_sent + 255) / 256)), dim3(256), 0, st,
                           A.ks_start, A.ks_len, A.kscan, A.n_kept_sent, A.ids, A.dense);
    };
    LDDL_HIP(hipMemsetAsync(W.sl_queue, 0, 4 * (4 + ((W.sl_ring_cap + 3) & ~(int64_t)3)), st));
    if (W.sl_dense == 2) densify();
    hipLaunchKernelGGL(planner_kernel(W), dim3((unsigned)W.sl_grid), dim3(64), kPlanLds, st, A);
    if (W.sl_dense == 0) densify();
    LDDL_HIP(hipGetLastError());
    return 0;
  }
  const unsigned grid = (unsigned)n + (A.n_kept_sent ? (unsigned)A.n_dense_wg : 0u);
  if (grid) hipLaunchKernelGGL(planner_kernel(W), dim3(grid), dim3(64), kPlanLds, st, A);
  LDDL_HIP(hipGetLastError());
  return 0;
}

// One range: launches plan_replay_kernel (between the plan's two events) and, when a pool
// overflowed, once more with the exact sizes. attempt 1: the re-plan of a split plan.
static int plan_replay_unsplit(lddl_pairs* P, PlanWork& W, int attempt) {
  const lddl_pair_params* prm = W.prm;
  const int64_t n_part = W.n_part;
  hipStream_t st = W.st;
  int rc;
  for (; n_part; ++attempt) {
    if ((rc = take_pools(P, W, false))) return rc;
    LDDL_HIP(hipEventRecord(P->ev[0], st));
    if ((rc = launch_planner(W, 0, n_part, st, true, nullptr))) return rc;
    LDDL_HIP(hipEventRecord(P->ev[1], st));
    // pairs per partition -> output offsets and the largest count, read back with the pool
    // counters in the planner's one sync
    if (!prm->masking) LDDL_HIP(hipMemsetAsync(W.pool_ctl, 0, 32, st));
    LDDL_HIP(scan_exclusive(Identity{W.part_npairs}, n_part, P->part_base, W.scratch, st));
    hipLaunchKernelGGL(max_pairs_kernel, dim3(64), dim3(256), 0, st, W.part_npairs, n_part, W.pool_ctl + 3);
    unsigned long long ctl[4];
    LDDL_HIP(hipMemcpyAsync(ctl, W.pool_ctl, 32, hipMemcpyDeviceToHost, st));
    LDDL_HIP(hipMemcpyAsync(&P->n_pairs, P->part_base + n_part, 8, hipMemcpyDeviceToHost, st));
    unsigned sl_ctl[4] = {0, 0, 0, 0};
    if (W.sliced) LDDL_HIP(hipMemcpyAsync(sl_ctl, W.sl_queue, 16, hipMemcpyDeviceToHost, st));
    LDDL_HIP(hipStreamSynchronize(st));
    P->n_slices = sl_ctl[1];
    W.max_np = std::max<int64_t>(1, (int64_t)ctl[3]);
    if (!prm->masking) break;
    if (!ctl[1]) {
      P->mtok = W.mtok_try;
      W.jpool = W.jpool_try;
      if ((rc = P->mem.take(&P->mpos, (int64_t)ctl[0]))) return rc;
      break;
    }
    P->mem.give(W.mtok_try);
    W.tmp.give(W.jpool_try);
    if (attempt > 0) LDDL_FAIL(-1, "mask pool overflow after resize");
    W.cap = (int64_t)ctl[0] + 1024;
    W.jcap = (int64_t)ctl[2] + 1024;
  }
  return 0;
}

// The context's side stream for the tail range: non-blocking (the caller's stream may be the
// null stream) and of the lowest priority, so the head range's workgroups are placed first.
static int plan_side_stream(lddl_ctx* c, hipStream_t* out) {
  if (!c->plan_side) {
    int least = 0, greatest = 0;
    LDDL_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    LDDL_HIP(hipStreamCreateWithPriority(&c->plan_side, hipStreamNonBlocking, least));
  }
  *out = c->plan_side;
  return 0;
}

// Split plan, first half: the head range [0, s) on the caller's stream and the tail range
// [s, n_part) on the side stream, both allocating from the same pools. The tail launch keeps the
// dense-packing workgroups for its kept sentences; the head's are packed by densify_head_kernel,
// first on the caller's stream after the head planner (by then every tail workgroup that fits is
// resident). Returns after the head's sync with rg[0].n_pairs and *usable = no pool overflow so
// far (else the head's slots may point past the pools and nothing downstream may run on them).
static int plan_replay_split_head(lddl_pairs* P, PlanWork& W, bool* usable) {
  const int64_t n_part = W.n_part, s = W.split;
  hipStream_t st = W.st, side;
  int rc;
  if ((rc = plan_side_stream(W.c, &side)) || (rc = take_pools(P, W, true)) ||
      (rc = W.tmp.take(&W.split_info, 2)) || (rc = W.tmp.take(&W.tail_rel, n_part - s + 1)))
    return rc;
  LDDL_HIP(hipEventCreateWithFlags(&P->ev_fork, hipEventDisableTiming));
  LDDL_HIP(hipEventCreateWithFlags(&P->ev_join, hipEventDisableTiming));
  hipLaunchKernelGGL(split_info_kernel, dim3(1), dim3(1), 0, st, P->kp_off, P->kd_off, P->kscan, s,
                     W.split_info);
  LDDL_HIP(hipGetLastError());
  LDDL_HIP(hipEventRecord(P->ev[0], st));
  // the side stream starts after the compaction (and everything else queued on st so far)
  LDDL_HIP(hipEventRecord(P->ev_fork, st));
  LDDL_HIP(hipStreamWaitEvent(side, P->ev_fork, 0));
  if ((rc = launch_planner(W, 0, s, st, false, nullptr))) return rc;
  P->tail_pending = true;  // (from here every return path joins before a block goes back)
  rc = launch_planner(W, s, n_part - s, side, true, W.split_info);
  LDDL_HIP(hipEventRecord(P->ev_join, side));
  if (rc) return rc;
  if (P->n_kept_sent)
    hipLaunchKernelGGL(densify_head_kernel, dim3((unsigned)((P->n_kept_sent + 255) / 256)), dim3(256),
                       0, st, P->ks_start, P->ks_len, P->kscan, W.split_info, W.d_ids, P->dense);
  LDDL_HIP(scan_exclusive(Identity{W.part_npairs}, s, P->part_base, W.scratch, st));
  hipLaunchKernelGGL(max_pairs_kernel, dim3(64), dim3(256), 0, st, W.part_npairs, s, W.pool_ctl + 3);
  LDDL_HIP(hipGetLastError());
  unsigned long long ctl[4];
  LDDL_HIP(hipMemcpyAsync(ctl, W.pool_ctl, 32, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipMemcpyAsync(&P->rg[0].n_pairs, P->part_base + s, 8, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipMemcpyAsync(W.h_split_info, W.split_info, 16, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipStreamSynchronize(st));
  W.max_np = std::max<int64_t>(1, (int64_t)ctl[3]);
  *usable = ctl[1] == 0;
  return 0;
}

// random.shuffle(partition_pairs) of one range, alone on the stream (its blocks need 16 waves
// and ~90 KB of LDS per CU: beside fy_resolve's small blocks on a second stream they waited for
// CUs to drain, 10.3 ms against ~2 alone); its last pass writes the pair maps (see PairMaps): with
// masking the planner-order slots and their output positions (the mask replay writes each
// pair's gather record there), else the output order. rel_base[i]: the first pair of the
// range's partition i, counted from the range's first pair.
static int shuffle_partitions(lddl_pairs* P, PlanWork& W, const PairRange& r, const int64_t* rel_base) {
  const lddl_pair_params* prm = W.prm;
  const int64_t n_part = r.p1 - r.p0;
  hipStream_t st = W.st;
  int rc;
  PairMaps& M = W.M;
  M = PairMaps{rel_base, nullptr, nullptr, nullptr};
  if (prm->masking) {
    if ((rc = W.tmp.take(&M.slots, r.n_pairs)) || (rc = W.tmp.take(&M.dstq, r.n_pairs))) return rc;
  } else {
    if ((rc = P->mem.take(&P->src, r.n_pairs))) return rc;
    M.src = P->src;
  }
  if (n_part) {
    const int64_t cap = W.max_np;
    const int64_t* kp_off = P->kp_off + r.p0;  // (the kernels index partitions by workgroup)
    const int64_t* part_npairs = W.part_npairs + r.p0;
    // dynamic-LDS budget of the swap kernel: what the device grants a block (160 KiB on
    // gfx950), minus headroom for the kernel's static LDS
    const size_t kLdsBudget = std::min<size_t>(150 * 1024, W.c->lds_per_block > 10 * 1024
                                                               ? W.c->lds_per_block - 10 * 1024 : 0);
    const bool force_global = getenv("LDDL_SHUFFLE_GLOBAL") != nullptr;  // tests: the large-partition path
    // partitions of <= cap_lds pairs: the parallel bucket-sort resolve (three 16-bit LDS tables);
    // larger ones: one lane swapping in global memory
    const int64_t cap_lds = force_global ? 0 : std::min<int64_t>({cap, 65534, (int64_t)(kLdsBudget / 6) - 2});
    if (cap_lds > 0)
      hipLaunchKernelGGL(shuffle_sort_kernel, dim3((unsigned)n_part), dim3(kShufThreads),
                         (size_t)6 * (size_t)((cap_lds + 2) & ~1), st, P->kd_off, kp_off,
                         prm->dup, part_npairs, W.jseq, P->order, (int32_t)cap_lds, M);
    if (cap > cap_lds) {  // partitions beyond the LDS tables: swaps in global memory, then the maps
      hipLaunchKernelGGL(apply_shuffle_kernel, dim3((unsigned)n_part), dim3(64), 0, st, P->kd_off,
                         kp_off, prm->dup, part_npairs, W.jseq, P->order, cap_lds);
      hipLaunchKernelGGL(map_pairs_kernel, dim3((unsigned)n_part), dim3(256), 0, st, P->kd_off,
                         kp_off, prm->dup, M.part_base, (const int32_t*)P->order, M.src, M.slots,
                         M.dstq);
    }
  }
  LDDL_HIP(hipGetLastError());
  return 0;
}

#ifdef LDDL_STAMPS
// diagnostic build: region shares of plan_replay_kernel and the timeline of its partitions
static int report_plan_stamps(const PlanWork& W) {
  const int64_t n_part = W.n_part;
  hipStream_t st = W.st;
  std::vector<uint64_t> h(n_part * kStampRegions);
  LDDL_HIP(hipMemcpyAsync(h.data(), W.d_stamps, 8 * h.size(), hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipStreamSynchronize(st));
  double tot[kStampRegions] = {0};
  for (int64_t q = 0; q < n_part; ++q)
    for (int r = 0; r < kStampRegions; ++r) tot[r] += (double)h[q * kStampRegions + r];
  const char* names[kStampRegions] = {"plan", "cand", "shuffle_draws", "random_next", "decisions",
                                      "trunc", "final_shuffle_draws", "fy_jacobi_passes_per_window"};
  double all = 0;
  for (int r = 0; r < kStampRegions - 1; ++r) all += tot[r];
  fprintf(stderr, "[stamps] plan_replay_kernel mean cycles per partition:");
  for (int r = 0; r < kStampRegions - 1; ++r)
    fprintf(stderr, " %s=%.3g (%.1f%%)", names[r], tot[r] / n_part, 100.0 * tot[r] / (all + 1e-9));
  fprintf(stderr, " %s=%.3f\n", names[kStampRegions - 1], tot[kStampRegions - 1] / n_part / 1e6);
  // timeline (100 MHz real-time clock): partition durations and concurrency over the launch
  std::vector<uint64_t> t(2 * n_part);
  LDDL_HIP(hipMemcpyAsync(t.data(), W.d_tl, 16 * n_part, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipStreamSynchronize(st));
  uint64_t t0 = ~0ull, t1 = 0;
  std::vector<double> dur(n_part);
  for (int64_t q = 0; q < n_part; ++q) {
    t0 = std::min(t0, t[2 * q]);
    t1 = std::max(t1, t[2 * q + 1]);
    dur[q] = (t[2 * q + 1] - t[2 * q]) / 1e5;  // ms
  }
  std::vector<double> sd = dur;
  std::sort(sd.begin(), sd.end());
  const double span = (t1 - t0) / 1e5;
  fprintf(stderr, "[timeline] span %.2f ms, partition ms min %.2f p10 %.2f p50 %.2f p90 %.2f max %.2f\n",
          span, sd[0], sd[n_part / 10], sd[n_part / 2], sd[n_part * 9 / 10], sd[n_part - 1]);
  const int nb = 40;
  fprintf(stderr, "[timeline] active partitions per %.2f ms bin:", span / nb);
  for (int b = 0; b < nb; ++b) {
    const uint64_t a = t0 + (t1 - t0) * b / nb, e = t0 + (t1 - t0) * (b + 1) / nb;
    double act = 0;  // partition-time inside the bin / bin length
    for (int64_t q = 0; q < n_part; ++q) {
      const uint64_t s0 = std::max(a, t[2 * q]), s1 = std::min(e, t[2 * q + 1]);
      if (s1 > s0) act += (double)(s1 - s0);
    }
    fprintf(stderr, " %.0f", act / (double)(e - a));
  }
  fprintf(stderr, "\n[timeline] start ms of partitions by index decile:");
  for (int k = 0; k <= 10; ++k) {
    const int64_t q = std::min<int64_t>(n_part - 1, n_part * k / 10);
    fprintf(stderr, " %.1f", (t[2 * q] - t0) / 1e5);
  }
  fprintf(stderr, "\n");
  if (W.sliced) {  // the slices (one per ticket): how many waves were planning in every bin
    const int64_t n_tk = n_part + W.sl_ring_cap;
    std::vector<uint64_t> ts(2 * n_tk);
    LDDL_HIP(hipMemcpyAsync(ts.data(), W.d_tls, 16 * n_tk, hipMemcpyDeviceToHost, st));
    LDDL_HIP(hipStreamSynchronize(st));
    std::vector<double> sl;
    for (int64_t q = 0; q < n_tk; ++q)
      if (ts[2 * q + 1]) sl.push_back((ts[2 * q + 1] - ts[2 * q]) / 1e5);
    std::sort(sl.begin(), sl.end());
    if (!sl.empty())
      fprintf(stderr, "[timeline] %zu slices on %lld waves, slice ms min %.2f p50 %.2f p90 %.2f max %.2f\n",
              sl.size(), (long long)W.sl_grid, sl[0], sl[sl.size() / 2], sl[sl.size() * 9 / 10], sl.back());
    fprintf(stderr, "[timeline] active waves (slices) per %.2f ms bin:", span / nb);
    for (int b = 0; b < nb; ++b) {
      const uint64_t a = t0 + (t1 - t0) * b / nb, e = t0 + (t1 - t0) * (b + 1) / nb;
      double act = 0;
      for (int64_t q = 0; q < n_tk; ++q) {
        if (!ts[2 * q + 1]) continue;
        const uint64_t s0 = std::max(a, ts[2 * q]), s1 = std::min(e, ts[2 * q + 1]);
        if (s1 > s0) act += (double)(s1 - s0);
      }
      fprintf(stderr, " %.0f", act / (double)(e - a));
    }
    fprintf(stderr, "\n");
  }
  return 0;
}
#endif

// The mask replay (fy_resolve, planner order): every pair's mask positions, and its gather
// record and counts at its output position.
static int resolve_masks(lddl_pairs* P, PlanWork& W, const PairRange& r) {
  if (!r.n_pairs) return 0;
  const int32_t seq = P->seq;
  const FyKnobs& fy = W.fy;
  hipStream_t st = W.st;
  ResolveArgs RA{W.M.slots, r.n_pairs, P->desc, W.spool, W.jpool, P->mpos, P->kscan, P->dense,
                 P->cls_id, P->sep_id, W.M.dstq, r.rec, W.pcnt, 0};
  // a lane's column covers the padded draw region (steps up to nc rounded up to 16)
  const size_t col = (size_t)((seq + 15) & ~15);
  RA.col_rows = (int32_t)col;
  // Branch-free steps for long pairs (C3, seq 512: 77.6 -> 46.8 ms), the guarded ones at
  // seq <= 131 (64 pairs per wave: 10.1 ms against 11.5 branch-free; profiles/r05k_*).
  // A/B: LDDL_FY_MODE=0 / 1 forces one kind everywhere; LDDL_FY_LW=32: 32 pairs per wave at
  // seq > 256 (50.7 ms)
  // move-only groups at seq > 256 read one entry ahead (46.8 -> 44.4 ms; 2 ahead 45.9, 3 ahead
  // 46.7: the forwarding selects grow; profiles/r05m_*). LDDL_FY_RA=0..3 (A/B)
  // draw vectors (8 steps each) in flight per lane at seq > 256 (A/B: LDDL_FY_PF=2 / 8)
#define LDDL_FY_LAUNCH(T, NG, LW, BF, ...)                                                     \
  hipLaunchKernelGGL((fy_resolve_kernel<T, T, NG, LW, BF, ##__VA_ARGS__>),                     \
                     dim3((unsigned)((r.n_pairs + LW - 1) / LW)), dim3(LW),                   \
                     (size_t)LW * sizeof(T) * col, st, RA)
  if (seq <= 131) {  // nc <= 128: all draws in registers (8 uint4 of 1-byte draws); 64
    // pairs per wave (C2: 10.2 ms; 32 per wave 11.9, 16 per wave 20.1, profiles/r04slw_*)
    if (fy.mode == 1) LDDL_FY_LAUNCH(uint8_t, 8, 64, true);
    else LDDL_FY_LAUNCH(uint8_t, 8, 64, false);
  // long pairs: 16 lanes (pairs) per wave (C3, seq 512: 106 ms with 64, 109 with 32, 93 with
  // 16; profiles/r04fy_*)
  } else if (seq <= 256) {  // candidate indices, positions and draws fit a byte
    if (fy.mode) LDDL_FY_LAUNCH(uint8_t, 0, 16, true);
    else LDDL_FY_LAUNCH(uint8_t, 0, 16, false);
  } else if (fy.lw == 32) {
    if (fy.mode) LDDL_FY_LAUNCH(uint16_t, 0, 32, true);
    else LDDL_FY_LAUNCH(uint16_t, 0, 32, false);
  } else {
    if (!fy.mode) LDDL_FY_LAUNCH(uint16_t, 0, 16, false);
    else if (fy.ra == 1 && fy.pf == 8) LDDL_FY_LAUNCH(uint16_t, 0, 16, true, 1, 8);
    else if (fy.ra == 1 && fy.pf == 2) LDDL_FY_LAUNCH(uint16_t, 0, 16, true, 1, 2);
    else if (fy.ra == 1) LDDL_FY_LAUNCH(uint16_t, 0, 16, true, 1);
    else if (fy.ra == 2) LDDL_FY_LAUNCH(uint16_t, 0, 16, true, 2);
    else if (fy.ra == 3) LDDL_FY_LAUNCH(uint16_t, 0, 16, true, 3);
    else LDDL_FY_LAUNCH(uint16_t, 0, 16, true);
  }
#undef LDDL_FY_LAUNCH
  return 0;
}

// Layout of one range of a replay plan with masking (its pair count came with the planner's
// sync): the mask replay writes every pair's masks, and its gather record and counts at its
// output position; the two output-order scans follow.
// (Round 4 ran pair_prep beside fy_resolve on a second stream: 15.6 ms for the section, both
// kernels slowed by the other; the fused replay reads each slot record once.)
static int layout_replay(lddl_pairs* P, PlanWork& W, PairRange& r) {
  int rc;
  if ((rc = layout_alloc(P, W, r)) || (rc = resolve_masks(P, W, r))) return rc;
  LDDL_HIP(hipGetLastError());
  return layout_scan(P, W, r);
}

// Everything downstream of the planner for a one-range replay plan. Without masking, pair_prep
// builds the records from the output order.
static int finish_unsplit(lddl_pairs* P, PlanWork& W) {
  int rc;
  P->n_rg = 1;
  PairRange& r = P->rg[0];
  r = PairRange{};
  r.p1 = W.n_part;
  r.n_pairs = P->n_pairs;
  if ((rc = shuffle_partitions(P, W, r, P->part_base))) return rc;
#ifdef LDDL_STAMPS
  if ((rc = report_plan_stamps(W))) return rc;
#endif
  return P->masking ? layout_replay(P, W, r) : layout_pairs(P, W);
}

// a range's shuffle and layout temporaries, when the next range (or the re-plan) takes its own
static void give_range_tmp(PlanWork& W) {
  for (void* b : {(void*)W.M.slots, (void*)W.M.dstq, (void*)W.pcnt, (void*)W.scr2})
    if (b) W.tmp.give(b);
  W.M = PairMaps{nullptr, nullptr, nullptr, nullptr};
  W.pcnt = nullptr;
  W.scr2 = nullptr;
}

static int32_t max_predictions(const lddl_pair_params* prm) {
  if (!prm->masking) return 0;
  const int32_t m = (int32_t)rint((double)prm->seq * prm->masked_lm_ratio);
  return std::min(std::max(m, 1), prm->seq);
}

// First half of a plan: the whole plan when it is not split (native RNG, no masking, too few
// partitions); else the head range planned, resolved and laid out while the tail range's
// planner still runs on the side stream (P->work carries the call over to plan_tail_stage).
static int plan_head_stage(lddl_pairs* P, const int64_t* d_sent_off, const int32_t* d_sent_len,
                           const int64_t* d_doc_sent_off, int64_t n_doc,
                           const int64_t* d_part_doc_off) {
  PlanWork& W = *P->work;
  int rc;
  if ((rc = compact_inputs(P, W, d_sent_off, d_sent_len, d_doc_sent_off, n_doc, d_part_doc_off)))
    return rc;
  if (W.prm->rng == LDDL_RNG_NATIVE) {
    if ((rc = plan_native(P, W))) return rc;
  } else {
    if ((rc = plan_replay_setup(P, W)) || (rc = choose_slice(P, W)) || (rc = choose_split(W, &W.split)))
      return rc;
    if (!W.split) {
      if ((rc = plan_replay_unsplit(P, W, 0)) || (rc = finish_unsplit(P, W))) return rc;
    } else {
      bool usable = false;
      if ((rc = plan_replay_split_head(P, W, &usable))) return rc;
      PairRange& r = P->rg[0];
      r.p1 = W.split;
      if (usable) {
        // (the pools of this attempt stand unless the tail overflows them)
        W.jpool = W.jpool_try;
        P->mtok = W.mtok_try;
        if ((rc = shuffle_partitions(P, W, r, P->part_base)) || (rc = layout_replay(P, W, r))) return rc;
        P->head_valid = true;
      } else {
        r.n_pairs = 0;
      }
    }
  }
  LDDL_HIP(hipStreamSynchronize(W.st));  // the ranges' totals (layout_scan)
  if (!W.split) {
    P->n_tokens = P->rg[0].n_tokens;
    P->n_masked = P->rg[0].n_masked;
    P->work.reset();
  }
  return 0;
}

// Second half of a split plan: joins the tail range, then either lays it out behind the head
// (offsets carried in as the range's bases) or, when a pool overflowed, drops the head's tables
// and plans everything again in one range with the exact pool sizes.
static int plan_tail_stage(lddl_pairs* P) {
  if (!P->work) return 0;
  PlanWork& W = *P->work;
  hipStream_t st = W.st;
  const int64_t s = W.split, n_tail = W.n_part - s;
  int rc;
  P->join(st);
  LDDL_HIP(hipEventRecord(P->ev[1], st));
  LDDL_HIP(scan_exclusive(Identity{W.part_npairs + s}, n_tail, W.tail_rel, W.scratch, st));
  hipLaunchKernelGGL(max_pairs_kernel, dim3(64), dim3(256), 0, st, W.part_npairs + s, n_tail,
                     W.pool_ctl + 3);
  LDDL_HIP(hipGetLastError());
  unsigned long long ctl[4];
  PairRange &h = P->rg[0], &t = P->rg[1];
  LDDL_HIP(hipMemcpyAsync(ctl, W.pool_ctl, 32, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipMemcpyAsync(&t.n_pairs, W.tail_rel + n_tail, 8, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipStreamSynchronize(st));
  W.max_np = std::max<int64_t>(1, (int64_t)ctl[3]);
  if (ctl[1]) {  // a pool overflowed: the head's output is void; one range, exact sizes
    P->head_valid = false;
    give_range_tmp(W);
    for (void* b : {(void*)W.mtok_try, (void*)P->mpos, (void*)h.rec, (void*)h.tok_off, (void*)h.pos_off})
      if (b) P->mem.give(b);
    W.tmp.give(W.jpool_try);
    P->mtok = nullptr;
    P->mpos = nullptr;
    W.jpool = nullptr;
    h = PairRange{};
    t = PairRange{};
    W.split = 0;
    W.cap = (int64_t)ctl[0] + 1024;
    W.jcap = (int64_t)ctl[2] + 1024;
    if ((rc = plan_replay_unsplit(P, W, 1)) || (rc = finish_unsplit(P, W))) return rc;
    LDDL_HIP(hipStreamSynchronize(st));
    P->n_tokens = h.n_tokens;
    P->n_masked = h.n_masked;
  } else {
    give_range_tmp(W);
    if (n_tail)
      hipLaunchKernelGGL(tail_part_base_kernel, dim3((unsigned)((n_tail + 255) / 256)), dim3(256), 0,
                         st, W.tail_rel, n_tail, h.n_pairs, P->part_base + s);
    LDDL_HIP(hipGetLastError());
    t.p0 = s;
    t.p1 = W.n_part;
    t.pair0 = h.n_pairs;
    t.tok0 = h.n_tokens;
    t.pos0 = h.n_masked;
    P->n_rg = 2;
    if ((rc = shuffle_partitions(P, W, t, W.tail_rel)) || (rc = layout_replay(P, W, t))) return rc;
    LDDL_HIP(hipStreamSynchronize(st));
    P->n_pairs = h.n_pairs + t.n_pairs;
    P->n_tokens = h.n_tokens + t.n_tokens;
    P->n_masked = h.n_masked + t.n_masked;
  }
  P->work.reset();
  return 0;
}

static void plan_counts(const lddl_pairs* P, int64_t* counts) {
  if (!counts) return;
  counts[0] = P->n_pairs;
  counts[1] = P->n_tokens;
  counts[2] = P->n_masked;
  counts[3] = P->n_kept_sent;
  counts[4] = P->n_kept_doc;
}

extern "C" int lddl_pairs_plan_head(lddl_ctx* c, void* stream, const lddl_pair_params* prm,
                                    const int64_t* d_sent_off, const int32_t* d_ids,
                                    const int32_t* d_sent_len, int64_t n_sent,
                                    const int64_t* d_doc_sent_off, int64_t n_doc,
                                    const int64_t* d_part_doc_off, const int64_t* d_part_seed,
                                    int64_t n_part, lddl_pairs** out, int64_t* head) {
  if (out) *out = nullptr;
  FyKnobs fy;
  int64_t split_knob, slice_knob, waves_knob;
  int rc;
  if (!out) LDDL_FAIL(-1, "null argument");
  if ((rc = check_plan_args(c, prm, &fy, &split_knob, &slice_knob, &waves_knob))) return rc;
  hipStream_t st = as_stream(stream);
  // until it is handed out, an error return drops the plan: its blocks go back on `st` (after
  // the tail launch, when one is in flight)
  std::unique_ptr<lddl_pairs> P(new lddl_pairs(&c->arena, st));
  P->n_part = n_part;
  P->prm = *prm;
  P->masking = prm->masking;
  P->seq = prm->seq;
  P->cls_id = c->tab.special_id[kCls];
  P->sep_id = c->tab.special_id[kSep];
  P->max_pred = max_predictions(prm);
  LDDL_HIP(hipEventCreate(&P->ev[0]));
  LDDL_HIP(hipEventCreate(&P->ev[1]));
  P->work.reset(new PlanWork{c, &P->prm, d_ids, d_part_seed, n_sent, n_part, st, P->mem, fy, split_knob,
                              slice_knob, waves_knob});
  if ((rc = plan_head_stage(P.get(), d_sent_off, d_sent_len, d_doc_sent_off, n_doc, d_part_doc_off)))
    return rc;
  if (head) {
    for (int i = 0; i < 8; ++i) head[i] = 0;
    if (P->work) {  // split: the head's counts and what they predict for the whole plan
      const PlanWork& W = *P->work;
      const PairRange& h = P->rg[0];
      head[0] = 1;
      head[1] = h.n_pairs;
      head[2] = h.n_tokens;
      head[3] = h.n_masked;
      head[4] = plan_suggest_capacity(h.n_pairs, W.n_kept_tok, W.h_split_info[1]);
      head[5] = plan_suggest_capacity(h.n_tokens, W.n_kept_tok, W.h_split_info[1]);
      head[6] = plan_suggest_capacity(h.n_masked, W.n_kept_tok, W.h_split_info[1]);
    }
    head[7] = P->n_slices;
  }
  *out = P.release();
  return 0;
}

extern "C" int lddl_pairs_plan_tail(lddl_pairs* P, int64_t* counts, int32_t* head_valid) {
  if (!P) LDDL_FAIL(-1, "null plan");
  int rc;
  if ((rc = plan_tail_stage(P))) return rc;
  plan_counts(P, counts);
  if (head_valid) *head_valid = P->head_valid ? 1 : 0;
  return 0;
}

extern "C" int lddl_pairs_plan(lddl_ctx* c, void* stream, const lddl_pair_params* prm,
                               const int64_t* d_sent_off, const int32_t* d_ids,
                               const int32_t* d_sent_len, int64_t n_sent,
                               const int64_t* d_doc_sent_off, int64_t n_doc,
                               const int64_t* d_part_doc_off, const int64_t* d_part_seed,
                               int64_t n_part, lddl_pairs** out, int64_t* counts) {
  lddl_pairs* P = nullptr;
  int rc;
  if (out) *out = nullptr;
  if ((rc = lddl_pairs_plan_head(c, stream, prm, d_sent_off, d_ids, d_sent_len, n_sent, d_doc_sent_off,
                                 n_doc, d_part_doc_off, d_part_seed, n_part, &P, nullptr)))
    return rc;
  if ((rc = lddl_pairs_plan_tail(P, counts, nullptr))) {
    delete P;  // (joins, then its blocks go back on the planning stream)
    return rc;
  }
  *out = P;
  return 0;
}

// Gathers the plan's ranges [r0, r1) into the caller's buffers (whole-plan indexing).
static int emit_ranges(lddl_pairs* P, int r0, int r1, void* stream, void* d_tokens, int64_t* d_tok_off,
                       int32_t* d_len_a, uint8_t* d_is_rn, uint16_t* d_pos, void* d_lab,
                       int64_t* d_pos_off) {
  hipStream_t st = as_stream(stream);
  for (int ri = r0; ri < r1; ++ri) {
    const PairRange& r = P->rg[ri];
    if (r.n_pairs == 0) continue;
    GatherArgs G{};
    G.dense = P->dense.p;
    G.rec = r.rec;
    G.mpos = P->mpos;
    G.mtok = P->mtok;
    G.masking = P->masking;
    G.n_pairs = r.n_pairs;
    G.tok_off = r.tok_off;
    G.pos_off = r.pos_off;
    G.tok_base = r.tok0;
    G.pos_base = r.pos0;
    G.out_tok = d_tokens;
    G.len_a = d_len_a + r.pair0;
    G.is_rn = d_is_rn + r.pair0;
    G.out_pos = d_pos;
    G.out_lab = d_lab;
    G.out_tok_off = d_tok_off ? d_tok_off + r.pair0 : nullptr;
    G.out_pos_off = d_pos_off ? d_pos_off + r.pair0 : nullptr;
    GatherLds Lg{(P->seq + 127) / 128 * 128, P->dense.ib, P->dense.ib == 2 && P->seq <= 600 ? 2 : 4};
    auto launch = [&](auto kern, int K) {
      const int64_t per_wg = (int64_t)2 * K * kGWaves;
      const int64_t nwg = (r.n_pairs + per_wg - 1) / per_wg;
      const int64_t gx = std::min<int64_t>(nwg, 65536);
      const size_t lds = P->masking ? (size_t)kGWaves * 2 * K * Lg.per_pair() : 0;
      hipLaunchKernelGGL(kern, dim3((unsigned)gx, (unsigned)((nwg + gx - 1) / gx)), dim3(64 * kGWaves),
                         lds, st, G, Lg);
    };
    const bool i16 = P->dense.ib == 2;
    if (P->seq <= 600) {
      if (i16) launch(gather16_kernel<16>, 2);  // (4 pairs per wave, like K = 2; LP = 8: 35.3 ms, r04ze)
      else launch(gather_kernel<2, int32_t>, 2);
    } else {  // (LDS: seq-entry decision tables)
      if (i16) launch(gather_kernel<1, uint16_t>, 1);
      else launch(gather_kernel<1, int32_t>, 1);
    }
    LDDL_HIP(hipGetLastError());
  }
  return 0;
}

extern "C" int lddl_pairs_emit(lddl_pairs* P, void* stream, void* d_tokens, int64_t* d_tok_off,
                               int32_t* d_len_a, uint8_t* d_is_rn, uint16_t* d_pos, void* d_lab,
                               int64_t* d_pos_off) {
  if (!P) LDDL_FAIL(-1, "null plan");
  if (P->work) LDDL_FAIL(-1, "lddl_pairs_emit before lddl_pairs_plan_tail");
  return emit_ranges(P, 0, P->n_rg, stream, d_tokens, d_tok_off, d_len_a, d_is_rn, d_pos, d_lab,
                     d_pos_off);
}

extern "C" int lddl_pairs_emit_head(lddl_pairs* P, void* stream, void* d_tokens, int64_t* d_tok_off,
                                    int32_t* d_len_a, uint8_t* d_is_rn, uint16_t* d_pos, void* d_lab,
                                    int64_t* d_pos_off) {
  if (!P) LDDL_FAIL(-1, "null plan");
  if (!P->work) LDDL_FAIL(-1, "lddl_pairs_emit_head: not a split plan between its head and tail calls");
  if (!P->head_valid) return 0;  // (a pool overflowed: lddl_pairs_plan_tail will say so)
  return emit_ranges(P, 0, 1, stream, d_tokens, d_tok_off, d_len_a, d_is_rn, d_pos, d_lab, d_pos_off);
}

extern "C" int lddl_pairs_emit_tail(lddl_pairs* P, void* stream, void* d_tokens, int64_t* d_tok_off,
                                    int32_t* d_len_a, uint8_t* d_is_rn, uint16_t* d_pos, void* d_lab,
                                    int64_t* d_pos_off) {
  if (!P) LDDL_FAIL(-1, "null plan");
  if (P->work || P->n_rg != 2 || !P->head_valid)
    LDDL_FAIL(-1, "lddl_pairs_emit_tail: no valid head range (use lddl_pairs_emit)");
  return emit_ranges(P, 1, 2, stream, d_tokens, d_tok_off, d_len_a, d_is_rn, d_pos, d_lab, d_pos_off);
}

extern "C" int lddl_pairs_destroy(lddl_pairs* P, void* stream) {
  if (!P) return 0;
  P->join(as_stream(stream));  // (a split plan dropped before its tail call)
  P->mem.release(as_stream(stream));  // (the last use of the blocks was on this stream)
  delete P;
  return 0;
}

extern "C" int lddl_pairs_plan_ms(const lddl_pairs* P, float* ms) {
  if (!P || !ms) LDDL_FAIL(-1, "null argument");
  *ms = 0.f;
  if (P->n_part && P->ev[0]) LDDL_HIP(hipEventElapsedTime(ms, P->ev[0], P->ev[1]));
  return 0;
}

extern "C" int lddl_pairs_part_offsets(lddl_pairs* P, void* stream, int64_t* d_part_pair_off) {
  if (!P || !d_part_pair_off) LDDL_FAIL(-1, "null argument");
  LDDL_HIP(hipMemcpyAsync(d_part_pair_off, P->part_base, 8 * (P->n_part + 1),
                          hipMemcpyDeviceToDevice, as_stream(stream)));
  return 0;
}
