// The replay planner's random numbers (pairs.hip): CPython's MT19937 executed wave-uniformly, with
// the draws of the reference's loops (random.shuffle, _truncate_seq_pair, the mask decisions)
// resolved a window of words at a time. Device code of one unit (anonymous namespace).
#pragma once
#include <type_traits>

#include "pairs_plan.h"

namespace lddl {
namespace {

// ---------------------------------------------------------------------------------------------
// Wave-uniform CPython MT19937 (Modules/_randommodule.c).
// Raw state and the tempered 624-word block live in LDS; draws are served from a register
// window (lane l holds word wbase+l) through readlane, so a draw costs a few instructions.
// Every lane executes the same sequential algorithm with identical scalars (uniform control
// flow); only parallel phases (twist, temper, speculative shuffle draws) use the lanes.
// ---------------------------------------------------------------------------------------------
constexpr int kN = 624, kM = 397;
constexpr int kLook = 64;  // MT words of look-ahead past the block (WaveRng)

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
      // One body for both kinds of window. tail: the window reaches past the last step; its
      // words there (u <= 1) are held "accepted", so they settle at once.
      auto settle = [&](auto tail) {
        auto pass = [&]() {
          const int32_t u = u1 + R;
          if constexpr (decltype(tail)::value) x = w >> (__clz((uint32_t)u) & 31);
          else x = w >> __clz((uint32_t)u);
#ifdef LDDL_STAMPS
          ++n_pass;
#endif
          if constexpr (decltype(tail)::value) return ballot(x >= (uint32_t)u) & ballot(u > 1);
          else return ballot(x >= (uint32_t)u);
        };
        uint64_t prev = pass();
        R = (int32_t)popc_below(prev);
        rej = pass();
        while (rej != prev) {
          prev = rej;
          R = (int32_t)popc_below(rej);
          rej = pass();
        }
      };
      if (s0 >= 64) settle(std::false_type{});  // every word of the window has a step (u >= 2)
      else settle(std::true_type{});
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

}  // namespace
}  // namespace lddl
