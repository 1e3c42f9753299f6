// Pair stage, the native planner's masking (LDDL_RNG_NATIVE; the stage's other units: file map in
// pairs_api.hip): mask_native_kernel (plain) and mask_ww_native_kernel (whole word) with their
// wave helpers, and the one host function that launches whichever applies, in the shape that
// native_shape.h gives.
#include "collate_dev.h"  // ContBits, cont_id
#include "native_dev.h"
#include "native_shape.h"

namespace lddl {
namespace {

// 80 / 10 / 10 of create_masked_lm_predictions (pretrain.py:214-229) on one 32-bit draw:
// [MASK] below ceil(0.8 * 2^32), the original token below ceil(0.9 * 2^32), else a random token.
constexpr uint32_t kNat80 = 3435973837u, kNat90 = 3865470567u;

// Masked positions of ppw consecutive pairs per wave (one lane per pair; 64, or fewer where the
// staged masks of 64 pairs exceed the LDS budget, the lanes above ppw idle), in lock step so that
// every lane's Philox refill comes at the same iteration:
//  1. Floyd's sampling of num candidate indices out of nc (a uniform num-subset: the shuffled
//     prefix of pretrain.py:197-207), one draw per step, into a lane-private LDS bitmap;
//  2. the set bits in ascending order (= sorted(masked_lms, key=index)), each with an 80/10/10
//     decision from its own stream (two draws per mask, whatever the decision), staged in LDS;
//  3. the wave's masks are one contiguous run of the pool (moff is the planner-order scan), copied
//     out with coalesced stores.
// Every draw's stream position depends on the pair alone (the sampling and the decisions use
// separate streams), so a pair's masks do not depend on the pairs that share its wave.
__global__ void __launch_bounds__(256) mask_native_kernel(NativeArgs A, int32_t stage_cap, int32_t ppw) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_mn[];
  const int w = wave_id(), lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  const int64_t q0 = ((int64_t)blockIdx.x * nw + w) * ppw;
  if (q0 >= A.n_pairs) return;
  uint32_t* bm = reinterpret_cast<uint32_t*>(s_mn) + (size_t)w * A.words * 64 + lane;
  int32_t* stok = reinterpret_cast<int32_t*>(s_mn + (size_t)nw * A.words * 64 * 4) + (size_t)w * stage_cap;
  uint16_t* spos = reinterpret_cast<uint16_t*>(s_mn + (size_t)nw * A.words * 64 * 4 +
                                                (size_t)nw * stage_cap * 4) + (size_t)w * stage_cap;
  const int64_t q = q0 + lane;
  const bool valid = lane < ppw && q < A.n_pairs;
  const int64_t qv = valid ? q : q0;
  const int64_t qe = q0 + ppw < A.n_pairs ? q0 + ppw : A.n_pairs;
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
// no such mode, so it exists with LDDL_RNG_NATIVE only. (Its streams: kStreamWordKey and
// kStreamWordDecide, native_dev.h; a token's draws: token_rng there.)
// ---------------------------------------------------------------------------------------------

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

}  // namespace

void launch_native_masks(const lddl_pairs* P, const PlanWork& W, NativeArgs& A) {
  const MaskShape m = native_mask_shape(W.prm->seq, P->max_pred);
  A.words = m.words;
  if (!A.n_pairs) return;
  if (!W.prm->whole_word) {
    hipLaunchKernelGGL(mask_native_kernel, dim3(m.grid(A.n_pairs)), dim3(m.threads()), m.lds_bytes(), W.st,
                       A, m.stage_cap, m.ppw);
  } else {
    const WwShape w = native_ww_shape(W.prm->seq);
    hipLaunchKernelGGL(mask_ww_native_kernel, dim3(w.grid(A.n_pairs)), dim3(w.threads()), w.lds_bytes(),
                       W.st, A, ContBits{W.c->d_cont_bits, W.c->vocab_size}, w.seqp);
  }
}

}  // namespace lddl
