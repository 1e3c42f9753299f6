// Pair stage, gather: the data plane. Copies every output pair's A and B windows from the dense
// tokens, applying the mask decisions and emitting positions and labels.
#include "pairs_plan.h"

namespace lddl {
namespace {

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

// Gathers the plan's ranges [r0, r1) into the caller's buffers (whole-plan indexing).
int emit_ranges(lddl_pairs* P, int r0, int r1, void* stream, void* d_tokens, int64_t* d_tok_off,
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

}  // namespace lddl
