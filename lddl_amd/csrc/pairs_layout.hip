// Pair stage, layout and mask replay: every output pair's gather record, the output-order scans
// of token and mask counts, and (replay plans with masking) the masked positions from the
// planner's recorded shuffle draws.
#include "pairs_plan.h"

namespace lddl {
namespace {

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

}  // namespace

// The gather records + output-order scans (tok_off, pos_off) of the plan's pairs.
// (of one range; W.rt.pcnt / W.rt.scr2 are the range's temporaries)
static int layout_alloc(lddl_pairs* P, PlanWork& W, PairRange& r) {
  const int64_t npairs = r.n_pairs;
  int rc;
  if ((rc = P->mem.take(&r.tok_off, npairs + 1)) || (rc = P->mem.take(&r.rec, npairs)) ||
      (rc = W.tmp.take(&W.rt.pcnt, npairs)) || (rc = W.tmp.take(&W.rt.scr2, 2 * scan_scratch_elems(npairs))))
    return rc;
  if (P->masking && (rc = P->mem.take(&r.pos_off, npairs + 1))) return rc;
  return 0;
}

// tok_off (and pos_off) from the counts, then the range's totals (read with the caller's sync)
static int layout_scan(lddl_pairs* P, PlanWork& W, PairRange& r) {
  if (P->masking)
    LDDL_HIP(scan_exclusive2(PairCounts{W.rt.pcnt}, r.n_pairs, r.tok_off, r.pos_off, W.rt.scr2, W.st));
  else
    LDDL_HIP(scan_exclusive(PairTokens{W.rt.pcnt}, r.n_pairs, r.tok_off, W.rt.scr2, W.st));
  LDDL_HIP(hipMemcpyAsync(&r.n_tokens, r.tok_off + r.n_pairs, 8, hipMemcpyDeviceToHost, W.st));
  if (P->masking)
    LDDL_HIP(hipMemcpyAsync(&r.n_masked, r.pos_off + r.n_pairs, 8, hipMemcpyDeviceToHost, W.st));
  return 0;
}

// gather records from the output order (src): the native path, and replay without masking
int layout_pairs(lddl_pairs* P, PlanWork& W) {
  int rc;
  PairRange& r = P->rg[0];  // (always one range)
  r.p1 = P->n_part;
  r.n_pairs = P->n_pairs;
  if ((rc = layout_alloc(P, W, r))) return rc;
  const int64_t npairs = P->n_pairs;
  if (npairs)
    hipLaunchKernelGGL(pair_prep_kernel, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, W.st,
                       P->src, npairs, P->desc, P->kscan, P->masking ? P->nmask : nullptr,
                       P->moff, r.rec, W.rt.pcnt);
  LDDL_HIP(hipGetLastError());
  return layout_scan(P, W, r);
}

// The mask replay (fy_resolve, planner order): every pair's mask positions, and its gather
// record and counts at its output position.
static int resolve_masks(lddl_pairs* P, PlanWork& W, const PairRange& r) {
  if (!r.n_pairs) return 0;
  const int32_t seq = P->seq;
  const FyKnobs& fy = W.knobs.fy;
  hipStream_t st = W.st;
  ResolveArgs RA{W.rt.M.slots, r.n_pairs, P->desc, W.spool, W.jpool, P->mpos, P->kscan, P->dense,
                 P->cls_id, P->sep_id, W.rt.M.dstq, r.rec, W.rt.pcnt, 0};
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
int layout_replay(lddl_pairs* P, PlanWork& W, PairRange& r) {
  int rc;
  if ((rc = layout_alloc(P, W, r)) || (rc = resolve_masks(P, W, r))) return rc;
  LDDL_HIP(hipGetLastError());
  return layout_scan(P, W, r);
}

}  // namespace lddl
