// What the host sides of the tokenizer's units share (unit map: tokenize.hip): the arguments of
// one lddl_tokenize call and the launchers that tokenize_api.hip calls. Kernels and their device
// helpers are private to their unit; each launcher is defined in the unit of the kernel it
// launches.
#pragma once
#include <cstdint>

#include "common.h"
#include "ctx.h"
#include "device.h"
#include "lddl_amd.h"
#include "tok_knobs.h"

namespace lddl {

constexpr int kFbHead = 1;  // fallback list: [0] = count, then sentence indices

// The arguments of one lddl_tokenize call, as its launches share them.
struct TokCall {
  lddl_ctx* c;
  hipStream_t st;
  const uint8_t* d_text;
  int64_t n_bytes;
  const int64_t* d_sent_off;
  int64_t n_sent;
  int32_t max_pieces;
  int32_t* d_ids;
  int32_t* d_sent_len;
  int32_t* fb = nullptr;         // the fallback list
  int32_t* chunk_ctr = nullptr;  // the batch kernel's chunk counter (after the list)
  int64_t n_cu = 256;
  int64_t grid_of[2] = {0, 0};  // the streaming launches' workgroups by diagnostic slice (0: none)
  TokKnobs knobs;
};

// The word memo of a call (tokenize.hip): which of its two launches a streaming pass is, and
// the table, which belongs to the call.
enum : int { kMemoOff = 0, kMemoBuild = 1, kMemoLookup = 2 };
// 4 M entries x 64 B = 256 MiB (2 M: 15.49 ms per 2 GB, 1 M: 15.83, 4 M: 15.25 — fewer words
// lose their slot to another; profiles/r06m_tok_memo_tuning.txt)
constexpr int kMemoLog2 = 22;
struct WordMemo {
  uint4* tab;  // entry e: tab[4e], tab[4e+1] key bytes 0..31 (zero past nb), tab[4e+2] pieces
               // (8 x uint16), tab[4e+3].x meta: kMemoReady | nb | npc << 8 (0: empty)
  uint32_t mask;
};

// tokenize_lane.hip: the lane kernel over sentences [s0, s0 + n): those on the fallback list, or
// all of them (whole) on a grid of at most grid_cap workgroups
int launch_lane(const TokCall& T, int64_t s0, int64_t n, int64_t grid_cap, bool whole);
// tokenize_wave.hip (diagnostics): one sentence per wavefront, then its fallback list
int tokenize_wave(const TokCall& T);
// tokenize.hip: the resident workgroups of the streaming kernel, and one launch of it over
// sentences [s0, s0 + n) followed by the lane kernel for its fallback list
int batch_grid_max(const TokCall& T, int64_t* grid_max);
int batch_pass(TokCall& T, int64_t grid_max, int64_t s0, int64_t n, int memo, WordMemo M);
#ifdef LDDL_STAMPS
// tokenize.hip, diagnostic build: the streaming kernel's wave timelines (tl) and region counters
// (rg), one slice per launch of the call
int stamps_begin(ArenaScope& diag, const TokCall& T, int64_t grid_max, unsigned long long** tl,
                 unsigned long long** rg);
int report_tok_stamps(const TokCall& T, const unsigned long long* tl, const unsigned long long* rg);
#endif

}  // namespace lddl
