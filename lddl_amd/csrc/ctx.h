// Host-side context: device copies of the normaliser table and the vocab hash.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "arena.h"
#include "device.h"
struct lddl_punkt_state;  // punkt_state.h
struct lddl_bart_state;   // bart.hip
struct lddl_ctx {
  int device = 0;
  lddl::Tables tab{};
  // owned device allocations
  uint16_t* d_l1 = nullptr;
  uint32_t* d_pages = nullptr;
  uint8_t* d_pool = nullptr;
  lddl::VEnt* d_vhash = nullptr;
  uint8_t* d_vbytes = nullptr;
  int64_t* d_voff = nullptr;
  uint8_t* d_render = nullptr;      // full token strings (as in vocab.txt, "##" kept)
  int64_t* d_render_off = nullptr;  // token i = d_render[off[i] .. off[i+1])
  uint32_t* d_bloom = nullptr;
  uint64_t* d_vlong = nullptr;
  // one bit per id: the vocab line is a continuation piece ("##" and more). Whole-word masking
  // only (collate.hip); not part of Tables
  uint32_t* d_cont_bits = nullptr;
  int32_t vocab_size = 0;
  // bytes per token id in the pair tables (dense kept tokens, sample tokens, labels): 2 when every
  // id fits uint16 with two values to spare for the gather's decision table (vocab_size <=
  // 65,534: BERT's uncased 30,522 and cased 28,996), else 4
  int32_t id_bytes() const { return vocab_size <= 65534 ? 2 : 4; }
  size_t lds_per_block = 0;         // hipDeviceAttributeMaxSharedMemoryPerBlock of `device`
  std::vector<std::string> tokens;  // host copy of the vocab lines
  lddl::DevArena arena;             // per-call temporaries (pair plans)
  lddl_punkt_state* punkt = nullptr;  // created by lddl_punkt_set_params (punkt.hip)
  lddl_bart_state* bart = nullptr;    // created by lddl_bart_count (bart.hip)
  // the pair planner's side stream (pairs.hip: the tail range of a split plan), created on first
  // use: non-blocking, lowest priority
  hipStream_t plan_side = nullptr;
};
extern "C" void lddl_punkt_release(lddl_ctx* c);
extern "C" void lddl_bart_release(lddl_ctx* c);

namespace lddl {
inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
// device copy of a host array (at least 16 bytes, so never null); *dst owns it, also when the
// copy fails
template <typename T>
int upload(T** dst, const void* src, size_t bytes) {
  LDDL_HIP(hipMalloc((void**)dst, bytes ? bytes : 16));
  if (bytes) LDDL_HIP(hipMemcpy((void*)*dst, src, bytes, hipMemcpyHostToDevice));
  return 0;
}
// the character class table of lddl_punkt_set_params (punkt_classes.h); false if it was never set
struct ClassTab;
bool punkt_class_tab(const lddl_ctx* c, ClassTab* out);
}  // namespace lddl
