// SentencePiece unigram, the normaliser and byte fallback: the entry points that
// set them on an lddl_unigram, and lddl_unigram_normalize_plan / _write. The plan keeps its
// per-tile temporaries (17 bytes per 64 bytes of text, from the handle's arena) until the next
// plan or the handle's end, because the write reads them. No host wait in either.
#include "common.h"
#include "ctx.h"
#include "lddl_amd.h"
#include "scan.h"
#include "unigram_norm.h"

using namespace lddl;

static_assert(kNormMaxKey == LDDL_UNIGRAM_NORM_MAX_KEY, "the header's constant is the kernels'");

namespace lddl {
void unigram_norm_free(lddl_unigram* u) {
  (void)hipFree(u->d_nslots);
  (void)hipFree(u->d_nroot);
  (void)hipFree(u->d_nrule);
  (void)hipFree(u->d_nrepl);
  (void)hipFree(u->d_npair);
  u->d_npair = nullptr;
  u->d_nslots = u->d_nroot = nullptr;
  u->d_nrule = nullptr;
  u->d_nrepl = nullptr;
  u->norm = NormTables{};
  u->n_rules = 0;
  u->max_repl = 0;
}
}  // namespace lddl

extern "C" int lddl_unigram_set_normalizer(lddl_unigram* u, const uint8_t* key_blob, const int64_t* key_off,
                                           const uint8_t* repl_blob, const int64_t* repl_off, int64_t n_rules) {
  if (!u) LDDL_FAIL(-1, "null unigram");
  if (n_rules < 0) LDDL_FAIL(-1, "negative size");
  NormHostTables H;
  if (n_rules > 0) {
    if (!repl_blob) LDDL_FAIL(-1, "null normaliser table");
    if (unigram_norm_build_tables(key_blob, key_off, repl_off, n_rules, &H)) return -1;
  }
  LDDL_HIP(hipSetDevice(u->device));
  LDDL_HIP(hipDeviceSynchronize());  // no call in flight reads the tables that go
  u->plan.reset();
  unigram_norm_free(u);
  if (n_rules == 0) return 0;
  int st = upload(&u->d_nslots, H.slots.data(), H.slots.size() * sizeof(UniSlot));
  st = st ? st : upload(&u->d_nroot, H.root, sizeof(H.root));
  st = st ? st : upload(&u->d_nrule, H.rule.data(), H.rule.size() * sizeof(NormRule));
  st = st ? st : upload(&u->d_nrepl, repl_blob, (size_t)repl_off[n_rules]);
  st = st ? st : upload(&u->d_npair, H.pair.data(), H.pair.size() * sizeof(uint64_t));
  if (st) {
    unigram_norm_free(u);
    return st;
  }
  u->norm = NormTables{u->d_nslots, u->d_nroot, u->d_nrule, u->d_nrepl, u->d_npair,
                       {H.start[0], H.start[1], H.start[2], H.start[3]},
                       {H.single[0], H.single[1], H.single[2], H.single[3]},
                       (uint32_t)H.slots.size() - 1, H.max_key};
  u->n_rules = n_rules;
  u->max_repl = H.max_repl;
  return 0;
}

extern "C" int lddl_unigram_set_byte_pieces(lddl_unigram* u, const int32_t* ids256) {
  if (!u) LDDL_FAIL(-1, "null unigram");
  std::vector<uint32_t> bits = u->cont_host;
  if (ids256)
    for (int b = 0; b < 256; ++b) {
      if (ids256[b] < 0 || ids256[b] >= u->n_pieces)
        LDDL_FAIL(-1, "byte piece 0x%02X: id %d outside the vocabulary", b, ids256[b]);
      bits[(size_t)ids256[b] >> 5] |= 1u << (ids256[b] & 31);  // never the first piece of a word
    }
  LDDL_HIP(hipSetDevice(u->device));
  LDDL_HIP(hipDeviceSynchronize());
  (void)hipFree(u->d_byte_ids);
  u->d_byte_ids = nullptr;
  LDDL_HIP(hipMemcpy(u->d_cont_bits, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  if (ids256 && upload(&u->d_byte_ids, ids256, 256 * sizeof(int32_t))) return -100;
  return 0;
}

extern "C" int lddl_unigram_norm_info(const lddl_unigram* u, int64_t* n_rules, int32_t* max_key,
                                      int32_t* max_repl, int32_t* byte_fallback) {
  if (!u) LDDL_FAIL(-1, "null unigram");
  if (n_rules) *n_rules = u->n_rules;
  if (max_key) *max_key = u->norm.max_key;
  if (max_repl) *max_repl = u->max_repl;
  if (byte_fallback) *byte_fallback = u->d_byte_ids != nullptr;
  return 0;
}

extern "C" int lddl_unigram_normalize_plan(lddl_unigram* u, void* stream, const uint8_t* d_text, int64_t n_bytes,
                                           const int64_t* d_sent_off, int64_t n_sent, int64_t* d_out_sent_off) {
  if (!u) LDDL_FAIL(-1, "null unigram");
  if (!u->norm.rule) LDDL_FAIL(-1, "no normaliser is set");
  if (n_bytes < 0 || n_sent < 0) LDDL_FAIL(-1, "negative size");
  if ((n_bytes && !d_text) || !d_sent_off || !d_out_sent_off) LDDL_FAIL(-1, "null argument");
  hipStream_t st = as_stream(stream);
  if (!u->h_total) LDDL_HIP(hipHostMalloc((void**)&u->h_total, sizeof(int64_t), hipHostMallocDefault));
  if (!u->plan_done) LDDL_HIP(hipEventCreateWithFlags(&u->plan_done, hipEventDisableTiming));
  u->plan.reset(new ArenaScope(&u->arena, st));
  NormWork W{};
  W.text = d_text;
  W.n_bytes = n_bytes;
  W.n_tiles = (n_bytes + 63) / 64;
  W.sent_off = d_sent_off;
  W.n_sent = n_sent;
  // 64-bit words: sent_bits (n_tiles + 2), tile_base (n_tiles + 1), the scan's scratch; then
  // info and count (32 bits a tile) and entry (8)
  const int64_t nt = W.n_tiles, scratch = scan_scratch_elems(nt);
  uint64_t* base;
  if (u->plan->take(&base, (nt + 2) + (nt + 1) + scratch) || u->plan->take(&W.info, 2 * nt) ||
      u->plan->take(&W.entry, nt)) {
    u->plan.reset();
    return -100;
  }
  W.sent_bits = base;
  W.tile_base = reinterpret_cast<int64_t*>(base + nt + 2);
  W.count = reinterpret_cast<int32_t*>(W.info + nt);
  u->plan_work = W;
  u->plan_stream = st;
  LDDL_HIP(unigram_norm_launch_plan(u->norm, W, W.tile_base + nt + 1, d_out_sent_off, st));
  LDDL_HIP(hipMemcpyAsync(u->h_total, W.tile_base + nt, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipEventRecord(u->plan_done, st));
  return 0;
}

extern "C" int lddl_unigram_normalize_write(lddl_unigram* u, void* stream, const uint8_t* d_text, int64_t n_bytes,
                                            const int64_t* d_sent_off, int64_t n_sent,
                                            const int64_t* d_out_sent_off, uint8_t* d_out_text, int64_t out_cap) {
  if (!u) LDDL_FAIL(-1, "null unigram");
  if (n_bytes < 0 || n_sent < 0 || out_cap < 0) LDDL_FAIL(-1, "negative size");
  if ((n_bytes && !d_text) || !d_sent_off || !d_out_sent_off || (out_cap && !d_out_text)) LDDL_FAIL(-1, "null argument");
  const NormWork& W = u->plan_work;
  if (!u->plan || W.text != d_text || W.n_bytes != n_bytes || W.sent_off != d_sent_off || W.n_sent != n_sent)
    LDDL_FAIL(-1, "lddl_unigram_normalize_plan was not the call before, on the same text and sentences");
  if (as_stream(stream) != u->plan_stream)  // the plan's temporaries go back to the arena on its stream
    LDDL_FAIL(-1, "lddl_unigram_normalize_write must run on its plan's stream");
  // the planned size is on the host once the caller has waited for the plan (it has, if it sized
  // out_text by it); no wait here
  if (hipEventQuery(u->plan_done) == hipSuccess && out_cap < *u->h_total)
    LDDL_FAIL(-1, "out_cap %lld is below the planned size %lld", (long long)out_cap, (long long)*u->h_total);
  (void)hipGetLastError();  // hipErrorNotReady of the query is no error
  LDDL_HIP(unigram_norm_launch_write(u->norm, W, d_out_text, out_cap, as_stream(stream)));
  return 0;
}

extern "C" int lddl_unigram_normalize_stats(lddl_unigram* u, void* stream, int64_t* d_stats) {
  if (!u || !d_stats) LDDL_FAIL(-1, "null argument");
  if (!u->plan) LDDL_FAIL(-1, "no plan");
  if (as_stream(stream) != u->plan_stream) LDDL_FAIL(-1, "lddl_unigram_normalize_stats must run on its plan's stream");
  LDDL_HIP(unigram_norm_launch_stats(u->plan_work, d_stats, u->plan_stream));
  return 0;
}

extern "C" int lddl_unigram_cont_bits_host(const lddl_unigram* u, uint32_t* bits) {
  if (!u || !bits) LDDL_FAIL(-1, "null argument");
  LDDL_HIP(hipSetDevice(u->device));
  LDDL_HIP(hipMemcpy(bits, u->d_cont_bits, u->cont_host.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return 0;
}
