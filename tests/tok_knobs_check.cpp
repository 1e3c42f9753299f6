// CPU check of the tokenizer's environment knobs (csrc/tok_knobs.h): every accepted value, every
// rejected value and the message it is rejected with, and the word memo's sample size at its
// boundaries. Built with AddressSanitizer + UBSan together with csrc/errors.cpp by
// tests/test_tok_knobs.py; exits non-zero on the first failed expectation.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>

#include "lddl_amd.h"
#include "tok_knobs.h"

using namespace lddl;

#define EXPECT(c)                                                    \
  do {                                                               \
    if (!(c)) {                                                      \
      fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

static const char* const kAll[] = {"LDDL_TOKENIZE_PATH", "LDDL_TOKENIZE_SLOW", "LDDL_TOKENIZE_GRID",
                                   "LDDL_TOKENIZE_MEMO_SAMPLE"};

struct Knobs {
  int rc;
  TokKnobs k;
};

// the knobs as a call would read them with the environment {name = value, ...} (null: unset)
static Knobs read_with(const char* n0, const char* v0, const char* n1 = nullptr, const char* v1 = nullptr) {
  for (const char* k : kAll) unsetenv(k);
  if (n0 && v0) setenv(n0, v0, 1);
  if (n1 && v1) setenv(n1, v1, 1);
  Knobs r;
  r.k.path = kTokLane, r.k.slow_loop = 99, r.k.grid_cap = 99, r.k.sample = 99;
  r.rc = read_tok_knobs(&r.k);
  return r;
}

static bool rejected(const Knobs& r, const std::string& msg) {
  return r.rc == -1 && msg == lddl_last_error();
}

static bool defaults_but(const TokKnobs& k, TokPath path, int32_t slow_loop, int64_t grid_cap, int64_t sample) {
  return k.path == path && k.slow_loop == slow_loop && k.grid_cap == grid_cap && k.sample == sample;
}

static const char kGridMsg[] = "LDDL_TOKENIZE_GRID must be a workgroup count >= 1";
static const char kSampleMsg[] = "LDDL_TOKENIZE_MEMO_SAMPLE must be a sentence count >= 0";
static std::string path_msg(const char* v) {
  return std::string("LDDL_TOKENIZE_PATH must be lane, wave, fused or plain (got ") + v + ")";
}
static std::string slow_msg(const char* v) {
  return std::string("LDDL_TOKENIZE_SLOW must be regs or loop (got ") + v + ")";
}

// memo_sample with LDDL_TOKENIZE_MEMO_SAMPLE = sample (-1: unset) and the path
static int64_t sample_of(int64_t n_sent, int32_t vocab, int64_t sample = -1, TokPath path = kTokFused) {
  TokKnobs k;
  k.sample = sample;
  k.path = path;
  return memo_sample(n_sent, vocab, k);
}

int main() {
  // ---- nothing set: the streaming kernel with the memo, units from registers, no grid cap ----
  {
    const Knobs r = read_with(nullptr, nullptr);
    EXPECT(r.rc == 0 && defaults_but(r.k, kTokFused, 0, INT64_MAX, -1));
  }
  // ---- LDDL_TOKENIZE_PATH: four names ----
  const struct {
    const char* name;
    TokPath path;
  } paths[] = {{"lane", kTokLane}, {"wave", kTokWave}, {"fused", kTokFused}, {"plain", kTokPlain}};
  for (const auto& p : paths) {
    const Knobs r = read_with("LDDL_TOKENIZE_PATH", p.name);
    EXPECT(r.rc == 0 && defaults_but(r.k, p.path, 0, INT64_MAX, -1));
  }
  for (const char* bad : {"cp", "", "Lane", "fused ", "batch"})
    EXPECT(rejected(read_with("LDDL_TOKENIZE_PATH", bad), path_msg(bad)));
  // ---- LDDL_TOKENIZE_SLOW: regs or loop ----
  EXPECT(defaults_but(read_with("LDDL_TOKENIZE_SLOW", "regs").k, kTokFused, 0, INT64_MAX, -1));
  {
    const Knobs r = read_with("LDDL_TOKENIZE_SLOW", "loop");
    EXPECT(r.rc == 0 && defaults_but(r.k, kTokFused, 1, INT64_MAX, -1));
  }
  for (const char* bad : {"fast", "", "1", "loops"})
    EXPECT(rejected(read_with("LDDL_TOKENIZE_SLOW", bad), slow_msg(bad)));
  // (a bad value is rejected whatever the path, the lane kernel's included)
  EXPECT(rejected(read_with("LDDL_TOKENIZE_PATH", "lane", "LDDL_TOKENIZE_SLOW", "fast"), slow_msg("fast")));
  // ---- LDDL_TOKENIZE_GRID: a whole decimal number >= 1 ----
  for (int64_t v : {int64_t(1), int64_t(3), int64_t(256), int64_t(1) << 40}) {
    const Knobs r = read_with("LDDL_TOKENIZE_GRID", std::to_string(v).c_str());
    EXPECT(r.rc == 0 && defaults_but(r.k, kTokFused, 0, v, -1));
  }
  for (const char* bad : {"0", "-1", "abc", "3x", "", "1.5", "0x10"})
    EXPECT(rejected(read_with("LDDL_TOKENIZE_GRID", bad), kGridMsg));
  // ---- LDDL_TOKENIZE_MEMO_SAMPLE: a whole decimal number >= 0 ----
  for (int64_t v : {int64_t(0), int64_t(1), int64_t(64), int64_t(1000), int64_t(1) << 40}) {
    const Knobs r = read_with("LDDL_TOKENIZE_MEMO_SAMPLE", std::to_string(v).c_str());
    EXPECT(r.rc == 0 && defaults_but(r.k, kTokFused, 0, INT64_MAX, v));
  }
  for (const char* bad : {"-1", "-64", "abc", "64k", "", "1e3"})
    EXPECT(rejected(read_with("LDDL_TOKENIZE_MEMO_SAMPLE", bad), kSampleMsg));
  // ---- several at once; the first bad one in the order path, slow, grid, sample is reported ----
  {
    const Knobs r = read_with("LDDL_TOKENIZE_MEMO_SAMPLE", "64", "LDDL_TOKENIZE_GRID", "1");
    EXPECT(r.rc == 0 && defaults_but(r.k, kTokFused, 0, 1, 64));
  }
  EXPECT(rejected(read_with("LDDL_TOKENIZE_MEMO_SAMPLE", "x", "LDDL_TOKENIZE_GRID", "y"), kGridMsg));
  EXPECT(rejected(read_with("LDDL_TOKENIZE_GRID", "y", "LDDL_TOKENIZE_PATH", "cp"), path_msg("cp")));
  EXPECT(rejected(read_with("LDDL_TOKENIZE_PATH", "lane", "LDDL_TOKENIZE_GRID", "0"), kGridMsg));

  // ---- memo_sample: the default is on from 2^16 sentences, for vocabs whose ids fit 16 bits ----
  EXPECT(kMemoDiv == 32 && kMemoMinSample == (1 << 14));
  EXPECT(sample_of(65535, 30522) == 0);
  EXPECT(sample_of(65536, 30522) == 16384);  // max(65536 / 32, 2^14)
  EXPECT(sample_of((1 << 14) * 32, 30522) == 16384);
  EXPECT(sample_of((1 << 14) * 32 + 32, 30522) == 16385);
  EXPECT(sample_of(1 << 21, 30522) == 65536);  // 2^21 / 32
  EXPECT(sample_of(1 << 21, 65536) == 65536);
  EXPECT(sample_of(1 << 21, 65537) == 0);
  EXPECT(sample_of(65536, 65537) == 0);
  EXPECT(sample_of(1, 30522) == 0);
  // a set sample replaces the size and gates the memo on 0 < sample < n_sent
  for (int64_t n : {int64_t(100), int64_t(65535), int64_t(65536), int64_t(1) << 21}) {
    EXPECT(sample_of(n, 30522, 0) == 0);
    EXPECT(sample_of(n, 30522, 1) == 1);
    EXPECT(sample_of(n, 30522, n - 1) == n - 1);
    EXPECT(sample_of(n, 30522, n) == 0);
    EXPECT(sample_of(n, 30522, n + 1) == 0);
    EXPECT(sample_of(n, 65536, 1) == 1);
    EXPECT(sample_of(n, 65537, 1) == 0);
    // LDDL_TOKENIZE_PATH=plain: never; the other streaming value changes nothing
    EXPECT(sample_of(n, 30522, 1, kTokPlain) == 0);
    EXPECT(sample_of(n, 30522, -1, kTokPlain) == 0);
    EXPECT(sample_of(n, 30522, -1, kTokFused) == sample_of(n, 30522));
  }
  printf("tok_knobs_check ok\n");
  return 0;
}
