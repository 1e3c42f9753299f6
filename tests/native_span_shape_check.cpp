// CPU check of mask_span_native_kernel's launch shape (csrc/native_shape.h, native_span_shape):
// argv = target sequence lengths. Exits non-zero on the first failed expectation.
#include <cstdio>
#include <cstdlib>

#include "native_shape.h"

#define EXPECT(c)                                                              \
  do {                                                                         \
    if (!(c)) {                                                                \
      fprintf(stderr, "%s:%d: seq %d failed: %s\n", __FILE__, __LINE__, seq, #c); \
      exit(1);                                                                 \
    }                                                                          \
  } while (0)

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    const int seq = atoi(argv[i]);
    const lddl::SpanShape s = lddl::native_span_shape(seq);
    EXPECT(s.seqp % 64 == 0 && s.seqp >= seq - 3 && s.seqp < seq - 3 + 64);
    // per wave: an 8-byte entry per token, a 4-byte table row per word and one past the last;
    // a multiple of 8, so every wave's entries are aligned
    EXPECT(s.wave_bytes >= (size_t)8 * s.seqp + (size_t)4 * (s.seqp + 1) && s.wave_bytes % 8 == 0);
    EXPECT(s.waves >= 1 && s.waves <= 4);
    EXPECT(s.lds_bytes() == s.wave_bytes * (size_t)s.waves && s.lds_bytes() <= lddl::kNativeMaskLds);
    EXPECT(s.waves == 4 || s.wave_bytes * (size_t)(s.waves + 1) > lddl::kNativeMaskLds);
    EXPECT(s.threads() == 64u * (unsigned)s.waves);
    for (long long n : {1LL, 255LL, 257LL, 1LL << 31})
      EXPECT((long long)s.grid(n) * s.waves >= n && ((long long)s.grid(n) - 1) * s.waves < n);
  }
  printf("native_span_shape_check ok\n");
  return 0;
}
