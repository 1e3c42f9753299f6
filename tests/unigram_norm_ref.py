"""The sequential rules of lddl_unigram_normalize_plan / _write and of byte fallback
(include/lddl_amd.h) in plain Python: helper code of test_unigram_norm_host.py and
test_unigram_norm_gpu.py, not a test."""
import os

import unigram_ref

NFKC_MODEL = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'unigram_nfkc.model')
F = unigram_ref.F


def normalize(rules, s):
    """One sentence (bytes) under `rules`, a dict of bytes -> bytes."""
    longest = max(map(len, rules))
    out, i = bytearray(), 0
    while i < len(s):
        for n in range(min(longest, len(s) - i), 0, -1):
            if s[i:i + n] in rules:
                out += rules[s[i:i + n]]
                break
        else:
            c = s[i]
            n = 1 if c < 0x80 else 2 if 0xC2 <= c <= 0xDF else 3 if 0xE0 <= c <= 0xEF else 4
            try:
                s[i:i + n].decode('utf-8')  # strict: whole, no overlong form, no surrogate
                out += s[i:i + n]
            except UnicodeDecodeError:
                out, n = out + b'\xef\xbf\xbd', 1
        i += n
    return bytes(out)


class ByteTables(unigram_ref.Tables):
    """unigram_ref.Tables with byte fallback: the same Viterbi; on the path every unknown
    piece becomes byte_pieces[b] for each of its bytes."""

    def __init__(self, *a, byte_pieces=None, **kw):
        super().__init__(*a, **kw)
        self.byte_pieces = byte_pieces

    def viterbi(self, b, first):
        if self.byte_pieces is None:
            return super().viterbi(b, first)
        off = 3 if first else 0
        clen = {0: 3} if first else {}
        clen.update({off + p: unigram_ref.char_len(b[off:], p) for p in range(len(b) - off)})
        best, back = {0: F(0.0)}, {}
        for s in (p for p in sorted(clen) if clen[p]):
            ends = {e: self.ids[b[s:e]] for e in range(s + 1, min(len(b), s + self.longest) + 1)
                    if b[s:e] in self.ids}
            if s + clen[s] not in ends:
                ends[s + clen[s]] = self.unk_id
            for e in sorted(ends):  # the unknown character after the pieces of its length: never both
                cand = F(best[s] + (self.unk_score if ends[e] == self.unk_id else self.scores[ends[e]]))
                if e not in best or cand > best[e]:
                    best[e], back[e] = cand, (s, ends[e])
        out, e = [], len(b)
        while e:
            s, i = back[e]
            out[0:0] = [int(self.byte_pieces[x]) for x in b[s:e]] if i == self.unk_id else [i]
            e = s
        return out
