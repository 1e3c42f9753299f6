"""The sequential rules of lddl_unigram_tokenize (include/lddl_amd.h) in plain Python with
numpy.float32: helper code of test_unigram_host.py and test_unigram_gpu.py, not a test."""
import os

import numpy as np

# the synthetic model of tools/unigram_synth.py (2,000 pieces, the `identity` normaliser)
SYNTH_MODEL = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'unigram_synth.model')
MARK = b'\xe2\x96\x81'
MAX_WORD = 1024
F = np.float32


def char_len(b, p):
    """0 if byte p of the word b is a continuation byte that a whole sequence claims, else the
    length of the character that starts there."""
    def whole(q):
        c = b[q]
        n = 2 if 0xC2 <= c <= 0xDF else 3 if 0xE0 <= c <= 0xEF else 4 if 0xF0 <= c <= 0xF4 else 1
        return n if q + n <= len(b) and all(x & 0xC0 == 0x80 for x in b[q + 1:q + n]) else 1
    if b[p] & 0xC0 != 0x80:
        return whole(p)
    for k in range(1, min(3, p) + 1):
        if b[p - k] >= 0xC0:
            return 0 if whole(p - k) > k else 1
        if b[p - k] < 0x80:
            break
    return 1


class Tables:
    def __init__(self, pieces, scores, types=None, unk_id=0, ascii_ws=False):
        pieces = [p.encode('utf-8') if isinstance(p, str) else p for p in pieces]
        types = [2 if i == unk_id else 1 for i in range(len(pieces))] if types is None else types
        self.ids = {p: i for i, p in enumerate(pieces) if types[i] in (1, 4)}
        self.scores = np.asarray(scores, F)
        self.unk_id = unk_id
        self.unk_score = F(min(self.scores[i] for i in range(len(pieces)) if types[i] == 1)) - F(10.0)
        self.longest = max(len(p) for p in self.ids)
        self.spaces = b' \t\n\x0c\r' if ascii_ws else b' '

    def viterbi(self, b, first):
        """The pieces of one slice b; `first`: it opens with the mark (character starts 0, 3)."""
        off = 3 if first else 0
        clen = {0: 3} if first else {}
        clen.update({off + p: char_len(b[off:], p) for p in range(len(b) - off)})
        best, back = {0: F(0.0)}, {}
        for s in (p for p in sorted(clen) if clen[p]):
            one = False
            for e in range(s + 1, min(len(b), s + self.longest) + 1):
                i = self.ids.get(b[s:e])
                if i is not None:
                    one |= e - s == clen[s]
                    cand = F(best[s] + self.scores[i])
                    if e not in best or cand > best[e]:
                        best[e], back[e] = cand, (s, i)
            if not one:
                e, cand = s + clen[s], F(best[s] + self.unk_score)
                if e not in best or cand > best[e]:
                    best[e], back[e] = cand, (s, self.unk_id)
        out, e = [], len(b)
        while e:
            e, i = back[e]
            if not (out and out[0] == self.unk_id == i):
                out.insert(0, i)
        return out

    def encode_word(self, w):
        out, a = [], 0
        while a < len(w):
            n = min(MAX_WORD, len(w) - a)
            while a + n < len(w) and char_len(w, a + n) == 0:
                n -= 1
            out += self.viterbi((MARK if a == 0 else b'') + w[a:a + n], a == 0)
            a += n
        return out

    def encode(self, sentence):
        words = bytes(0x20 if c in self.spaces else c for c in sentence).split(b' ')
        return [i for w in words if w for i in self.encode_word(w)]

    def encode_sentences(self, sentences, max_pieces=512):
        return [self.encode(s)[:min(max_pieces, len(s))] for s in sentences]
