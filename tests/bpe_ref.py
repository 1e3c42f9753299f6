"""The plain reference of the byte-level BPE tokenizer, stdlib only: GPT-2's
pre-tokenizer as a sequential matcher that tries the pattern's alternatives in order at each
position, the classic bpe() loop, and the assignment of a pre-token to the sentence of its last
byte. Classes come from unicodedata and the White_Space list."""
import unicodedata

WHITE_SPACE = frozenset([*range(0x09, 0x0E), 0x20, 0x85, 0xA0, 0x1680, *range(0x2000, 0x200B),
                         0x2028, 0x2029, 0x202F, 0x205F, 0x3000])
CONTRACTIONS = ("'s", "'t", "'re", "'ve", "'m", "'ll", "'d")
MAX_WORD = 1024  # LDDL_BPE_MAX_WORD


def char_class(c):
    if ord(c) in WHITE_SPACE:
        return 'S'
    cat = unicodedata.category(c)[0]
    return cat if cat in 'LN' else 'O'


def pretokens(s):
    """'s|'t|'re|'ve|'m|'ll|'d| ?\\p{L}+| ?\\p{N}+| ?[^\\s\\p{L}\\p{N}]+|\\s+(?!\\S)|\\s+ over str s."""
    out, i, n = [], 0, len(s)

    def run(j):
        k = char_class(s[j])
        while j < n and char_class(s[j]) == k:
            j += 1
        return j
    while i < n:
        e = next((i + len(c) for c in CONTRACTIONS if s.startswith(c, i)), None)
        if e is None:
            j = i + 1 if s[i] == ' ' else i  # ' ?' and a run of letters, numbers or others
            if j < n and char_class(s[j]) != 'S':
                e = run(j)
            else:
                e = run(i)                   # \s+(?!\S): give back one if a non-space follows
                if e < n and e - 1 > i:
                    e -= 1                   # (with nothing to give back, \s+ takes the one)
        out.append(s[i:e])
        i = e
    return out


class Tables:
    """byte_id[256] and {(left, right): (rank, merged)} from the tokens (bytes by id) and the
    merge triples in rank order."""

    def __init__(self, tokens, merges):
        self.byte_id = [None] * 256
        for i, t in enumerate(tokens):
            if len(t) == 1 and self.byte_id[t[0]] is None:
                self.byte_id[t[0]] = i
        self.ranks = {}
        for r, (a, b, m) in enumerate(merges):
            self.ranks.setdefault((int(a), int(b)), (r, int(m)))
        self.memo = {}

    def bpe(self, word):
        """The ids of one pre-token (bytes), in slices of MAX_WORD bytes."""
        if word not in self.memo:
            out = []
            for k in range(0, len(word), MAX_WORD):
                sym = [self.byte_id[b] for b in word[k:k + MAX_WORD]]
                while True:
                    pairs = [p for p in zip(sym, sym[1:]) if p in self.ranks]
                    if not pairs:
                        break
                    a, b = min(pairs, key=lambda p: self.ranks[p][0])
                    new, i = [], 0
                    while i < len(sym):
                        if i + 1 < len(sym) and sym[i] == a and sym[i + 1] == b:
                            new.append(self.ranks[a, b][1])
                            i += 2
                        else:
                            new.append(sym[i])
                            i += 1
                    sym = new
                out += sym
            self.memo[word] = out
        return self.memo[word]

    def encode(self, text):
        """GPT-2's encode of one document (bytes of valid UTF-8) -> ids."""
        return [i for w in pretokens(text.decode('utf-8')) for i in self.bpe(w.encode('utf-8'))]

    def encode_sentences(self, sentences, max_pieces=512):
        """One document as its sentences (bytes): the kept ids per sentence. A pre-token goes to
        the sentence of its last byte; a sentence keeps min(pieces, max_pieces, its bytes)."""
        ends, out, pos, s = [], [[] for _ in sentences], 0, 0
        for x in sentences:
            ends.append((ends[-1] if ends else 0) + len(x))
        for w in pretokens(b''.join(sentences).decode('utf-8')):
            w = w.encode('utf-8')
            pos += len(w)
            while ends[s] < pos:  # the sentence that holds byte pos - 1
                s += 1
            out[s] += self.bpe(w)
        return [o[:min(max_pieces, len(x))] for o, x in zip(out, sentences)]
