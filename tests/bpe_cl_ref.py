"""The plain reference of the cl100k-style pre-tokenizer, stdlib only: a sequential
matcher that tries the alternatives of
  (?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\\r\\n\\p{L}\\p{N}]?\\p{L}+|\\p{N}{1,3}| ?[^\\s\\p{L}\\p{N}]+[\\r\\n]*|\\s*[\\r\\n]+|\\s+(?!\\S)|\\s+
in order at each position (digit_group = 1 gives Qwen2's \\p{N}), and `ignore_merges` as a lookup
of the whole pre-token in front of bpe_ref's merge loop."""
from bpe_ref import MAX_WORD, Tables, char_class

CONTRACTIONS = ("'s", "'t", "'re", "'ve", "'m", "'ll", "'d")


def _fold(c):
    return 's' if c == 'ſ' else c.lower()  # (?i): ASCII case and the long s


def pretokens(s, digit_group=3):
    out, i, n = [], 0, len(s)
    cls = [char_class(c) for c in s]
    nl = [c in '\r\n' for c in s]

    def run(j, pred):
        while j < n and pred(j):
            j += 1
        return j
    while i < n:
        e = next((i + len(c) for c in CONTRACTIONS if len(s) >= i + len(c) and s[i] == "'" and
                  all(_fold(x) == y for x, y in zip(s[i + 1:], c[1:]))), None)
        if e is None:  # [^\r\n\p{L}\p{N}]?\p{L}+
            j = i + 1 if cls[i] not in 'LN' and not nl[i] else i
            if j < n and cls[j] == 'L':
                e = run(j, lambda k: cls[k] == 'L')
        if e is None and cls[i] == 'N':  # \p{N}{1,3}
            e = run(i, lambda k: cls[k] == 'N' and k < i + digit_group)
        if e is None:  # ' ?[^\s\p{L}\p{N}]+[\r\n]*'
            j = i + 1 if s[i] == ' ' else i
            if j < n and cls[j] == 'O':
                e = run(run(j, lambda k: cls[k] == 'O'), lambda k: nl[k])
        if e is None:  # from here s[i] is white space
            j = run(i, lambda k: cls[k] == 'S')
            k = j
            while k > i and not nl[k - 1]:  # \s*[\r\n]+: back to the run's last newline
                k -= 1
            if k > i:
                e = k
            elif j < n and j - 1 > i:       # \s+(?!\S): give back one if a non-space follows
                e = j - 1
            else:                           # the run at the end, or \s+ with nothing to give back
                e = j
        out.append(s[i:e])
        i = e
    return out


class ClTables(Tables):
    """bpe_ref.Tables with the cl100k pre-tokenizer; ignore_merges: a pre-token of at most
    MAX_WORD bytes whose bytes are a token is that token (the lowest id of equal tokens)."""

    def __init__(self, tokens, merges, digit_group=3, ignore_merges=False):
        super().__init__(tokens, merges)
        self.digit_group, self.whole = digit_group, {}
        if ignore_merges:
            for i, t in enumerate(tokens):
                if 2 <= len(t) <= MAX_WORD:
                    self.whole.setdefault(bytes(t), i)

    def bpe(self, word):
        return [self.whole[word]] if word in self.whole else super().bpe(word)

    def pretokens(self, text):
        return pretokens(text, self.digit_group)

    def encode(self, text):
        return [i for w in self.pretokens(text.decode('utf-8')) for i in self.bpe(w.encode('utf-8'))]
