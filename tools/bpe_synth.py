"""Trains the synthetic byte-level BPE vocabulary (lddl_amd/assets/bpe_synth_vocab.json and
bpe_synth_merges.txt) by plain-Python BPE over lddl_amd.synth's corpus, the source
the vocab_synth_* files were made from. Fixed seed; ties go to the pair seen first. Ids as BART
lays them out: <s> <pad> </s> <unk>, the 256 byte tokens, the merges in rank order, <mask>.

    python tools/bpe_synth.py [n_merges] [corpus_bytes]
"""
import collections
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# close enough to GPT-2's pattern for training: the merges only have to be a valid list
WORDS = re.compile(r" ?[^\W\d_]+| ?\d+| ?[^\s\w]+|\s+")


def train(text, n_merges):
    from lddl_amd.bpe import bytes_to_unicode
    b2u = bytes_to_unicode()
    words = collections.Counter(WORDS.findall(text))
    words = [([b2u[b] for b in w.encode('utf-8')], n) for w, n in words.items()]
    merges = []
    while len(merges) < n_merges:
        pairs = collections.Counter()
        for sym, n in words:
            for p in zip(sym, sym[1:]):
                pairs[p] += n
        if not pairs:
            break
        best = max(pairs.items(), key=lambda kv: kv[1])  # the first of equal counts
        if best[1] < 2:
            break
        a, b = best[0]
        merges.append((a, b))
        for sym, _ in words:
            i = 0
            while i + 1 < len(sym):
                if sym[i] == a and sym[i + 1] == b:
                    sym[i:i + 2] = [a + b]
                i += 1
    tokens = ['<s>', '<pad>', '</s>', '<unk>'] + [b2u[b] for b in range(256)]
    for a, b in merges:
        if a + b not in tokens:
            tokens.append(a + b)
    tokens.append('<mask>')
    return {t: i for i, t in enumerate(tokens)}, merges


if __name__ == '__main__':
    from lddl_amd import synth
    n_merges = int(sys.argv[1]) if len(sys.argv) > 1 else 1500
    n_bytes = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 18
    corp = synth.generate(seed=2024, n_bytes=n_bytes, nonascii_frac=0.05, threads=1)
    text = ' '.join(' '.join(d) for d in corp.documents())
    vocab, merges = train(text, n_merges)
    assets = os.path.join(ROOT, 'lddl_amd', 'assets')
    with open(os.path.join(assets, 'bpe_synth_vocab.json'), 'w', encoding='utf-8') as f:
        json.dump(vocab, f, ensure_ascii=False, separators=(',', ':'))
    with open(os.path.join(assets, 'bpe_synth_merges.txt'), 'w', encoding='utf-8') as f:
        f.write('#version: 0.2\n' + ''.join('{} {}\n'.format(a, b) for a, b in merges))
    print('{} tokens, {} merges'.format(len(vocab), len(merges)))
