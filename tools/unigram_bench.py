"""Times lddl_unigram_tokenize on synthetic text with the synthetic unigram model,
alternating with lddl_tokenize (WordPiece) and lddl_bpe_tokenize (byte-level BPE), the two
yardsticks, on the same text: device events around each call, the median of `--reps` after one
warm-up of each. Writes ms per GiB of the three, the two ratios, the pieces, the shares of words
that take the tile pass's second window (they cross their tile's end) and the long pass (over 64
bytes) from lddl_unigram_word_stats, the size of the trie tables and the build id to
profiles/unigram_bench.json. Needs a GPU.

    python tools/unigram_bench.py [--bytes N] [--reps 10] [--model FILE] [--out profiles/unigram_bench.json]

The synthetic model has about 2,000 pieces: its trie is far smaller than that of a 32,000-piece
checkpoint, whose cache behaviour this tool does not show.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bytes', type=int, default=1 << 30)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'unigram_bench.json'))
    ap.add_argument('--model', default=os.path.join(ROOT, 'tests', 'golden', 'unigram_synth.model'))
    a = ap.parse_args()
    import torch
    from lddl_amd import bpe, synth, unigram
    from lddl_amd._native import lib
    from lddl_amd.context import ASSETS, LEN_MASK, Context
    corp = synth.generate(seed=1234, n_bytes=a.bytes, nonascii_frac=0.05, threads=16)
    wp = Context(os.path.join(ASSETS, 'vocab_synth_uncased_30522.txt'))
    bp = bpe.BpeContext(bpe.SYNTH_VOCAB, bpe.SYNTH_MERGES)
    ug = unigram.UnigramContext(a.model)
    text, so, dso = (torch.from_numpy(x).cuda() for x in (corp.text, corp.sent_off, corp.doc_sent_off))
    calls = {'wordpiece': lambda: wp.tokenize(text, so), 'bpe': lambda: bp.tokenize(text, so, dso),
             'unigram': lambda: ug.tokenize(text, so, dso)}
    pieces = {k: int((f()[1] & LEN_MASK).sum()) for k, f in calls.items()}  # the warm-up
    ms = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    n_words, n_cross, n_long = ug.word_stats(text, so, dso).tolist()
    gib = len(corp.text) / 2 ** 30
    med = {k: statistics.median(v) / gib for k, v in ms.items()}
    res = {'build_id': lib.lddl_build_id().decode(), 'device': torch.cuda.get_device_name(0),
           'text_bytes': len(corp.text), 'sentences': corp.n_sent, 'documents': corp.n_doc,
           'unigram_model': ug.info(), 'reps': a.reps, 'pieces': pieces, 'ms_per_gib': med,
           'ms_per_gib_min_max': {k: [min(v) / gib, max(v) / gib] for k, v in ms.items()},
           'ratio_unigram_over_wordpiece': med['unigram'] / med['wordpiece'],
           'ratio_unigram_over_bpe': med['unigram'] / med['bpe'],
           'word_stats': {'words': n_words, 'second_window_share': n_cross / max(n_words, 1),
                          'long_share': n_long / max(n_words, 1)}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
