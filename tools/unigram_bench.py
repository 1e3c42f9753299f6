"""Times lddl_unigram_tokenize on synthetic text with the synthetic unigram model,
alternating with lddl_tokenize (WordPiece) and lddl_bpe_tokenize (byte-level BPE), the two
yardsticks, on the same text: device events around each call, the median of `--reps` after one
warm-up of each. Writes ms per GiB of the three, the two ratios, the pieces, the shares of words
that take the tile pass's second window (they cross their tile's end) and the long pass (over 64
bytes) from lddl_unigram_word_stats, the size of the trie tables and the build id to
profiles/unigram_bench.json. Needs a GPU.

    python tools/unigram_bench.py [--bytes N] [--reps 10] [--model FILE] [--out profiles/unigram_bench.json]
    python tools/unigram_bench.py --normalize [--bytes N] [--reps 10]    

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


def fullwidth(text, share, seed=99):
    """`text` (ASCII-mostly uint8) with about `share` of its words' ASCII letters made full-width
    (U+FF21.., three bytes each): the normaliser's dirty path."""
    import numpy as np
    word = np.cumsum(text == 0x20)
    hit = np.random.default_rng(seed).random(int(word[-1]) + 1) < share
    m = (((text >= 0x41) & (text <= 0x5A)) | ((text >= 0x61) & (text <= 0x7A))) & hit[word]
    lens = np.where(m, 3, 1)
    off = np.cumsum(lens) - lens
    out = np.empty(int(lens.sum()), np.uint8)
    out[off[~m]] = text[~m]
    cp = 0xFF00 + text[m].astype(np.int64) - 0x20
    out[off[m]], out[off[m] + 1], out[off[m] + 2] = 0xEF, 0x80 | ((cp >> 6) & 0x3F), 0x80 | (cp & 0x3F)
    return out


def normalize_bench(a):
    """The plan and the write of the normaliser, alternating with lddl_unigram_tokenize on the
    same text: device events, one warm-up, the median of --reps; once on the synthetic text and
    once with 20 % of its words full-width."""
    import ctypes
    import numpy as np
    import torch
    from lddl_amd import synth, unigram
    from lddl_amd._native import check, lib
    from lddl_amd.context import _ptr, _stream
    model = os.path.join(ROOT, 'tests', 'golden', 'unigram_nfkc.model')
    ug = unigram.UnigramContext(model)
    corp = synth.generate(seed=1234, n_bytes=a.bytes, nonascii_frac=0.05, threads=16)
    step = 1 << 28  # the same text, 256 MiB at a time: the index arrays are eight times the text
    wide = np.concatenate([fullwidth(corp.text[i:i + step], 0.2, seed=99 + i) for i in range(0, len(corp.text), step)])
    res = {'build_id': lib.lddl_build_id().decode(), 'device': torch.cuda.get_device_name(0),
           'reps': a.reps, 'model': ug.info(), 'runs': {}}
    for name, raw in (('synthetic', corp.text), ('fullwidth_20', wide)):
        text = torch.from_numpy(raw.copy()).cuda()
        so = torch.tensor([0, len(raw)], device='cuda')  # one sentence: the pass's cost is per tile
        so2 = torch.empty(2, dtype=torch.int64, device='cuda')
        head = (ug.handle, _stream(), _ptr(text), text.numel(), _ptr(so), 1, _ptr(so2))
        check(lib.lddl_unigram_normalize_plan(*head))
        size = int(so2[-1])
        out = torch.empty(size, dtype=torch.uint8, device='cuda')
        calls = {'plan': lambda: check(lib.lddl_unigram_normalize_plan(*head)),
                 'write': lambda: check(lib.lddl_unigram_normalize_write(*head, _ptr(out), size)),
                 'tokenize': lambda: ug.tokenize(out, so2)}
        ms = {k: [] for k in calls}
        for rep in range(a.reps + 1):  # the first is the warm-up
            for k, f in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                if rep:
                    ms[k].append(e0.elapsed_time(e1))
        gib = len(raw) / 2 ** 30
        stats = torch.empty(2, dtype=torch.int64, device='cuda')  # of the last plan, from its tiles
        check(lib.lddl_unigram_normalize_plan(*head))
        check(lib.lddl_unigram_normalize_stats(ug.handle, _stream(), _ptr(stats)))
        dirty = stats[1].item() / max(stats[0].item(), 1)
        res['runs'][name] = {'text_bytes': len(raw), 'normalised_bytes': size, 'dirty_tile_share': float(dirty),
                             'ms_per_gib': {k: statistics.median(v) / gib for k, v in ms.items()},
                             'ms_per_gib_min_max': {k: [min(v) / gib, max(v) / gib] for k, v in ms.items()}}
    out_path = os.path.join(ROOT, 'profiles', 'unigram_norm_bench.json')
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bytes', type=int, default=1 << 30)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'unigram_bench.json'))
    ap.add_argument('--model', default=os.path.join(ROOT, 'tests', 'golden', 'unigram_synth.model'))
    ap.add_argument('--normalize', action='store_true',
                    help='time lddl_unigram_normalize_plan / _write (DESIGN §33) instead, with the '
                         'golden nmt_nfkc model, into profiles/unigram_norm_bench.json')
    a = ap.parse_args()
    if a.normalize:
        return normalize_bench(a)
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
