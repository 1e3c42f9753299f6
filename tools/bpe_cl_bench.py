"""Times lddl_bpe_tokenize with GPT-2's pattern and with cl100k's, each with and
without ignore_merges, alternating in one run on the same synthetic text with the synthetic BPE
vocabulary: device events around each call, one warm-up of each, the median of `--reps` with min
and max. Writes ms per GiB, the pieces and pre-tokens of each and the build id to
profiles/bpe_cl_bench.json. Needs a GPU.

    python tools/bpe_cl_bench.py [--bytes N] [--reps 10] [--out profiles/bpe_cl_bench.json]

The synthetic text has hardly any run of digits or white space that fills a 64-byte tile, so
the walk over whole-run tiles (bpe_cl_carry_kernel) is launched but not what is timed.
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bpe_cl_bench.json'))
    a = ap.parse_args()
    import torch
    from lddl_amd import bpe, synth
    from lddl_amd._native import lib
    corp = synth.generate(seed=1234, n_bytes=a.bytes, nonascii_frac=0.05, threads=16)
    text, so, dso = (torch.from_numpy(x).cuda() for x in (corp.text, corp.sent_off, corp.doc_sent_off))
    ctx = {'{}{}'.format(p, '+whole' if w else ''): bpe.BpeContext(
        bpe.SYNTH_VOCAB, bpe.SYNTH_MERGES, pattern=p, ignore_merges=w)
        for p in ('gpt2', 'cl100k') for w in (False, True)}
    pieces = {k: int(c.tokenize(text, so, dso)[1].sum()) for k, c in ctx.items()}  # the warm-up
    ms = {k: [] for k in ctx}
    for _ in range(a.reps):
        for k, c in ctx.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c.tokenize(text, so, dso)
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    gib = len(corp.text) / 2 ** 30
    res = {'build_id': lib.lddl_build_id().decode(), 'device': torch.cuda.get_device_name(0),
           'text_bytes': len(corp.text), 'documents': corp.n_doc, 'reps': a.reps, 'pieces': pieces,
           'pretokens': {k: c.pretoken_stats(text, so, dso).tolist() for k, c in ctx.items() if '+' not in k},
           'ms_per_gib': {k: statistics.median(v) / gib for k, v in ms.items()},
           'ms_per_gib_min_max': {k: [min(v) / gib, max(v) / gib] for k, v in ms.items()}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
