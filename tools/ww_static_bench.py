"""Time the native-RNG pair planner with static masking, per-token and whole-word
(`make_pairs(..., rng='native', masking=True, whole_word=...)`), on one synthetic corpus that
stays resident on the GPU, the two alternating call by call.

The figure is `PairBatch.plan_ms`: HIP events from the planner's first launch to the end of its
last kernel, which on the native path spans the walk (count and emit pass), the mask stage and
the order kernel; the two variants differ in the mask stage only. Per sequence length and
variant: `--reps` timed calls after `--warmup` untimed ones; the line gives the median, min and
max over the calls (the spread within the run) and the pairs and masked positions of a call. On a
tree without whole-word static masking (no `whole_word` keyword of make_pairs) only the
per-token path is timed, so the same script measures a parent commit. Prints one JSON line and,
with `--out`, writes it to that file.

    python tools/ww_static_bench.py [--mib 256] [--part-kib 1024] [--seqs 128 512] [--reps 15]
"""
import argparse
import inspect
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from lddl_amd import synth  # noqa: E402
from lddl_amd._native import lib  # noqa: E402
from lddl_amd.context import Context  # noqa: E402
from lddl_amd.pairs import make_pairs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mib', type=int, default=256, help='corpus size')
    ap.add_argument('--part-kib', type=int, default=1024, help='partition size')
    ap.add_argument('--seqs', type=int, nargs='+', default=[128, 512])
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--per-token-only', action='store_true',
                    help='time the per-token path alone, as on a parent tree (separates the '
                         'build from the alternation with whole-word calls)')
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    vocab = os.path.join(REPO, 'lddl_amd', 'assets', 'vocab_synth_uncased_30522.txt')
    torch.cuda.set_device(0)
    ctx = Context(vocab)
    corp = synth.generate(seed=2025, n_bytes=a.mib << 20, nonascii_frac=0.01, threads=16)
    doc_bytes = corp.sent_off[corp.doc_sent_off]
    cuts = np.searchsorted(doc_bytes, np.arange(0, doc_bytes[-1], a.part_kib << 10), 'left')
    part = np.unique(np.concatenate([[0], cuts, [corp.n_doc]])).astype(np.int64)
    dev = ctx.device
    sent_off = torch.from_numpy(corp.sent_off).to(dev)
    ids, sent_len = ctx.tokenize(torch.from_numpy(corp.text).to(dev), sent_off)
    doc_off = torch.from_numpy(corp.doc_sent_off).to(dev)
    d_part = torch.from_numpy(part).to(dev)
    d_seed = torch.arange(len(part) - 1, dtype=torch.int64, device=dev) * 7919 + 12345
    has_ww = 'whole_word' in inspect.signature(make_pairs).parameters and not a.per_token_only
    variants = [('per_token', {})] + ([('whole_word', {'whole_word': True})] if has_ww else [])
    res = {'build_id': lib.lddl_build_id().decode(), 'device': torch.cuda.get_device_name(0),
           'corpus_mib': a.mib, 'partitions': len(part) - 1, 'dup': 5, 'reps': a.reps,
           'warmup': a.warmup, 'plan_ms': {}}

    for seq in a.seqs:
        def call(kw):
            pb = make_pairs(ctx, sent_off, ids, sent_len, doc_off, d_part, d_seed, seq=seq, dup=5,
                            masking=True, rng='native', native_seed=99, **kw)
            torch.cuda.synchronize()
            return pb.plan_ms, pb.n_pairs, pb.n_masked

        for _ in range(a.warmup):
            for _, kw in variants:
                call(kw)
        ms = {name: [] for name, _ in variants}
        shape = {}
        for _ in range(a.reps):
            for name, kw in variants:
                t, n_pairs, n_masked = call(kw)
                ms[name].append(t)
                shape[name] = (n_pairs, n_masked)
        res['plan_ms']['seq{}'.format(seq)] = {
            name: {'median': round(float(np.median(v)), 3), 'min': round(min(v), 3),
                   'max': round(max(v), 3), 'pairs': shape[name][0], 'masked': shape[name][1]}
            for name, v in ms.items()}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
