"""Time the loader's fused dynamic-masking collate, plain and whole-word, on the same packed
batch: `encode_packed(mask=..., events=...)`, i.e. HIP events around the one kernel
(lddl_collate_encode_masked / lddl_collate_encode_masked_ww), the two alternating call by call.

Sizes B=256 at L=128 and L=512. Per size and variant: `--reps` repetitions of `--inner` timed
calls after `--warmup` untimed ones; a repetition's figure is the median of its calls, and the
line gives the median, min and max of those figures (the spread within the run). On a tree
without whole-word masking (no `whole_word` argument of encode_packed) only plain is timed, so the
same script measures a parent commit. Prints one JSON line.

    python tools/wwm_bench.py [--batch 256] [--seqs 128 512] [--reps 10] [--inner 100]
"""
import argparse
import inspect
import json
import os
import random
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from lddl_amd._native import lib  # noqa: E402
from lddl_amd.context import Context  # noqa: E402
from lddl_amd.torch.bert import encode_packed  # noqa: E402
from lddl_amd.torch.packing import PackedBatch  # noqa: E402


def make_batch(vocab_file, B, L, seed=5):
    """B dynamic-masking samples of 3/4 L .. L tokens (the longest exactly L); the words are a
    vocab slice that holds '##' pieces (about a third), so words of several pieces occur."""
    with open(vocab_file, encoding='utf-8') as f:
        words = [w for w in (l.rstrip('\n') for l in f) if w and not w.startswith('[')][1000:6000]
    rng = random.Random(seed)
    batch = []
    for b in range(B):
        n = L - 3 if b == 0 else rng.randint(3 * L // 4, L) - 3
        na = rng.randint(1, n - 1)
        batch.append((' '.join(rng.choice(words) for _ in range(na)),
                      ' '.join(rng.choice(words) for _ in range(n - na)), rng.random() < 0.5))
    return batch, sum(w.startswith('##') for w in words) / len(words)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--seqs', type=int, nargs='+', default=[128, 512])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--inner', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=50)
    a = ap.parse_args()
    vocab = os.path.join(REPO, 'lddl_amd', 'assets', 'vocab_synth_uncased_30522.txt')
    ctx = Context(vocab)
    has_ww = 'whole_word' in inspect.signature(encode_packed).parameters
    variants = [('plain', {})] + ([('whole_word', {'whole_word': True})] if has_ww else [])
    res = {'build_id': lib.lddl_build_id().decode(), 'device': torch.cuda.get_device_name(0),
           'batch': a.batch, 'reps': a.reps, 'inner': a.inner, 'warmup': a.warmup, 'us': {}}
    for L in a.seqs:
        batch, frac = make_batch(vocab, a.batch, L)
        pk = PackedBatch(batch)
        res['continuation_fraction'] = round(frac, 3)

        def run(kw, counter, timed):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if timed else None
            enc = encode_packed(pk, ctx, 8, mask=(0.15, 99, counter), events=ev, **kw)
            assert enc['input_ids'].shape == (a.batch, L)
            return ev

        for i in range(a.warmup):
            for _, kw in variants:
                run(kw, i, False)
        torch.cuda.synchronize()
        per_rep = {name: [] for name, _ in variants}
        for r in range(a.reps):
            evs = {name: [] for name, _ in variants}
            for i in range(a.inner):
                for name, kw in variants:
                    evs[name].append(run(kw, (r << 20) + i, True))
            torch.cuda.synchronize()
            for name, _ in variants:
                per_rep[name].append(float(np.median([e0.elapsed_time(e1) * 1e3
                                                      for e0, e1 in evs[name]])))
        res['us']['L{}'.format(L)] = {
            name: {'median': round(float(np.median(v)), 2), 'min': round(min(v), 2),
                   'max': round(max(v), 2)} for name, v in per_rep.items()}
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
