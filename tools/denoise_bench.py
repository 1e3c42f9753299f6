"""Time lddl_bart_denoise against lddl_collate_pairs_masked_span, the nearest kernel
that reads a token table and decides spans, on the same samples: HIP events around the one
call, the two alternating call by call.

As in span_bench.py the calls take no timing events, so every repetition first queues a spin
kernel of `--backlog-ms` (torch.cuda._sleep): the host queues the repetition's calls behind it
and each pair of events spans device time only. A repetition's figure is the median of its
`--inner` calls; the line gives the median, min and max over `--reps` repetitions.

The samples are span_bench's pairs (wwm_bench.make_batch: about a third continuation pieces);
for the denoise call a pair is a document cut into sentences of `--sentence` pieces. Also
printed: the share of words deep in a row (ten words before them at least) that text infilling
deleted or replaced, next to mask_ratio (noised_share). One JSON line.

    python tools/denoise_bench.py [--batch 256] [--seqs 128 512] [--reps 10] [--inner 50]
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))
from lddl_amd._native import lib  # noqa: E402
from lddl_amd.context import Context  # noqa: E402
from lddl_amd.torch import span as S  # noqa: E402
from lddl_amd.torch.denoise import bart_denoise  # noqa: E402
from lddl_amd.torch.online import collate_pairs  # noqa: E402
from span_bench import pair_table  # noqa: E402
from wwm_bench import make_batch  # noqa: E402


def token_table(pb, sentence):
    """The pairs of a PairBatch as documents of `sentence`-piece sentences, in tokenize's layout."""
    off = pb.tok_off.cpu().numpy()
    n = np.diff(off)
    per = (n + sentence - 1) // sentence
    dso = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    k = np.arange(dso[-1]) - np.repeat(dso[:-1], per)  # the sentence's index in its document
    sent_off = np.repeat(off[:-1], per) + k * sentence
    sent_len = np.minimum(sentence, np.repeat(n, per) - k * sentence).astype(np.int32)
    ids = pb.tokens.to(torch.int32) & (0xFFFF if pb.tokens.element_size() == 2 else -1)
    dev = pb.tokens.device
    return (ids.contiguous(), torch.from_numpy(np.append(sent_off, off[-1])).to(dev),
            torch.from_numpy(sent_len).to(dev), torch.from_numpy(dso).to(dev))


def noised_share(ctx, a, P, deep=10, batches=8):
    """The share of words with at least `deep` words before them that text infilling deleted or
    replaced: rows of P pieces whose ids are distinct within the row, so a piece of `labels` is
    kept iff its id is in `input_ids`; a word's fate is its head's. No permutation, no random
    ids, and a width of 2 P + 2 that no insertion can overflow."""
    rng = np.random.default_rng(3)
    cont = np.array([t.startswith('##') and len(t) > 2 for t in ctx.tokens])
    pool = {False: np.flatnonzero(~cont)[1000:], True: np.flatnonzero(cont)}
    is_cont = rng.random((a.batch, P)) < 1 / 3
    is_cont[:, ::a.sentence] = False  # the first piece of a sentence is a head whatever its id
    ids = np.empty((a.batch, P), np.int32)
    for b in range(a.batch):
        for c in (False, True):
            ids[b, is_cont[b] == c] = rng.permutation(pool[c])[:int((is_cont[b] == c).sum())]
    dev = ctx.device
    rows = SimpleNamespace(tokens=torch.from_numpy(ids.reshape(-1)).to(dev),
                           tok_off=torch.arange(0, a.batch * P + 1, P, device=dev))
    tab = token_table(rows, a.sentence)
    head = torch.from_numpy(~is_cont).to(dev)
    deep_head = head & (torch.cumsum(head, 1) > deep)
    gone = total = 0
    for c in range(batches):
        o = bart_denoise(ctx, *tab, seq_len=2 * P + 2, mask=(a.mask_ratio, 7, c), random_ratio=0.0,
                         permute_sentence_ratio=0.0, check=False)
        assert int(o['src_lengths'].max()) <= 2 * P + 2
        kept = (o['labels'][:, 1:P + 1, None] == o['input_ids'][:, None, :]).any(2)
        gone += int((deep_head & ~kept).sum())
        total += int(deep_head.sum())
    return round(gone / total, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--seqs', type=int, nargs='+', default=[128, 512])
    ap.add_argument('--sentence', type=int, default=24)
    ap.add_argument('--mask-ratio', type=float, default=0.3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--backlog-ms', type=float, default=40.0)
    a = ap.parse_args()
    vocab = os.path.join(REPO, 'lddl_amd', 'assets', 'vocab_synth_uncased_30522.txt')
    ctx = Context(vocab)
    span = S.parse(3)
    cal = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda._sleep(1_000_000)
    cal[0].record()
    torch.cuda._sleep(20_000_000)
    cal[1].record()
    torch.cuda.synchronize()
    backlog = int(20_000_000 / cal[0].elapsed_time(cal[1]) * a.backlog_ms)
    res = {'build_id': lib.lddl_build_id().decode(), 'device': torch.cuda.get_device_name(0),
           'batch': a.batch, 'sentence': a.sentence, 'mask_ratio': a.mask_ratio, 'reps': a.reps,
           'inner': a.inner, 'us': {}, 'noised_share': {}}
    for L in a.seqs:
        pb = pair_table(ctx, make_batch(vocab, a.batch, L)[0])
        tab = token_table(pb, a.sentence)
        calls = {
            'denoise': lambda c: bart_denoise(ctx, *tab, seq_len=L, mask=(a.mask_ratio, 99, c),
                                              check=False),
            'pairs_span': lambda c: collate_pairs(ctx, pb, None, 8, -1, mask=(0.15, 99, c),
                                                  seq_len=L, check=False, span=span)}

        def timed(fn, c):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            fn(c)
            ev[1].record()
            return ev
        for i in range(a.warmup):
            for fn in calls.values():
                fn(i)
        torch.cuda.synchronize()
        per_rep = {k: [] for k in calls}
        for r in range(a.reps):
            evs = {k: [] for k in calls}
            torch.cuda._sleep(backlog)
            for i in range(a.inner):
                for k, fn in calls.items():
                    evs[k].append(timed(fn, (r << 20) + i))
            torch.cuda.synchronize()
            for k in calls:
                per_rep[k].append(float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in evs[k]])))
        out = {k: {'median': round(float(np.median(v)), 2), 'min': round(min(v), 2),
                   'max': round(max(v), 2)} for k, v in per_rep.items()}
        out['ratio'] = round(out['denoise']['median'] / out['pairs_span']['median'], 2)
        res['us']['L{}'.format(L)] = out
        res['noised_share']['L{}'.format(L)] = noised_share(ctx, a, L - 2)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
