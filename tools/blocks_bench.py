"""Times the RoBERTa blocks by the method of denoise_bench.py: device events around
each call behind a spin kernel, medians, the calls alternating with their yardsticks.

collate  lddl_collate_blocks_masked (word mode, spans of up to 3 words) at --batch rows and each
         of --seqs, against lddl_collate_pairs_masked_span and lddl_bart_denoise on samples of the
         same lengths (denoise_bench's pairs as documents of --sentence-piece sentences, FULL
         mode: about one block per document).
plan     lddl_blocks_plan on the sentences of --bytes of synthetic text (bpe_bench's corpus)
         against lddl_bpe_tokenize of the same text; per pass, the kernels' device times of one
         call under torch.profiler, summed by pass (null if the profiler gives none).

Writes profiles/blocks_bench.json and prints it as one line. Needs a GPU.

    python tools/blocks_bench.py [--bytes N] [--batch 256] [--seqs 128 512] [--skip-plan]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))
from lddl_amd._native import lib  # noqa: E402
from lddl_amd.context import ASSETS, Context  # noqa: E402
from lddl_amd.torch import span as S  # noqa: E402
from lddl_amd.torch.denoise import bart_denoise  # noqa: E402
from lddl_amd.torch.online import collate_pairs  # noqa: E402
from lddl_amd.torch.roberta import collate_blocks, roberta_blocks  # noqa: E402

PASSES = ('sep', 'scan', 'tile', 'chain', 'mark', 'write')


class Bits:
    """A WordPiece context's continuation ids as the bitmap collate_blocks takes."""

    def __init__(self, ctx):
        cont = np.array([t.startswith('##') and len(t) > 2 for t in ctx.tokens])
        bits = np.zeros((len(cont) + 31) // 32 * 32, bool)
        bits[:len(cont)] = cont
        self.t = torch.from_numpy(np.packbits(bits, bitorder='little').view(np.uint32)).cuda()
        self.cont_bits, self.special_ids, self.n = (self.t.data_ptr(), len(cont)), ctx.special_ids, len(cont)

    def __len__(self):
        return self.n


def spin_ticks(ms):
    cal = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda._sleep(1_000_000)
    cal[0].record()
    torch.cuda._sleep(20_000_000)
    cal[1].record()
    torch.cuda.synchronize()
    return int(20_000_000 / cal[0].elapsed_time(cal[1]) * ms)


def alternate(calls, reps, inner, warmup, backlog):
    """us per call: the median over reps of the median of `inner` calls behind the spin kernel."""
    for i in range(warmup):
        for fn in calls.values():
            fn(i)
    torch.cuda.synchronize()
    per_rep = {k: [] for k in calls}
    for r in range(reps):
        evs = {k: [] for k in calls}
        torch.cuda._sleep(backlog)
        for i in range(inner):
            for k, fn in calls.items():
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                fn((r << 20) + i)
                ev[1].record()
                evs[k].append(ev)
        torch.cuda.synchronize()
        for k in calls:
            per_rep[k].append(statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in evs[k]))
    return {k: {'median': round(statistics.median(v), 2), 'min': round(min(v), 2),
                'max': round(max(v), 2)} for k, v in per_rep.items()}


def collate_bench(a, backlog):
    from denoise_bench import token_table
    from span_bench import pair_table
    from wwm_bench import make_batch
    vocab = os.path.join(ASSETS, 'vocab_synth_uncased_30522.txt')
    ctx = Context(vocab)
    bits, span, sp = Bits(ctx), S.parse(3), ctx.special_ids
    ids = dict(bos_id=sp['[CLS]'], eos_id=sp['[SEP]'], pad_id=sp['[PAD]'], mask_id=sp['[MASK]'])
    res = {}
    for L in a.seqs:
        pb = pair_table(ctx, make_batch(vocab, a.batch, L)[0])
        tab = token_table(pb, a.sentence)
        plan, nb = roberta_blocks(tab, L, 'full')
        rows = torch.arange(a.batch, device='cuda') % nb
        calls = {
            'blocks_span': lambda c: collate_blocks(bits, tab, plan, rows, mask=(0.15, 99, c),
                                                    span=span, special_ids=ids),
            'pairs_span': lambda c: collate_pairs(ctx, pb, None, 8, -1, mask=(0.15, 99, c),
                                                  seq_len=L, check=False, span=span),
            'denoise': lambda c: bart_denoise(ctx, *tab, seq_len=L, mask=(0.3, 99, c), check=False)}
        out = alternate(calls, a.reps, a.inner, a.warmup, backlog)
        out['blocks'] = nb
        out['ratio_over_pairs_span'] = round(out['blocks_span']['median'] / out['pairs_span']['median'], 2)
        out['ratio_over_denoise'] = round(out['blocks_span']['median'] / out['denoise']['median'], 2)
        res['L{}'.format(L)] = out
    return res


def plan_bench(a):
    from lddl_amd import bpe, synth
    corp = synth.generate(seed=1234, n_bytes=a.bytes, nonascii_frac=0.05, threads=16)
    bp = bpe.BpeContext(bpe.SYNTH_VOCAB, bpe.SYNTH_MERGES)
    text, so, dso = (torch.from_numpy(x).cuda() for x in (corp.text, corp.sent_off, corp.doc_sent_off))
    ids, sent_len = bp.tokenize(text, so, dso)
    tab = (ids, so, sent_len, dso)
    calls = {'bpe_tokenize': lambda: bp.tokenize(text, so, dso),
             'plan_full': lambda: roberta_blocks(tab, 512, 'full'),
             'plan_doc': lambda: roberta_blocks(tab, 512, 'doc')}
    n_blocks = {k: f()[1] for k, f in list(calls.items())[1:]}  # the warm-up
    ms = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    passes = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            calls['plan_full']()
            torch.cuda.synchronize()
        passes = {p: 0.0 for p in PASSES}
        for e in prof.events():
            for p in PASSES:
                if ('blocks_' + p) in e.name or (p == 'scan' and 'scan_' in e.name):
                    passes[p] += getattr(e, 'device_time', 0) or getattr(e, 'cuda_time', 0)
                    break
        passes = {p: round(v, 1) for p, v in passes.items()} if any(passes.values()) else None
    except Exception as e:  # the figures above stand without the split
        passes = None
        print('profiler: {}'.format(e), file=sys.stderr)
    return {'text_bytes': len(corp.text), 'sentences': corp.n_sent, 'documents': corp.n_doc,
            'tiles': -(-corp.n_sent // 2048), 'seq_len': 512, 'n_blocks': n_blocks,
            'ms': {k: {'median': round(statistics.median(v), 3), 'min': round(min(v), 3),
                       'max': round(max(v), 3)} for k, v in ms.items()},
            'plan_over_tokenize': round(statistics.median(ms['plan_full']) /
                                        statistics.median(ms['bpe_tokenize']), 4),
            'plan_full_passes_us': passes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bytes', type=int, default=1 << 30)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--seqs', type=int, nargs='+', default=[128, 512])
    ap.add_argument('--sentence', type=int, default=24)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--backlog-ms', type=float, default=40.0)
    ap.add_argument('--skip-plan', action='store_true')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'blocks_bench.json'))
    a = ap.parse_args()
    res = {'build_id': lib.lddl_build_id().decode(), 'device': torch.cuda.get_device_name(0),
           'batch': a.batch, 'sentence': a.sentence, 'reps': a.reps, 'inner': a.inner,
           'collate_us': collate_bench(a, spin_ticks(a.backlog_ms))}
    print(json.dumps(res), flush=True)
    if not a.skip_plan:
        res['plan'] = plan_bench(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
