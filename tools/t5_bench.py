"""Times T5 span corruption by the method of blocks_bench.py: device events around
each call behind a spin kernel, medians, the calls alternating with their yardstick.

t5           lddl_t5_corrupt at the defaults (density 0.15, mean span length 3, 100 sentinels) at
             --batch rows, for each of --in-lens the plan length whose in_len it is
             (t5_tokens_length), on FULL blocks of blocks_bench's documents.
t5_one_span  the same rows with a mean span length that gives k = 1: the select and start passes
             are skipped, so this is the table and the emit alone, and t5 minus it is the four
             passes over the keys.
blocks_span  the yardstick: lddl_collate_blocks_masked in word mode (spans of up to 3 words) on
             the same blocks, rows as wide as the plan.

Writes profiles/t5_bench.json and prints it as one line. Needs a GPU.

    python tools/t5_bench.py [--batch 256] [--in-lens 128 512]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))
from blocks_bench import Bits, alternate, spin_ticks  # noqa: E402
from lddl_amd._native import lib  # noqa: E402
from lddl_amd.context import ASSETS, Context  # noqa: E402
from lddl_amd.torch import span as S  # noqa: E402
from lddl_amd.torch.roberta import collate_blocks, roberta_blocks  # noqa: E402
from lddl_amd.torch.t5 import t5_corrupt, t5_lengths, t5_tokens_length  # noqa: E402


def bench(a, backlog):
    from denoise_bench import token_table
    from span_bench import pair_table
    from wwm_bench import make_batch
    vocab = os.path.join(ASSETS, 'vocab_synth_uncased_30522.txt')
    ctx = Context(vocab)
    bits, span, sp = Bits(ctx), S.parse(3), ctx.special_ids
    ids = dict(bos_id=sp['[CLS]'], eos_id=sp['[SEP]'], pad_id=sp['[PAD]'], mask_id=sp['[MASK]'])
    res = {}
    for in_len in a.in_lens:
        L = t5_tokens_length(in_len) + 2
        tab = token_table(pair_table(ctx, make_batch(vocab, a.batch, L)[0]), a.sentence)
        plan, nb = roberta_blocks(tab, L, 'full')
        rows = torch.arange(a.batch, device='cuda') % nb
        calls = {
            't5': lambda c: t5_corrupt(bits, tab, plan, rows, noise=(99, c)),
            't5_one_span': lambda c: t5_corrupt(bits, tab, plan, rows, noise=(99, c),
                                                mean_noise_span_length=65536.0),
            'blocks_span': lambda c: collate_blocks(bits, tab, plan, rows, mask=(0.15, 99, c),
                                                    span=span, special_ids=ids)}
        out = alternate(calls, a.reps, a.inner, a.warmup, backlog)
        t5, one, ref = (out[k]['median'] for k in ('t5', 't5_one_span', 'blocks_span'))
        out.update(plan_seq_len=L, widths=t5_lengths(L - 2), blocks=nb,
                   mean_block_tokens=round(float(plan.block_len[:nb].float().mean()), 1),
                   ratio_over_blocks_span=round(t5 / ref, 2),
                   key_passes_us=round(t5 - one, 2), key_passes_share=round((t5 - one) / t5, 2))
        res['in_len{}'.format(in_len)] = out
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--in-lens', type=int, nargs='+', default=[128, 512])
    ap.add_argument('--sentence', type=int, default=24)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--backlog-ms', type=float, default=40.0)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 't5_bench.json'))
    a = ap.parse_args()
    res = {'build_id': lib.lddl_build_id().decode(), 'device': torch.cuda.get_device_name(0),
           'batch': a.batch, 'sentence': a.sentence, 'reps': a.reps, 'inner': a.inner,
           'us': bench(a, spin_ticks(a.backlog_ms))}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
