"""Times the GPT stream on synthetic text tokenized with the synthetic byte-level
BPE vocabulary: lddl_stream_plan over the whole corpus, and lddl_stream_rows and
lddl_stream_cu_seqlens for one batch of seeded random rows at 8 x 8192 and 64 x 2048, with and
without fill-in-the-middle, under a seeded document permutation. The yardstick is the bytes
lddl_stream_rows stores per second (32 a slot) next to what lddl_collate_blocks (24 a slot,
unmasked) reaches on the same corpus at the same batch shapes, the two alternating in one run.
A time is that of a call: device events around `--inner` back-to-back calls on preallocated
outputs, divided by their number (launch gaps included), the median of `--reps` after one
warm-up of every shape. Writes profiles/gpt_bench.json with the build id. Needs a GPU.

    python tools/gpt_bench.py [--bytes N] [--reps 10] [--inner 200] [--out profiles/gpt_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((8, 8192), (64, 2048))


def timed(f, inner):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bytes', type=int, default=64 << 20)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--inner', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gpt_bench.json'))
    a = ap.parse_args()
    import numpy as np
    import torch
    from lddl_amd import bpe, synth
    from lddl_amd._native import check, lib
    from lddl_amd.context import LEN_MASK, _ptr, _stream
    from lddl_amd.torch import roberta_blocks, stream_plan
    corp = synth.generate(seed=1234, n_bytes=a.bytes, nonascii_frac=0.05, threads=16)
    bp = bpe.BpeContext(bpe.SYNTH_VOCAB, bpe.SYNTH_MERGES)
    text, so, dso = (torch.from_numpy(x).cuda() for x in (corp.text, corp.sent_off, corp.doc_sent_off))
    ids, sent_len = bp.tokenize(text, so, dso)
    table = (ids, so, sent_len, dso)
    n_sent, n_doc = sent_len.numel(), dso.numel() - 1
    rng = np.random.default_rng(34)
    order = torch.from_numpy(rng.permutation(n_doc)).cuda()
    eos, sent = bp.special_ids['</s>'], [len(bp) + k for k in range(3)]
    new = lambda *s, dt=torch.long: torch.empty(*s, dtype=dt, device='cuda')  # noqa: E731
    calls, meta = {}, {}
    for B, L in SHAPES:
        shape = '{}x{}'.format(B, L)
        bplan, n_blocks = roberta_blocks(table, L, 'full')
        brows = torch.from_numpy(rng.permutation(n_blocks)[:B]).cuda()
        bout = [new(B, L) for _ in range(3)]
        calls['blocks_collate/' + shape] = lambda p=bplan, r=brows, o=bout, B=B, L=L: check(
            lib.lddl_collate_blocks(_stream(), _ptr(ids), _ptr(so), _ptr(p.piece_off),
                                    _ptr(p.sent_sep), _ptr(p.block_sent), _ptr(r), B, L,
                                    *[_ptr(v) for v in o], 0, eos, 1))
        meta['blocks_collate/' + shape] = B * L * 24
        for name, fim in (('plain', None), ('fim', (0.5, 0.5, 7, 0))):
            plan, n_rows = stream_plan(table, L, order, fim)
            rows = torch.from_numpy(rng.permutation(n_rows)[:B]).cuda()
            out = [new(B, L) for _ in range(4)]
            cap = min(B * L, B + n_doc)  # collate_stream's default for distinct rows
            cu, ns = new(cap + 1, dt=torch.int32), new(1, dt=torch.int32)
            key = '{}/{}'.format(name, shape)
            calls['plan/' + key] = lambda p=plan, L=L: check(lib.lddl_stream_plan(
                _stream(), _ptr(sent_len), n_sent, _ptr(dso), n_doc, _ptr(order), L, *p.fim,
                _ptr(p.sent_tok_off), _ptr(p.doc_off), _ptr(p.counts)))
            calls['rows/' + key] = lambda p=plan, r=rows, o=out, B=B, L=L: check(lib.lddl_stream_rows(
                _stream(), _ptr(ids), _ptr(so), n_sent, _ptr(dso), n_doc, _ptr(order),
                _ptr(p.sent_tok_off), _ptr(p.doc_off), _ptr(r), B, L, *p.fim, eos, *sent, 0, 1,
                -100, *[_ptr(v) for v in o]))
            calls['cu_seqlens/' + key] = lambda p=plan, r=rows, B=B, L=L, m=cap, c=cu, s=ns: check(
                lib.lddl_stream_cu_seqlens(_stream(), _ptr(p.doc_off), n_doc, _ptr(r), B, L, m,
                                           _ptr(c), _ptr(s)))
            meta['rows/' + key] = B * L * 32
            meta['plan/' + key + '/rows'] = n_rows
    us = {k: [] for k in calls}
    for rep in range(a.reps + 1):  # the first is the warm-up; the calls alternate
        for k, f in calls.items():
            t = timed(f, 2 if k.startswith('plan/') else a.inner)
            if rep:
                us[k].append(t)
    med = {k: statistics.median(v) for k, v in us.items()}
    res = {'build_id': lib.lddl_build_id().decode(), 'device': torch.cuda.get_device_name(0),
           'text_bytes': len(corp.text), 'sentences': n_sent, 'documents': n_doc,
           'tokens': int((sent_len & LEN_MASK).sum()), 'reps': a.reps, 'inner': a.inner,
           'us_per_call': med, 'us_per_call_min_max': {k: [min(v), max(v)] for k, v in us.items()},
           'plan_rows': {k[5:-5]: v for k, v in meta.items() if k.endswith('/rows')},
           'stored_gb_per_s': {k: meta[k] / med[k] / 1e3 for k in med if k in meta}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
