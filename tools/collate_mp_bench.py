"""Time the static-masking collate with and without the loss mask, on one synthetic batch that
stays on the device: HIP events around `--inner` back-to-back calls of

  1. lddl_collate_encode;
  2. lddl_collate_encode_mp (the same kernel also writes the [B, L] loss mask);
  3. lddl_collate_encode, then torch.zeros + scatter_ over precomputed flat indices (the
     loss mask as a second pass, which the kernel's extra store replaces),

the three alternating within every repetition. Prints one JSON line: per-call microseconds
(min and median over the repetitions), the ratios and the bytes each variant writes.

    python tools/collate_mp_bench.py [--batch 256] [--seq 512] [--reps 30] [--inner 200]
"""
import argparse
import io
import json
import os
import random
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from lddl_amd._native import check, lib  # noqa: E402
from lddl_amd.context import Context, _ptr, _stream  # noqa: E402
from lddl_amd.torch.packing import PackedBatch  # noqa: E402


def make_batch(vocab_file, B, L, seed=5):
    """B static-masking samples of 3/4 L .. L tokens (the longest exactly L), 15% masked."""
    with open(vocab_file, encoding='utf-8') as f:
        words = [w for w in (l.rstrip('\n') for l in f) if w and not w.startswith('[')][1000:6000]
    rng = random.Random(seed)
    batch = []
    for b in range(B):
        n = L - 3 if b == 0 else rng.randint(3 * L // 4, L) - 3
        na = rng.randint(1, n - 1)
        A = [rng.choice(words) for _ in range(na)]
        Bt = [rng.choice(words) for _ in range(n - na)]
        seq = ['[CLS]'] + A + ['[SEP]'] + Bt + ['[SEP]']
        cand = [i for i in range(1, n + 2) if i != na + 1]
        pos = sorted(rng.sample(cand, max(1, int(0.15 * n))))
        bio = io.BytesIO()
        np.save(bio, np.asarray(pos, np.uint16))
        batch.append((' '.join(A), ' '.join(Bt), rng.random() < 0.5, bio.getvalue(),
                      ' '.join(seq[p] for p in pos)))
    return batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--seq', type=int, default=512)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--inner', type=int, default=200)
    a = ap.parse_args()
    vocab = os.path.join(REPO, 'lddl_amd', 'assets', 'vocab_synth_uncased_30522.txt')
    ctx = Context(vocab)
    dev = ctx.device
    pk = PackedBatch(make_batch(vocab, a.batch, a.seq))
    B, L = len(pk), int((pk.na + pk.nb).max()) + 3
    assert L == a.seq
    lab_off, pos, pos_off = pk.extra
    rows = np.repeat(np.arange(B, dtype=np.int64), np.diff(pos_off))
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in dict(
        blob=pk.blob, a=pk.a_off, b=pk.b_off, na=pk.na, nb=pk.nb, lab_off=lab_off,
        pos=pos.view(np.int16), pos_off=pos_off, flat=rows * L + pos.astype(np.int64)).items()}
    o = {k: torch.empty(B, L, dtype=torch.long, device=dev)
         for k in ('input_ids', 'token_type_ids', 'attention_mask', 'labels', 'loss_mask')}
    args = (ctx.handle, _stream(), _ptr(t['blob']), _ptr(t['a']), _ptr(t['b']), _ptr(t['na']),
            _ptr(t['nb']), B, L, _ptr(o['input_ids']), _ptr(o['token_type_ids']),
            _ptr(o['attention_mask']), None, _ptr(t['blob']), _ptr(t['lab_off']), _ptr(t['pos']),
            _ptr(t['pos_off']), _ptr(o['labels']), -1)
    ones = torch.ones_like(t['flat'])
    two_pass = [None]

    def plain():
        check(lib.lddl_collate_encode(*args))

    def fused():
        check(lib.lddl_collate_encode_mp(*args, _ptr(o['loss_mask'])))

    def scatter():
        check(lib.lddl_collate_encode(*args))
        two_pass[0] = torch.zeros(B * L, dtype=torch.long, device=dev).scatter_(0, t['flat'], ones)

    variants = (('encode', plain), ('encode_mp', fused), ('encode_then_scatter', scatter))
    for _, fn in variants:  # warm up; the two loss masks must agree before anything is timed
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    assert torch.equal(two_pass[0].view(B, L), o['loss_mask'])
    us = {name: [] for name, _ in variants}
    for _ in range(a.reps):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / a.inner)
    slot = B * L * 8
    res = {'build_id': lib.lddl_build_id().decode(), 'device': torch.cuda.get_device_name(0),
           'batch': B, 'seq': L, 'masked_positions': int(len(pos)), 'reps': a.reps,
           'inner': a.inner,
           'us_per_call': {k: {'min': round(min(v), 2), 'median': round(float(np.median(v)), 2)}
                           for k, v in us.items()},
           'bytes_written': {'encode': 4 * slot, 'encode_mp': 5 * slot,
                             'encode_then_scatter': 5 * slot + 8 * int(len(pos))}}
    m = {k: float(np.median(v)) for k, v in us.items()}
    res['mp_over_encode'] = round(m['encode_mp'] / m['encode'], 3)
    res['mp_over_scatter'] = round(m['encode_mp'] / m['encode_then_scatter'], 3)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
