"""Measure the compact MLM targets against torch's own formulations on the same
build, in the same process, alternating call by call, after checking that the outputs agree.

(a) Compaction. HIP events around one call on labels [--rows, --seq] (p = --p masked, P = --P):
      hip_rows       compact_labels(layout='rows')  (lddl_mlm_compact_rows, one kernel)
      hip_flat       compact_labels(layout='flat')  (lddl_mlm_compact_flat, two kernels)
      torch_nonzero  (labels.view(-1) != ignore).nonzero() + the ids: WAITS FOR THE HOST, and its
                     shape changes from step to step; listed as what the others replace
      torch_cumsum   sync-free flat form: cumsum of the mask, scatter into capacity + 1 slots
      torch_sort     sync-free rows form: stable sort of the ignore flag per row, gather
    `host` is the time the Python call takes to return (enqueue only, except nonzero). The
    calls are shorter than the host's work to queue them, so every round of calls is queued
    behind a --fill-mib fill that keeps the stream busy, the sync-free variants take the place
    behind it in turn, and `gap` (previous end event to this start event) shows whether the
    stream ran dry; nonzero drains the stream by its nature and runs last in its round.
(b) Head step. An MLM-head-only training step on bf16 hidden states [rows, seq, --hidden]:
    dense(H, H) + GELU + LayerNorm + Linear(H, --vocab) + cross-entropy, forward and backward
    (the gradient reaches the hidden states), timed with HIP events
      dense       on every slot, labels with ignore_index
      rows        on hidden gathered by masked_lm_positions   (rows * P slots)
      flat        on hidden gathered by masked_lm_flat_positions, capacity rows * P
      flat_tight  the same with the capacity the flat form allows: the batch's mean count plus
                  six sigma (binomial over rows * seq slots), rounded up to a multiple of 8 * rows
    The targets are made once, outside the timed step ((a) times them).

Per variant: --reps repetitions of --inner timed calls after --warmup untimed ones; a
repetition's figure is the median of its calls, and the line gives the median, min and max of
those figures. Prints one JSON line and writes it to --out.

    python tools/mlm_compact_bench.py [--out profiles/mlm_compact.json] [--skip-head]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


# ---- torch's formulations ---------------------------------------------------------------------
def torch_nonzero(labels, ignore):
    flat = labels.view(-1)
    idx = (flat != ignore).nonzero().squeeze(1)  # the host waits here for the count
    return idx, flat[idx]


def torch_cumsum(labels, ignore, capacity):
    """compact_labels(layout='flat') without a host wait: the rank of a masked slot is the
    running count of the mask; unmasked and overflowing slots go to a dump slot past the end."""
    flat = labels.view(-1)
    m = flat != ignore
    rank = torch.cumsum(m, 0) - 1
    dst = torch.where(m & (rank < capacity), rank, capacity)
    src = torch.arange(flat.numel(), device=labels.device)
    pos = torch.zeros(capacity + 1, dtype=torch.int64, device=labels.device).scatter_(0, dst, src)
    ids = torch.full((capacity + 1,), ignore, dtype=torch.int64,
                     device=labels.device).scatter_(0, dst, flat)
    num = m.view(labels.shape).sum(1, dtype=torch.int32)
    return {'masked_lm_flat_positions': pos[:capacity], 'masked_lm_flat_ids': ids[:capacity],
            'num_masked': num, 'num_masked_total': num.sum(dtype=torch.int64).view(1)}


def torch_sort(labels, ignore, P):
    """compact_labels(layout='rows') without a host wait: a stable sort of the ignore flag moves
    the masked slots to the front of each row in position order."""
    L = labels.shape[1]
    m = labels != ignore
    order = torch.sort((~m).to(torch.int8), dim=1, stable=True).indices
    if P > L:
        order = torch.nn.functional.pad(order, (0, P - L))
    order = order[:, :P]
    num = m.sum(1, dtype=torch.int32)
    keep = torch.arange(P, device=labels.device)[None, :] < num[:, None]
    return {'masked_lm_positions': torch.where(keep, order, 0),
            'masked_lm_ids': torch.where(keep, labels.gather(1, order.clamp(max=L - 1)), ignore),
            'masked_lm_weights': keep.to(torch.float32), 'num_masked': num}


def make_labels(rows, seq, p, ignore, seed, device):
    g = torch.Generator().manual_seed(seed)
    lab = torch.where(torch.rand(rows, seq, generator=g) < p,
                      torch.randint(0, 30522, (rows, seq), generator=g), ignore)
    return lab.to(device)


# ---- timing -----------------------------------------------------------------------------------
def spread(per_rep):
    return {'median': round(float(np.median(per_rep)), 3), 'min': round(min(per_rep), 3),
            'max': round(max(per_rep), 3)}


def time_variants(variants, a, scale=1e3, fill=None, last=()):
    """variants: name -> callable. -> name -> {'dev': spread of the event time, 'host': spread of
    the time to return[, 'gap': spread of the time from the previous call's end event to this
    call's start event]}, in us (scale 1e3) or ms (scale 1).

    The compaction calls are shorter than the host's work to queue them, so events on an idle
    stream would time the host. With `fill` (a large tensor) every round of calls is queued
    behind a fill of it, the variants take the place behind the fill in turn, and `gap` shows
    whether the stream ran dry before a call (the launch gap if not). Variants in `last` (those
    that make the host wait, which drains the stream) run at the end of their round."""
    names = [v for v in variants if v not in last]
    for _ in range(a.warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    dev = {v: [] for v in variants}
    host = {v: [] for v in variants}
    gap = {v: [] for v in variants}
    for _ in range(a.reps):
        evs = {v: [] for v in variants}
        hs = {v: [] for v in variants}
        for i in range(a.inner):
            k = i % len(names)
            prev = None
            if fill is not None:
                fill.fill_(i)
                prev = torch.cuda.Event(enable_timing=True)
                prev.record()
            for v in names[k:] + names[:k] + list(last):  # alternating, call by call
                e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                e0.record()
                t0 = time.perf_counter()
                variants[v]()
                hs[v].append((time.perf_counter() - t0) * 1e3 * scale)
                e1.record()
                evs[v].append((prev, e0, e1))
                prev = e1
        torch.cuda.synchronize()
        for v in variants:
            dev[v].append(float(np.median([e0.elapsed_time(e1) * scale for _, e0, e1 in evs[v]])))
            host[v].append(float(np.median(hs[v])))
            if fill is not None:
                gap[v].append(float(np.median([p.elapsed_time(e0) * scale
                                               for p, e0, _ in evs[v]])))
    out = {v: {'dev': spread(dev[v]), 'host': spread(host[v])} for v in variants}
    if fill is not None:
        for v in variants:
            out[v]['gap'] = spread(gap[v])
    return out


def compaction(a):
    from lddl_amd.torch import compact_labels
    ign = a.ignore_index
    lab = make_labels(a.rows, a.seq, a.p, ign, a.seed, 'cuda')
    cap = a.rows * a.P
    rows, flat = compact_labels(lab, a.P, ign), compact_labels(lab, a.P, ign, 'flat')
    total = int(flat['num_masked_total'])
    idx, ids = torch_nonzero(lab, ign)
    k = min(total, cap)
    assert idx.numel() == total
    assert torch.equal(idx[:k], flat['masked_lm_flat_positions'][:k])
    assert torch.equal(ids[:k], flat['masked_lm_flat_ids'][:k])
    for name, got, ref in (('cumsum', torch_cumsum(lab, ign, cap), flat),
                           ('sort', torch_sort(lab, ign, a.P), rows)):
        assert set(got) == set(ref), name
        for key in ref:
            assert got[key].dtype == ref[key].dtype and torch.equal(got[key], ref[key]), \
                (name, key)
    variants = {'hip_rows': lambda: compact_labels(lab, a.P, ign),
                'hip_flat': lambda: compact_labels(lab, a.P, ign, 'flat'),
                'torch_nonzero': lambda: torch_nonzero(lab, ign),
                'torch_cumsum': lambda: torch_cumsum(lab, ign, cap),
                'torch_sort': lambda: torch_sort(lab, ign, a.P)}
    out = {'unit': 'us', 'masked_total': total, 'capacity': cap,
           'max_row_count': int(rows['num_masked'].max()), 'outputs_equal': True}
    fill = torch.empty(a.fill_mib << 20, dtype=torch.uint8, device='cuda')
    out['fill_mib'] = a.fill_mib
    out.update(time_variants(variants, a, fill=fill, last=('torch_nonzero',)))
    return out


# ---- the head step ----------------------------------------------------------------------------
class Head(torch.nn.Module):
    def __init__(self, hidden, vocab):
        super().__init__()
        self.dense = torch.nn.Linear(hidden, hidden)
        self.norm = torch.nn.LayerNorm(hidden)
        self.decoder = torch.nn.Linear(hidden, vocab)

    def forward(self, x):
        return self.decoder(self.norm(torch.nn.functional.gelu(self.dense(x))))


def tight_P(a):
    n = a.rows * a.seq
    cap = n * a.p + 6 * math.sqrt(n * a.p * (1 - a.p))
    return int(math.ceil(cap / (8 * a.rows))) * 8


def head_step(a):
    from lddl_amd.torch import compact_labels
    ign = a.ignore_index
    lab = make_labels(a.rows, a.seq, a.p, ign, a.seed, 'cuda')
    torch.manual_seed(a.seed)
    head = Head(a.hidden, a.vocab).cuda().to(torch.bfloat16)
    hidden = torch.randn(a.rows, a.seq, a.hidden, device='cuda', dtype=torch.bfloat16)
    hidden.requires_grad_(True)
    rows = compact_labels(lab, a.P, ign)
    flat = compact_labels(lab, a.P, ign, 'flat')
    Pt = tight_P(a)
    tight = compact_labels(lab, Pt, ign, 'flat')
    total = int(flat['num_masked_total'])
    assert int(rows['num_masked'].max()) <= a.P and total <= a.rows * Pt, 'overflow: raise --P'
    r_idx = torch.arange(a.rows, device='cuda')[:, None]
    ce = torch.nn.functional.cross_entropy
    losses = {}

    def step(name, x, y):
        hidden.grad = None
        for q in head.parameters():
            q.grad = None
        loss = ce(head(x).float(), y, ignore_index=ign, reduction='sum') / total
        loss.backward()
        losses[name] = loss.detach()

    def by_flat(t):
        return (hidden.view(-1, a.hidden).index_select(0, t['masked_lm_flat_positions']),
                t['masked_lm_flat_ids'])
    variants = {
        'dense': lambda: step('dense', hidden.view(-1, a.hidden), lab.view(-1)),
        'rows': lambda: step('rows', hidden[r_idx, rows['masked_lm_positions']].view(-1, a.hidden),
                             rows['masked_lm_ids'].view(-1)),
        'flat': lambda: step('flat', *by_flat(flat)),
        'flat_tight': lambda: step('flat_tight', *by_flat(tight)),
    }
    out = {'unit': 'ms', 'hidden': a.hidden, 'vocab': a.vocab, 'masked_total': total,
           'slots': {'dense': a.rows * a.seq, 'rows': a.rows * a.P, 'flat': a.rows * a.P,
                     'flat_tight': a.rows * Pt}, 'flat_tight_P': Pt}
    res = time_variants(variants, a, scale=1)
    out['loss'] = {k: round(float(v), 5) for k, v in losses.items()}
    ref = out['loss']['dense']  # the same sum over the same slots, in bf16 GEMMs of other shapes
    assert all(abs(v - ref) <= 1e-2 * abs(ref) for v in out['loss'].values()), out['loss']
    out.update({v: res[v]['dev'] for v in res})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=256)
    ap.add_argument('--seq', type=int, default=512)
    ap.add_argument('--p', type=float, default=0.15)
    ap.add_argument('--P', type=int, default=128)
    ap.add_argument('--ignore-index', type=int, default=-1)
    ap.add_argument('--hidden', type=int, default=1024)
    ap.add_argument('--vocab', type=int, default=30522)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--head-inner', type=int, default=5)
    ap.add_argument('--head-warmup', type=int, default=3)
    ap.add_argument('--seed', type=int, default=1234)
    ap.add_argument('--fill-mib', type=int, default=2048,
                    help='the fill queued ahead of every round of compaction calls')
    ap.add_argument('--skip-head', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mlm_compact_bench needs the GPU: there is nothing to time without it')
    from lddl_amd._native import lib
    res = {'build_id': lib.lddl_build_id().decode(), 'device': torch.cuda.get_device_name(0),
           'rows': a.rows, 'seq': a.seq, 'p': a.p, 'P': a.P, 'reps': a.reps, 'inner': a.inner,
           'warmup': a.warmup}
    res['compaction'] = compaction(a)
    if not a.skip_head:
        a.inner, a.warmup = a.head_inner, a.head_warmup
        res['head_inner'], res['head_warmup'] = a.inner, a.warmup
        res['head_step'] = head_step(a)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
