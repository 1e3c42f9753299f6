"""Time the loader's fused dynamic-masking collate unpacked and sequence-packed on
the same batches: `encode_packed(mask=..., events=...)` against `encode_seqpacked(...)`, i.e. HIP
events around the one kernel each (lddl_collate_encode_masked / lddl_collate_seqpack_masked), the
two alternating call by call.

The batches are C5's (bench.py --workload c5): 256 samples of the seq-512 dataset that the
preprocessor CLI writes from the synthetic corpus (cased vocab, 8 bins, dynamic masking), from a
smaller corpus by default (--corpus-bytes). Two sets of --batches batches each:
`binned`, each batch from one bin, the bins drawn in proportion to their samples (what the C5
loader yields), and `unbinned`, each batch from all samples (a dataset preprocessed without
bins). Per set and variant: --reps repetitions of --inner timed calls per batch after --warmup
untimed ones; a repetition's figure is the sum over the batches of the median of the batch's
calls, and the line gives the median, min and max of those figures (the spread within the run),
with the rows, the share of real slots and the bytes written per real token (4 int64 tensors per
slot unpacked, 6 packed). Prints one JSON line and writes it to --out.

    python tools/seqpack_bench.py [--batches 8] [--reps 5] [--inner 20] [--out profiles/...]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402  (the C5 dataset recipe)
from lddl_amd._native import lib  # noqa: E402
from lddl_amd.context import Context  # noqa: E402
from lddl_amd.torch.bert import encode_packed, encode_seqpacked  # noqa: E402
from lddl_amd.torch.packing import PackedBatch  # noqa: E402
from lddl_amd.torch.seqpack import SeqPackedBatch  # noqa: E402
from lddl_amd.utils import (get_all_bin_ids, get_all_parquets_under,  # noqa: E402
                            get_file_paths_for_bin_id)

SEQ, BATCH = 512, 256


def c5_samples(a, root):
    """{bin id: [(A, B, is_random_next)]} of the C5 dataset."""
    import pyarrow.parquet as pq
    ns = argparse.Namespace(seed=a.seed, c5_corpus_bytes=a.corpus_bytes, gen_threads=16,
                            c5_bin_size=64, c5_workers=2)
    paths = get_all_parquets_under(bench.c5_dataset(ns, root))
    bins = {}
    for b in get_all_bin_ids(paths):
        rows = []
        for p in get_file_paths_for_bin_id(paths, b):
            t = pq.read_table(p, columns=['A', 'B', 'is_random_next']).to_pydict()
            rows += list(zip(t['A'], t['B'], t['is_random_next']))
        bins[b] = rows
    return bins


def make_batches(bins, n, seed):
    rng = np.random.default_rng(seed)
    ids = sorted(b for b in bins if len(bins[b]) >= BATCH)
    w = np.asarray([len(bins[b]) for b in ids], float)
    binned = []
    for b in rng.choice(ids, n, p=w / w.sum()):
        binned.append([bins[b][j] for j in rng.choice(len(bins[b]), BATCH, replace=False)])
    pool = [s for b in sorted(bins) for s in bins[b]]
    unbinned = [[pool[j] for j in rng.choice(len(pool), BATCH, replace=False)] for _ in range(n)]
    return {'binned': binned, 'unbinned': unbinned}


def measure(a, ctx, batches):
    pks = [(PackedBatch(b), SeqPackedBatch(b, SEQ)) for b in batches]

    def run(k, variant, counter, timed):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if timed else None
        pk, spk = pks[k]
        if variant == 'unpacked':
            encode_packed(pk, ctx, 8, mask=(0.15, a.seed, counter), events=ev)
        else:
            encode_seqpacked(spk, ctx, SEQ, 8, mask=(0.15, a.seed, counter), events=ev)
        return ev

    variants = ('unpacked', 'packed')
    for i in range(a.warmup):
        for k in range(len(pks)):
            for v in variants:
                run(k, v, i, False)
    torch.cuda.synchronize()
    per_rep = {v: [] for v in variants}
    for r in range(a.reps):
        evs = {(v, k): [] for v in variants for k in range(len(pks))}
        for i in range(a.inner):
            for k in range(len(pks)):
                for v in variants:
                    evs[v, k].append(run(k, v, (r << 20) + i, True))
        torch.cuda.synchronize()
        for v in variants:
            per_rep[v].append(sum(float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in
                                                   evs[v, k]])) for k in range(len(pks))))
    real = sum(int((pk.na + pk.nb + 3).sum()) for pk, _ in pks)
    slots = {'unpacked': sum(BATCH * ((int((pk.na + pk.nb).max()) + 3 + 7) // 8 * 8)
                             for pk, _ in pks),
             'packed': sum(spk.plan.R * SEQ for _, spk in pks)}
    out = {'real_tokens': real}
    for v, tensors in zip(variants, (4, 6)):
        t = per_rep[v]
        out[v] = {'rows': slots[v] // SEQ if v == 'packed' else BATCH * len(pks),
                  'slots': slots[v], 'real_share': round(real / slots[v], 4),
                  'bytes_written_per_real_token': round(8 * tensors * slots[v] / real, 2),
                  'us': {'median': round(float(np.median(t)), 2), 'min': round(min(t), 2),
                         'max': round(max(t), 2)},
                  'ns_per_real_token': round(float(np.median(t)) * 1e3 / real, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--seed', type=int, default=1234)
    ap.add_argument('--corpus-bytes', type=int, default=24 << 20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    root = tempfile.mkdtemp(prefix='lddl_seqpack_', dir=os.environ.get('TMPDIR', '/tmp'))
    try:
        bins = c5_samples(a, root)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    ctx = Context(bench.VOCAB_CASED, do_lower_case=False)
    res = {'build_id': lib.lddl_build_id().decode(), 'device': torch.cuda.get_device_name(0),
           'batch': BATCH, 'seq': SEQ, 'batches': a.batches, 'reps': a.reps, 'inner': a.inner,
           'warmup': a.warmup, 'corpus_bytes': a.corpus_bytes,
           'samples_per_bin': {str(b): len(bins[b]) for b in sorted(bins)}}
    for name, batches in make_batches(bins, a.batches, a.seed).items():
        res[name] = measure(a, ctx, batches)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
