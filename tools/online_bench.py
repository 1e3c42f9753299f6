"""Measurements of the online loader. Two modes, one JSON line each (also written to
--out).

--mode kernel: `lddl_collate_pairs_masked` against the string path's `lddl_collate_encode_masked`
on the same batches of 256 samples at seq 512 (C5's shape; cased vocab), HIP events around the
one kernel each, the two alternating call by call. The pairs come from the synthetic corpus
(make_pairs, native rng); a batch is 256 rows of one bin of 64 tokens, the bins drawn in
proportion to their rows (what a binned loader yields), or 256 rows of the whole table
(`unbinned`). The string path gets the same rows rendered (output.render) and packed
(PackedBatch). Per set and variant: --reps repetitions of --inner timed calls per batch after
--warmup untimed ones; a repetition's figure is the sum over the batches of the median of the
batch's calls; the line gives the median, min and max of those figures, plain and whole-word.
The outputs of the two paths are compared (torch.equal) before anything is timed.

--mode loader: one epoch of get_bert_pretrain_online_data_loader over --corpus-bytes of synthetic
documents written to a temporary `source` directory, at --seq with --bin-size, batch 256,
dynamic masking, a consumer that only sums the attention mask on the device (so the figure is
the loader's ceiling, not a training step's). Reports samples/s and real token slots/s over the
epoch (host clock, ending in a device synchronise; the first epoch and a second one, which has
the code objects loaded), the median / p99 / longest time a next() call holds the caller, the
time the caller waits per round, and the peak HBM allocated (torch's allocator, which also
serves the library's temporaries).

    python tools/online_bench.py --mode kernel [--batches 8] [--reps 5] [--inner 20]
    python tools/online_bench.py --mode loader --seq 128 [--corpus-bytes 1000000000]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from lddl_amd._native import lib  # noqa: E402
from lddl_amd.context import Context  # noqa: E402

VOCAB_CASED = os.path.join(REPO, 'lddl_amd', 'assets', 'vocab_synth_cased_28996.txt')
SEQ, BATCH, BIN = 512, 256, 64


# ---- kernel ----------------------------------------------------------------------------------
def pair_table(a, ctx):
    from lddl_amd import synth
    from lddl_amd.pairs import make_pairs
    corp = synth.generate(seed=a.seed, n_bytes=a.table_bytes, nonascii_frac=0.01, threads=16)
    so = torch.from_numpy(corp.sent_off).cuda()
    ids, sl = ctx.tokenize(torch.from_numpy(corp.text).cuda(), so)
    part = np.linspace(0, corp.n_doc, 17).astype(np.int64)
    return make_pairs(ctx, so, ids, sl, torch.from_numpy(corp.doc_sent_off).cuda(),
                      torch.from_numpy(part).cuda(), torch.arange(1, 17).cuda(), seq=SEQ, dup=1,
                      masking=False, rng='native', native_seed=a.seed)


def make_row_sets(pb, n, seed):
    rng = np.random.default_rng(seed)
    nt = pb.num_tokens.cpu().numpy()
    bins = np.minimum((nt - 1) // BIN, SEQ // BIN - 1)
    ids = [b for b in range(SEQ // BIN) if (bins == b).sum() >= BATCH]
    w = np.asarray([(bins == b).sum() for b in ids], float)
    binned = [rng.choice(np.flatnonzero(bins == b), BATCH, replace=False)
              for b in rng.choice(ids, n, p=w / w.sum())]
    unbinned = [rng.choice(len(nt), BATCH, replace=False) for _ in range(n)]
    return {'binned': binned, 'unbinned': unbinned}, nt


def measure_kernel(a, ctx, pb, row_sets, nt):
    from lddl_amd import output
    from lddl_amd.torch.bert import encode_packed
    from lddl_amd.torch.online import collate_pairs
    from lddl_amd.torch.packing import PackedBatch
    items = []
    for idx in row_sets:
        rows = torch.from_numpy(np.asarray(idx, np.int64)).cuda()
        rd = output.render(ctx, pb, rows)
        pk = PackedBatch([(d['A'], d['B'], d['is_random_next'])
                          for d in (rd.row(r) for r in range(rd.n))])
        L = (int(nt[idx].max()) - 1) // 8 * 8 + 8
        items.append((pk, rows, L))

    def run(k, variant, ww, counter, timed):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if timed else None
        pk, rows, L = items[k]
        if variant == 'strings':
            return encode_packed(pk, ctx, 8, mask=(0.15, a.seed, counter), events=ev,
                                 whole_word=ww), ev
        if timed:
            ev[0].record()
        out = collate_pairs(ctx, pb, rows, 8, mask=(0.15, a.seed, counter), whole_word=ww,
                            seq_len=L, check=False)
        if timed:
            ev[1].record()
        return out, ev

    for k in range(len(items)):  # the two paths agree before they are timed
        for ww in (False, True):
            x, y = run(k, 'strings', ww, 5, False)[0], run(k, 'pairs', ww, 5, False)[0]
            assert set(x) == set(y) and all(torch.equal(x[key], y[key]) for key in x)
    variants = [(v, ww) for ww in (False, True) for v in ('strings', 'pairs')]
    for i in range(a.warmup):
        for k in range(len(items)):
            for v, ww in variants:
                run(k, v, ww, i, False)
    torch.cuda.synchronize()
    per_rep = {vw: [] for vw in variants}
    for r in range(a.reps):
        evs = {(vw, k): [] for vw in variants for k in range(len(items))}
        for i in range(a.inner):
            for k in range(len(items)):
                for vw in variants:
                    evs[vw, k].append(run(k, vw[0], vw[1], (r << 20) + i, True)[1])
        torch.cuda.synchronize()
        for vw in variants:
            per_rep[vw].append(sum(float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in
                                                    evs[vw, k]])) for k in range(len(items))))
    slots = sum(BATCH * L for _, _, L in items)
    out = {'slots': slots, 'real_tokens': int(sum(nt[idx].sum() for idx in row_sets)),
           'string_bytes': int(sum(len(pk.blob) for pk, _, _ in items))}
    for (v, ww), t in per_rep.items():
        out['{}{}'.format(v, '_ww' if ww else '')] = {
            'us': {'median': round(float(np.median(t)), 2), 'min': round(min(t), 2),
                   'max': round(max(t), 2)},
            'ns_per_slot': round(float(np.median(t)) * 1e3 / slots, 4)}
    return out


def mode_kernel(a):
    ctx = Context(VOCAB_CASED)
    pb = pair_table(a, ctx)
    sets, nt = make_row_sets(pb, a.batches, a.seed)
    res = {'tool': 'online_bench', 'mode': 'kernel', 'build_id': lib.lddl_build_id().decode(),
           'device': torch.cuda.get_device_name(0), 'seq': SEQ, 'batch': BATCH,
           'pairs_in_table': pb.n_pairs, 'batches': a.batches, 'reps': a.reps, 'inner': a.inner}
    for name, rs in sets.items():
        res[name] = measure_kernel(a, ctx, pb, rs, nt)
    return res


# ---- loader ----------------------------------------------------------------------------------
def write_source(a, root):
    from lddl_amd import synth
    src = os.path.join(root, 'source')
    os.makedirs(src)
    chunk, done, f = 128 << 20, 0, 0
    while done < a.corpus_bytes:
        n = min(chunk, a.corpus_bytes - done)
        text, doc_off = synth.generate_doc_text(seed=a.seed + f, n_bytes=n, doc_begin=f << 24,
                                                nonascii_frac=0.01, threads=16)
        raw = text.tobytes()
        with open(os.path.join(src, 'docs_{:03d}.txt'.format(f)), 'wb') as fh:
            fh.write(b''.join(b'doc-%d-%d ' % (f, d) + raw[doc_off[d]:doc_off[d + 1]] + b'\n'
                              for d in range(len(doc_off) - 1)))
        done += n
        f += 1
    return src


def run_epoch(loader):
    dev = torch.device('cuda', torch.cuda.current_device())
    real = torch.zeros((), dtype=torch.long, device=dev)
    loader.stats = {}
    waits, samples, slots, n = [], 0, 0, 0
    torch.cuda.synchronize()
    it = iter(loader)
    t0 = time.perf_counter()
    while True:
        t = time.perf_counter()
        b = next(it, None)
        waits.append(time.perf_counter() - t)
        if b is None:
            break
        real += b['attention_mask'].sum()
        samples += b['input_ids'].shape[0]
        slots += b['input_ids'].numel()
        n += 1
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    w = np.sort(np.asarray(waits[:-1] or [0.0]))
    return {'seconds': round(sec, 3), 'batches': n, 'samples': samples,
            'samples_per_s': round(samples / sec, 1), 'real_token_slots': int(real.item()),
            'real_token_slots_per_s': round(int(real.item()) / sec, 1), 'slots': slots,
            'rounds': loader.num_rounds, 'dropped_samples': loader.dropped_samples,
            'next_ms': {'median': round(float(np.median(w)) * 1e3, 4),
                        'p99': round(float(w[int(0.99 * (len(w) - 1))]) * 1e3, 3),
                        'max': round(float(w[-1]) * 1e3, 3)},
            'round_wait_ms': [round(x * 1e3, 1) for x in loader.stats.get('round_wait_s', [])],
            'round_cut_ms': [round(x * 1e3, 1) for x in loader.stats.get('round_cut_s', [])]}


def mode_loader(a):
    from lddl_amd.torch import get_bert_pretrain_online_data_loader
    root = tempfile.mkdtemp(prefix='online_bench_', dir=a.tmp)
    try:
        t0 = time.perf_counter()
        src = write_source(a, root)
        gen_s = time.perf_counter() - t0
        loader = get_bert_pretrain_online_data_loader(
            books=src, vocab_file=VOCAB_CASED, batch_size=BATCH, target_seq_length=a.seq,
            bin_size=a.bin_size, block_size=a.block_size, gpu_batch_bytes=a.gpu_batch_bytes,
            base_seed=a.seed, tokenizer_kwargs={'do_lower_case': True})
        res = {'tool': 'online_bench', 'mode': 'loader', 'build_id': lib.lddl_build_id().decode(),
               'device': torch.cuda.get_device_name(0), 'seq': a.seq, 'bin_size': a.bin_size,
               'batch': BATCH, 'corpus_bytes': a.corpus_bytes, 'block_size': a.block_size,
               'gpu_batch_bytes': a.gpu_batch_bytes, 'write_source_s': round(gen_s, 2),
               'epochs': []}
        for _ in range(a.epochs):
            torch.cuda.reset_peak_memory_stats()
            e = run_epoch(loader)
            e['peak_hbm_bytes'] = int(torch.cuda.max_memory_allocated())
            res['epochs'].append(e)
        return res
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=['kernel', 'loader'], required=True)
    ap.add_argument('--seed', type=int, default=1234)
    ap.add_argument('--out', default=None)
    # kernel
    ap.add_argument('--table-bytes', type=int, default=48 << 20)
    ap.add_argument('--batches', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    # loader
    ap.add_argument('--seq', type=int, default=128)
    ap.add_argument('--bin-size', type=int, default=8)
    ap.add_argument('--corpus-bytes', type=int, default=1_000_000_000)
    ap.add_argument('--block-size', type=int, default=1 << 20)
    ap.add_argument('--gpu-batch-bytes', type=int, default=64 << 20)
    ap.add_argument('--epochs', type=int, default=2)
    ap.add_argument('--tmp', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('online_bench needs the GPU: there is nothing to measure without one')
    res = mode_kernel(a) if a.mode == 'kernel' else mode_loader(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
