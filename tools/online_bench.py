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

--max-seq-length N measures sequence packing instead. --mode kernel:
`lddl_collate_pairs_seqpack_masked` into rows of N slots, planned by `lddl_seqpack_plan`, against
`lddl_collate_pairs_masked` on the same rows, by the same method (every sample's packed segment
compared with its unpacked row first), with the bytes each writes per real token, and the
planner's one launch for all the batches. --mode loader: the packed loader, the unpacked loader
unbinned and the unpacked loader with --bin-size, the three alternating epoch by epoch over the
same source; per epoch also the rows yielded, the real share of the slots and the device time of
each round's row planner (events around its launch).

    python tools/online_bench.py --mode kernel [--batches 8] [--reps 5] [--inner 20]
    python tools/online_bench.py --mode loader --seq 128 [--corpus-bytes 1000000000]
    python tools/online_bench.py --mode kernel --max-seq-length 512
    python tools/online_bench.py --mode loader --seq 512 --bin-size 8 --max-seq-length 512
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


def measure_seqpack(a, ctx, pb, row_sets, nt):
    """lddl_collate_pairs_seqpack_masked (rows of --max-seq-length slots, planned by
    lddl_seqpack_plan) against lddl_collate_pairs_masked on the same rows, and the planner's one
    launch for all the batches."""
    from lddl_amd.torch.online import collate_pairs, collate_pairs_seqpacked, plan_rows_device
    cap = a.max_seq_length
    rows = torch.from_numpy(np.concatenate(row_sets).astype(np.int64)).cuda()
    off = np.arange(len(row_sets) + 1) * BATCH
    plan = plan_rows_device(ctx, pb, rows, off, cap, clamp=False)
    R = plan.num_rows.tolist()
    strides = [(int(nt[idx].max()) - 1) // 8 * 8 + 8 for idx in row_sets]

    def run(k, variant, ww, counter, timed):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if timed else None
        if timed:
            ev[0].record()
        if variant == 'pairs':
            out = collate_pairs(ctx, pb, rows[off[k]:off[k + 1]], 8, mask=(0.15, a.seed, counter),
                                whole_word=ww, seq_len=strides[k], check=False)
        else:
            out = collate_pairs_seqpacked(ctx, pb, rows, plan, k, R[k], cap, strides[k],
                                          mask=(0.15, a.seed, counter), whole_word=ww,
                                          check=False)
        if timed:
            ev[1].record()
        return out, ev

    for k in range(len(row_sets)):  # every sample's segment is its unpacked row, before timing
        lens = pb.num_tokens[rows[off[k]:off[k + 1]]]
        x = torch.arange(strides[k], device='cuda')[None, :]
        real = x < lens[:, None]
        at = (plan.dst[off[k]:off[k + 1], None] + x)[real]
        for ww in (False, True):
            u, p = run(k, 'pairs', ww, 5, False)[0], run(k, 'seqpack', ww, 5, False)[0]
            for key in ('input_ids', 'token_type_ids', 'labels'):
                assert torch.equal(p[key].view(-1)[at], u[key][real]), key
            assert int(p['attention_mask'].sum()) == int(lens.sum())
            assert int(p['attention_mask'].view(-1)[at].sum()) == int(lens.sum())
    variants = [(v, ww) for ww in (False, True) for v in ('pairs', 'seqpack')]
    for i in range(a.warmup):
        for k in range(len(row_sets)):
            for v, ww in variants:
                run(k, v, ww, i, False)
    torch.cuda.synchronize()
    # These kernels are shorter than the host's work per call, so events around a call on an idle
    # stream would time the host. A 1 GiB fill ahead of every group of four calls keeps the
    # stream busy while the host queues them; `gap_us`, the time from one call's end event to
    # the next call's start event, shows whether it did (it is then the launch gap alone).
    blocker = torch.empty(1 << 30, dtype=torch.uint8, device='cuda')
    per_rep, plan_us, gaps = {vw: [] for vw in variants}, [], []
    for r in range(a.reps):
        evs = {(vw, k): [] for vw in variants for k in range(len(row_sets))}
        pev, groups = [], []
        for i in range(a.inner):
            for k in range(len(row_sets)):
                blocker.zero_()
                s = (i + k) % len(variants)  # each variant comes first behind the fill in turn
                order = variants[s:] + variants[:s]
                groups.append([run(k, vw[0], vw[1], (r << 20) + i, True)[1] for vw in order])
                for vw, ev in zip(order, groups[-1]):
                    evs[vw, k].append(ev)
            pev.append([torch.cuda.Event(enable_timing=True) for _ in range(2)])
            plan_rows_device(ctx, pb, rows, off, cap, clamp=False, events=pev[-1])
        torch.cuda.synchronize()
        for vw in variants:
            per_rep[vw].append(sum(float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in
                                                    evs[vw, k]])) for k in range(len(row_sets))))
        plan_us.append(float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in pev])))
        gaps += [x[1].elapsed_time(y[0]) * 1e3 for g in groups for x, y in zip(g, g[1:])]
    real_tokens = int(sum(nt[idx].sum() for idx in row_sets))
    slots = {'pairs': sum(BATCH * s for s in strides), 'seqpack': sum(R) * cap}
    # int64 outputs: 4 per slot unpacked (ids, types, attention, labels) + nsl per sample; 6 per
    # slot packed (+ position_ids, sequence_ids) + nsl, cls_positions, seq_lens per sample
    written = {'pairs': slots['pairs'] * 32 + len(row_sets) * BATCH * 8,
               'seqpack': slots['seqpack'] * 48 + len(row_sets) * BATCH * 20}
    out = {'max_seq_length': cap, 'real_tokens': real_tokens, 'rows': {'pairs': len(row_sets) * BATCH,
                                                                        'seqpack': sum(R)},
           'slots': slots, 'real_share': {v: round(real_tokens / slots[v], 4) for v in slots},
           'plan_us': {'median': round(float(np.median(plan_us)), 2),
                       'min': round(min(plan_us), 2), 'max': round(max(plan_us), 2)},
           'gap_us': {'median': round(float(np.median(gaps)), 2),
                      'p99': round(float(np.sort(gaps)[int(0.99 * (len(gaps) - 1))]), 2)}}
    for (v, ww), t in per_rep.items():
        out['{}{}'.format(v, '_ww' if ww else '')] = {
            'us': {'median': round(float(np.median(t)), 2), 'min': round(min(t), 2),
                   'max': round(max(t), 2)},
            'us_per_1k_real_tokens': round(float(np.median(t)) * 1e3 / real_tokens, 4),
            'bytes_written_per_real_token': round(written[v] / real_tokens, 2)}
    return out


def mode_kernel(a):
    ctx = Context(VOCAB_CASED)
    pb = pair_table(a, ctx)
    sets, nt = make_row_sets(pb, a.batches, a.seed)
    res = {'tool': 'online_bench', 'mode': 'kernel', 'build_id': lib.lddl_build_id().decode(),
           'device': torch.cuda.get_device_name(0), 'seq': SEQ, 'batch': BATCH,
           'pairs_in_table': pb.n_pairs, 'batches': a.batches, 'reps': a.reps, 'inner': a.inner}
    for name, rs in sets.items():
        if a.max_seq_length is None:
            res[name] = measure_kernel(a, ctx, pb, rs, nt)
        else:
            res[name] = measure_seqpack(a, ctx, pb, rs, nt)
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
    waits, samples, rows, slots, n = [], 0, 0, 0, 0
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
        samples += b['next_sentence_labels'].shape[0]
        rows += b['input_ids'].shape[0]
        slots += b['input_ids'].numel()
        n += 1
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    w = np.sort(np.asarray(waits[:-1] or [0.0]))
    plan_ms = [round(e0.elapsed_time(e1), 4) for e0, e1 in loader.stats.get('plan_events', [])]
    return {'seconds': round(sec, 3), 'batches': n, 'samples': samples, 'rows': rows,
            'real_share_of_slots': round(int(real.item()) / max(slots, 1), 4),
            'plan_device_ms': plan_ms,
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
        kw = dict(books=src, vocab_file=VOCAB_CASED, batch_size=BATCH, target_seq_length=a.seq,
                  block_size=a.block_size, gpu_batch_bytes=a.gpu_batch_bytes, base_seed=a.seed,
                  tokenizer_kwargs={'do_lower_case': True})
        res = {'tool': 'online_bench', 'mode': 'loader', 'build_id': lib.lddl_build_id().decode(),
               'device': torch.cuda.get_device_name(0), 'seq': a.seq, 'bin_size': a.bin_size,
               'batch': BATCH, 'corpus_bytes': a.corpus_bytes, 'block_size': a.block_size,
               'gpu_batch_bytes': a.gpu_batch_bytes, 'write_source_s': round(gen_s, 2)}
        if a.max_seq_length is None:
            loaders = {'epochs': get_bert_pretrain_online_data_loader(bin_size=a.bin_size, **kw)}
        else:
            # packed against unpacked-unbinned against unpacked-binned, the three alternating
            # epoch by epoch (epoch e of each has the same seed, so the same pairs)
            from lddl_amd.torch import get_bert_pretrain_online_packed_data_loader
            res['max_seq_length'] = a.max_seq_length
            loaders = {
                'packed': get_bert_pretrain_online_packed_data_loader(a.max_seq_length, **kw),
                'unbinned': get_bert_pretrain_online_data_loader(bin_size=None, **kw),
                'binned': get_bert_pretrain_online_data_loader(bin_size=a.bin_size, **kw)}
        for name in loaders:
            res[name] = []
        for _ in range(a.epochs):
            for name, loader in loaders.items():
                torch.cuda.reset_peak_memory_stats()
                e = run_epoch(loader)
                e['peak_hbm_bytes'] = int(torch.cuda.max_memory_allocated())
                res[name].append(e)
            if a.max_seq_length is not None:  # the same samples, rearranged
                p, u = res['packed'][-1], res['unbinned'][-1]
                assert (p['samples'], p['real_token_slots'], p['batches']) == \
                    (u['samples'], u['real_token_slots'], u['batches'])
        return res
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=['kernel', 'loader'], required=True)
    ap.add_argument('--seed', type=int, default=1234)
    ap.add_argument('--out', default=None)
    ap.add_argument('--max-seq-length', type=int, default=None,
                    help='measure sequence packing into rows of this many slots (DESIGN §19)')
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
