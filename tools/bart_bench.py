"""Time the BART path's GPU stages on synthetic raw documents: HIP events around punkt.segment
(lddl_segment_count + fill) and around bart.aggregate (lddl_bart_count + fill) on the same batch,
with the aggregate stage's algorithmic traffic; with --cli, also one end-to-end
`preprocess_bart_pretrain` run over the same text written as source files, with its host wall
time per stage.

    python tools/bart_bench.py [--gib 1.0] [--target-seq-length 128] [--cli] [--format parquet]
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
from lddl_amd import bart, punkt, synth  # noqa: E402
from lddl_amd._native import lib  # noqa: E402
from lddl_amd.context import Context  # noqa: E402

HBM_PEAK = 8.0e12  # MI355X, bytes/s


def timed(fn, warmup=2, reps=5):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        del out
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return out, ms


def cli_run(text, doc_off, a):
    from lddl_amd.dask.bart import pretrain as P
    root = tempfile.mkdtemp(prefix='lddl_bart_', dir=os.environ.get('TMPDIR', '/tmp'))
    try:
        src = os.path.join(root, 'source', 'en')
        os.makedirs(src)
        n_doc = len(doc_off) - 1
        per = (n_doc + a.files - 1) // a.files
        for f in range(a.files):
            with open(os.path.join(src, 'wiki_{}.txt'.format(f)), 'wb') as fh:
                for d in range(f * per, min(n_doc, (f + 1) * per)):
                    fh.write(b'wiki-%d ' % d + text[doc_off[d]:doc_off[d + 1]].tobytes() + b'\n')
        src_bytes = sum(os.path.getsize(os.path.join(src, x)) for x in os.listdir(src))
        with open(os.path.join(root, 'punkt.json'), 'w') as f:
            f.write('{}')
        argv = ['--schedule', 'local', '--wikipedia', os.path.join(root, 'source'), '--sink',
                os.path.join(root, 'out'), '--target-seq-length', str(a.target_seq_length),
                '--num-blocks', str(a.num_blocks), '--output-format', a.format, '--punkt-params',
                os.path.join(root, 'punkt.json')]
        t0 = time.perf_counter()
        n_files = P.main(P.attach_args().parse_args(argv))
        wall = time.perf_counter() - t0
        out = os.path.join(root, 'out')
        return {'source_bytes': src_bytes, 'cli_wall_s': round(wall, 3),
                'source_MB_per_s': round(src_bytes / wall / 1e6, 1), 'files': n_files,
                'output_bytes': sum(os.path.getsize(os.path.join(out, x)) for x in os.listdir(out)),
                'stage_seconds': {k: round(v, 3) for k, v in P.last_stage_seconds.items()},
                'argv': argv[argv.index('--target-seq-length'):-2]}
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gib', type=float, default=1.0)
    ap.add_argument('--target-seq-length', type=int, default=128)
    ap.add_argument('--cli', action='store_true')
    ap.add_argument('--format', default='parquet', choices=['parquet', 'txt'])
    ap.add_argument('--num-blocks', type=int, default=128)
    ap.add_argument('--files', type=int, default=16)
    a = ap.parse_args()
    text, doc_off = synth.generate_doc_text(seed=1234, n_bytes=int(a.gib * (1 << 30)),
                                            nonascii_frac=0.01, threads=16)
    ctx = Context(os.path.join(REPO, 'lddl_amd', 'assets', 'vocab_synth_uncased_30522.txt'))
    punkt.set_params(ctx, None)
    t = torch.from_numpy(text).cuda()
    d = torch.from_numpy(doc_off).cuda()
    (so, ds), seg_ms = timed(lambda: punkt.segment(ctx, t, d))
    (out, co, nt, dco), agg_ms = timed(lambda: bart.aggregate(ctx, t, so, ds, a.target_seq_length))
    n_sent, n_doc, n_chunks = so.numel() - 1, ds.numel() - 1, co.numel() - 1
    # text read by the statistics and by the fill, the chunk bytes written, and the tables per
    # sentence (sent_off twice, three int32 statistics written and read, the destination scan
    # written and read twice), per document and per chunk
    traffic = 2 * t.numel() + out.numel() + n_sent * (2 * 8 + 3 * 4 * 2 + 8 * 3) + \
        n_doc * (8 + 4 * 2 + 8 * 2) + n_chunks * (8 + 4) * 2
    res = {
        'build_id': lib.lddl_build_id().decode(), 'device': torch.cuda.get_device_name(0),
        'input_bytes': int(t.numel()), 'documents': n_doc, 'sentences': n_sent, 'chunks': n_chunks,
        'output_bytes': int(out.numel()), 'target_seq_length': a.target_seq_length,
        'segment_ms': {'min': round(min(seg_ms), 3), 'mean': round(float(np.mean(seg_ms)), 3),
                       'input_GB_per_s': round(t.numel() / min(seg_ms) / 1e6, 1)},
        'aggregate_ms': {'min': round(min(agg_ms), 3), 'mean': round(float(np.mean(agg_ms)), 3),
                         'input_GB_per_s': round(t.numel() / min(agg_ms) / 1e6, 1)},
        'aggregate_traffic_bytes': int(traffic),
        'aggregate_fraction_of_hbm_peak': round(traffic / (min(agg_ms) * 1e-3) / HBM_PEAK, 4),
    }
    print(json.dumps(res), flush=True)
    if a.cli:
        del out, co, nt, dco, so, ds, t, d
        print(json.dumps({'cli': cli_run(text, doc_off, a)}), flush=True)


if __name__ == '__main__':
    main()
