"""`preprocess_bart_pretrain` — drop-in for the reference's `lddl.dask.bart.pretrain`
(lddl/dask/bart/pretrain.py:41-290): same flags, same output files, GPU data plane.

Pipeline:
  read `*.txt` sources into blocks, strip lines, drop empty ones
    (readers.py:60-71; wikipedia, books, common crawl, open webtext
    concatenated in that order, pretrain.py:57-80)            -> lddl_amd.dask.readers (host)
  the article is the WHOLE stripped line (no split_id_text: the
    leading id is text and counts as a word)
  strict UTF-8 decode of every block (dask.bag.read_text)      -> lddl_utf8_check (HIP)
  sent_tokenize + strip + drop empty (82-86)                   -> lddl_segment_* (HIP Punkt)
  _aggregate_sentences (88-128)                                -> lddl_bart_count / fill (HIP)
  to_parquet(write_index=False) / to_textfiles (136-152)       -> pyarrow / text writer (host)

There is no RNG, sampling or shuffle: the output is a function of the input files and the block
size only. `--short-seq-prob` is accepted and unused, as in the reference. `--schedule`,
`--local-n-workers` and `--local-threads-per-worker` are accepted and ignored: one process, one
GPU (multi-rank sharding of the BART output is out of scope).

Partitions are processed in GPU batches of whole partitions (<= --gpu-batch-bytes of input);
the read of the next batch and the file writes of the previous one overlap the GPU work. The
lines are read by `readers.read_block` in a thread pool (the native C++ reader has no whole-line
mode), so the end-to-end rate is bound by the reader.
"""
import argparse
import functools
import json
import os
import sys
import time

import numpy as np

from ...utils import expand_outdir_and_mkdir, parse_str_of_num_bytes
from .. import readers
from ..bert.corpus import ASSETS, greedy, prefetch, punkt_params
from ..bert.writers import pad_name


def plan_partitions(args):
    """Every partition of the corpus as an unread readers.Block, in the reference's partition
    order (db.concat of the four bags, pretrain.py:57-80, 133)."""
    blocksize = args.block_size
    if args.num_blocks is not None:
        if blocksize is not None:
            raise ValueError('Only one of num_blocks or blocksize needs to be set!')
        blocksize = readers.estimate_block_size(
            (args.wikipedia, args.books, args.common_crawl, args.open_webtext), args.num_blocks)
    blocks = []
    if args.wikipedia is not None:
        blocks += readers.plan_blocks(readers.wikipedia_dir(args.wikipedia, args.wikipedia_lang),
                                      blocksize)
    for path in (args.books, args.common_crawl, args.open_webtext):
        if path is not None:
            blocks += readers.plan_blocks(path, blocksize)
    return blocks


def iter_batches(args, blocks, pool):
    """GPU batches of whole partitions: yields ([partition numbers], text uint8, doc_off int64,
    part_doc_off int64); a document is one whole stripped line."""
    for batch in greedy(list(range(len(blocks))), lambda p: blocks[p].nbytes,
                        args.gpu_batch_bytes):
        parts = list(pool.map(lambda p: readers.read_block(blocks[p], as_bytes=True), batch))
        lines = [x for ls in parts for x in ls]
        text = np.frombuffer(b''.join(lines), np.uint8) if lines else np.zeros(0, np.uint8)
        doc_off = np.zeros(len(lines) + 1, np.int64)
        np.cumsum(np.fromiter(map(len, lines), np.int64, len(lines)), out=doc_off[1:])
        part_doc_off = np.zeros(len(parts) + 1, np.int64)
        np.cumsum([len(ls) for ls in parts], out=part_doc_off[1:])
        yield batch, text, doc_off, part_doc_off


def batch_chunks(ctx, args, text, doc_off, part_doc_off, timer=None):
    """The GPU path over one batch -> host (bytes uint8, chunk_off int64, part_chunk_off int64):
    partition i of the batch holds chunks part_chunk_off[i]:part_chunk_off[i+1]."""
    import torch
    from ... import bart, punkt
    tm = timer or (lambda name: None)
    dev = ctx.device
    d_text = torch.from_numpy(text).to(dev) if len(text) else torch.zeros(
        1, dtype=torch.uint8, device=dev)[:0]
    d_doc = torch.from_numpy(doc_off).to(dev)
    tm('h2d')
    bad = punkt.utf8_first_invalid(d_text)
    if bad >= 0:  # dask.bag.read_text decodes strictly: the reference raises here too
        raise UnicodeDecodeError('utf-8', bytes(text[max(bad - 8, 0):bad + 8]), min(bad, 8),
                                 min(bad, 8) + 1, 'invalid UTF-8 in the input (byte {} of the '
                                 'batch text)'.format(bad))
    d_so, d_dso = punkt.segment(ctx, d_text, d_doc)
    tm('segment')
    out, chunk_off, _, doc_chunk_off = bart.aggregate(ctx, d_text, d_so, d_dso,
                                                      args.target_seq_length)
    tm('aggregate')
    part_chunk_off = doc_chunk_off[torch.from_numpy(part_doc_off).to(dev)]
    res = out.cpu().numpy(), chunk_off.cpu().numpy(), part_chunk_off.cpu().numpy()
    tm('d2h')
    return res


_MAX_ARROW_STRING = (1 << 31) - 1  # bytes one Arrow `string` array can hold (int32 offsets)


def string_column(data, off, r0, r1, limit=_MAX_ARROW_STRING):
    """Rows [r0, r1) of the ragged strings (data, off) as an Arrow chunked `string` array over
    the buffers (no per-row work): one chunk unless the rows hold more than `limit` bytes."""
    import pyarrow as pa
    chunks = []
    a = r0
    while a < r1:
        # the most rows from a whose bytes fit one array (at least one)
        z = int(np.searchsorted(off[a:r1 + 1], off[a] + limit, side='right')) - 1 + a
        z = min(max(z, a + 1), r1)
        b0, b1 = int(off[a]), int(off[z])
        if b1 - b0 > _MAX_ARROW_STRING:
            raise ValueError('one chunk string of {} bytes does not fit an Arrow string '
                             'array'.format(b1 - b0))
        rel = (off[a:z + 1] - b0).astype(np.int32)
        chunks.append(pa.Array.from_buffers(pa.string(), z - a, [None, pa.py_buffer(rel),
                                                                 pa.py_buffer(data[b0:b1])]))
        a = z
    return pa.chunked_array(chunks, type=pa.string())


def schema():
    import pyarrow as pa
    return pa.schema([('sentences', pa.string())])  # pretrain.py:138-146


def write_parquet_part(path, data, off, r0, r1):
    import pyarrow as pa
    import pyarrow.parquet as pq
    from ... import output
    t = pa.Table.from_arrays([string_column(data, off, r0, r1)], schema=schema())
    pq.write_table(t, path, compression=output.DEFAULT_COMPRESSION)
    return path


def write_txt_part(path, data, off, r0, r1):
    """dask.bag.to_textfiles: one element per line, no newline after the last one."""
    b0, b1 = int(off[r0]), int(off[r1])
    if r1 - r0 <= 1:
        body = data[b0:b1].tobytes()
    else:  # a '\n' between the rows: every row moves right by its index
        n = r1 - r0
        o = off[r0:r1 + 1] - b0
        buf = np.empty(b1 - b0 + n - 1, np.uint8)
        dst = np.arange(b1 - b0, dtype=np.int64) + np.repeat(np.arange(n, dtype=np.int64),
                                                             np.diff(o))
        buf[dst] = data[b0:b1]
        buf[o[1:-1] + np.arange(n - 1, dtype=np.int64)] = 0x0A
        body = buf.tobytes()
    with open(path, 'wb') as f:
        f.write(body)
    return path


class _StageTimer:
    """Cumulative host wall time per stage (the GPU stages end in a synchronising copy)."""

    def __init__(self):
        self.t, self.acc = time.perf_counter(), {}

    def __call__(self, name):
        now = time.perf_counter()
        self.acc[name] = self.acc.get(name, 0.0) + now - self.t
        self.t = now


# per-stage seconds of the last main() (tools/bart_bench.py, LDDL_PROFILE_STAGES=1 prints them)
last_stage_seconds = {}


def main(args):
    if args.output_format not in ('parquet', 'txt'):
        raise ValueError('Format {} not supported!'.format(args.output_format))
    tic = time.perf_counter()
    outdir = expand_outdir_and_mkdir(args.sink)
    blocks = plan_partitions(args)
    n_part = len(blocks)
    from concurrent.futures import ThreadPoolExecutor
    rpool = ThreadPoolExecutor(max_workers=max(1, args.read_threads))
    wpool = ThreadPoolExecutor(max_workers=max(1, args.write_threads))
    batches = prefetch(iter_batches(args, blocks, rpool))  # reads while the device is set up
    from ... import punkt
    from ...context import Context
    # (the context carries the tokenizer tables of the BERT path; BART uses its Punkt tables only)
    ctx = Context(os.path.join(ASSETS, 'vocab_synth_uncased_30522.txt'))
    punkt.set_params(ctx, punkt_params(args))
    name = pad_name(n_part)
    timer = _StageTimer()
    inflight = []  # write futures per batch: at most two batches of chunks in host memory
    n_files = 0
    try:
        for parts, text, doc_off, part_doc_off in batches:
            timer('read')
            data, off, pco = batch_chunks(ctx, args, text, doc_off, part_doc_off, timer)
            futs = []
            for i, p in enumerate(parts):
                r0, r1 = int(pco[i]), int(pco[i + 1])
                if args.output_format == 'parquet':
                    fn = os.path.join(outdir, 'part.{}.parquet'.format(p))
                    futs.append(wpool.submit(write_parquet_part, fn, data, off, r0, r1))
                else:
                    fn = os.path.join(outdir, '{}.txt'.format(name(p)))
                    futs.append(wpool.submit(write_txt_part, fn, data, off, r0, r1))
            inflight.append(futs)
            while len(inflight) > 2:
                n_files += len([f.result() for f in inflight.pop(0)])
            timer('write_wait')
        for futs in inflight:
            n_files += len([f.result() for f in futs])
        timer('write_wait')
    finally:
        rpool.shutdown()
        wpool.shutdown()
    if args.output_format == 'parquet':
        from ... import output
        output.write_dataset_metadata(outdir, n_part)
        timer('metadata')
    ctx.close()
    last_stage_seconds.clear()
    last_stage_seconds.update(timer.acc)
    print('Running the dask pipeline took {} s'.format(time.perf_counter() - tic))
    if os.environ.get('LDDL_PROFILE_STAGES'):
        print('stage seconds: ' + json.dumps({k: round(v, 3) for k, v in timer.acc.items()}))
    return n_files


def attach_args(parser=None):
    parser = parser or argparse.ArgumentParser(
        'LDDL preprocessor for the BART pretraining task (MI355X data plane): text shards under '
        "'source' directories -> parquet or txt shards of sentence chunks under --sink.")
    parser.add_argument('--schedule', type=str, default='mpi', choices=['mpi', 'local'],
                        help='accepted for compatibility (one process, one GPU). Default: mpi')
    parser.add_argument('--local-n-workers', type=int, default=os.cpu_count(),
                        help='accepted for compatibility. Default: the number of CPUs')
    parser.add_argument('--local-threads-per-worker', type=int, default=1,
                        help='accepted for compatibility. Default: 1')
    parser.add_argument('--wikipedia', type=str, default=None,
                        help='path to the Wikipedia corpus')
    parser.add_argument('--books', type=str, default=None,
                        help='path to the Toronto books corpus')
    parser.add_argument('--common-crawl', type=str, default=None,
                        help='path to the Common Crawl news corpus')
    parser.add_argument('--open-webtext', type=str, default=None,
                        help='path to the Open WebText Corpus')
    parser.add_argument('--sink', type=str, default=None, required=True,
                        help='path to the dir to store output files')
    parser.add_argument('--output-format', type=str, default='parquet',
                        choices=['parquet', 'txt'], help='output file format. Default: parquet')
    parser.add_argument('--wikipedia-lang', type=str, default='en', choices=['en', 'zh'],
                        help='wikipedia language type. Default: en')
    parser.add_argument('--target-seq-length', type=int, default=128,
                        help='a chunk is closed once it has this many words minus 3 '
                             '([CLS], [SEP], [SEP]). Default: 128')
    parser.add_argument('--short-seq-prob', type=float, default=0.1,
                        help='accepted and unused, as in the reference. Default: 0.1')
    parser.add_argument('--block-size', type=functools.partial(parse_str_of_num_bytes,
                                                               return_str=False),
                        default=None, metavar='n[KMG]',
                        help='bytes per input block (= partition = output shard)')
    parser.add_argument('--num-blocks', type=int, default=None,
                        help='number of input blocks (alternative to --block-size)')
    parser.add_argument('--gpu-batch-bytes', type=int, default=512 << 20,
                        help='lddl_amd: input text bytes per GPU batch of whole partitions '
                             '(bounds HBM use; does not change the output). Default: 512 MiB')
    parser.add_argument('--read-threads', type=int, default=min(os.cpu_count() or 1, 16),
                        help='lddl_amd: host threads that read the blocks. Default: '
                             'min(cpus, 16)')
    parser.add_argument('--write-threads', type=int, default=min(os.cpu_count() or 1, 16),
                        help='lddl_amd: files written concurrently (threads). Default: '
                             'min(cpus, 16)')
    parser.add_argument('--punkt-params', type=str, default=None,
                        help='JSON PunktParameters (abbrev_types, collocations, sent_starters, '
                             'ortho_context); default: nltk English model if loadable, else '
                             'untrained')
    return parser


def console_script():
    main(attach_args().parse_args())


if __name__ == '__main__':
    sys.exit(0 if console_script() is None else 0)
