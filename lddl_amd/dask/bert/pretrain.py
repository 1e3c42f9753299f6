"""`preprocess_bert_pretrain` — drop-in for the reference's `lddl.dask.bert.pretrain`
(lddl/dask/bert/pretrain.py:563-884): same flags, same output layout, GPU data plane.

Pipeline (reference call stack in SURVEY.md §3.1):
  read `*.txt` sources into blocks (readers.py)            -> lddl_amd.dask.readers (host; each
                                                              rank reads only its own blocks)
  random shuffle of documents over partitions (100-111)    -> seeded shuffle of the documents of
                                                              each shuffle group of partitions
                                                              (host; the reference's is global
                                                              and unseeded)
  split_id_text (readers.py:131-136)                       -> host, per line
  sent_tokenize + strip + drop empty (86-88)               -> lddl_segment_* (HIP Punkt; nltk on
                                                              the host with --sentence-splitter host)
  tokenizer.tokenize(s, max_length=512, truncation=True)   -> lddl_tokenize (HIP)
  _to_partition_pairs / create_pairs_from_document /
    create_masked_lm_predictions (386-402, 241-365, 182-238) -> lddl_pairs_plan / emit (HIP)
  _to_dataframe_binned (binning.py:63-93)                  -> lddl_bin_partitions (HIP)
  instance dict + serialize_np_array (345-358)             -> lddl_render_* (HIP)
  to_parquet / write_partition_binned + _metadata          -> pyarrow writer (host)

Random state: the reference draws from each Dask worker's unseeded global `random` (H1). Here
partition p is processed as if `random.seed(partition_seed(--seed, p))` had been called before
its `_to_partition_pairs`, which the test-suite replays bit for bit on the CPU.

Multi-GPU (`--schedule mpi`, launched with torchrun, one process per GPU): rank r owns the
partitions p with p % world_size == r (partitions are independent) and reads only
those blocks.

`--num-shards S` (lddl_amd; the reference runs `balance_dask_output` as a second job over the
files) writes the balancer's layout directly: `shard-<k>.parquet_<b>` (or `shard-<k>.parquet`
unbinned) with N or N+1 samples per bin, plus `.num_samples.json` (lddl/dask/load_balance.py:
90-92, 372-378) — what get_bert_pretrain_data_loader consumes. `--balance-plan stream` (default)
balances every GPU batch in HBM as it is produced (lddl_amd/balance.py: RCCL all-gather of the
batch's per-bin counts, per-rank shard quotas, all-to-all-v of only each bin's surplus rows over
a rank's quota), so HBM holds one batch at any corpus size and each shard file grows
by one row group per batch; `--balance-plan reference` writes the part files and runs the
drop-in balance_dask_output over them (the reference's exact shard contents).
"""
import argparse
import functools
import json
import os
import threading
import time

from ...utils import attach_bool_arg, expand_outdir_and_mkdir, parse_str_of_num_bytes
# (get_partitions, build_doc_corpus, partition_seed, rank_batches, write_txt and _txt_line are
# re-exported for the tests; writers._D2H_CHUNK_BYTES and writers._row_order are read there at
# call time and are deliberately NOT: a patch of a copy here would change nothing)
from .corpus import (ASSETS, build_corpus, build_doc_corpus, get_partitions,  # noqa: F401
                     iter_batches, iter_doc_batches, partition_seed, plan_partitions, prefetch,
                     punkt_params, rank_batches)
from .gpu_batch import _empty_pairs, _warm_gpu_path, make_batch_pairs
from .trace import trace as _trace
from .writers import (InflightWindow, ShardWriters, _default_inflight_bytes,  # noqa: F401
                      _txt_line, _warm_parquet_writer, num_samples_of_shards, process_batch,
                      write_txt)


def _resolve_vocab(vocab_file):
    if os.path.isfile(vocab_file):
        return vocab_file
    raise FileNotFoundError(
        '--vocab-file {!r} is not a file. The reference falls back to '
        'BertTokenizerFast.from_pretrained (a network download); lddl_amd runs offline and needs '
        'a vocab.txt path (e.g. {}/vocab_synth_uncased_30522.txt)'.format(vocab_file, ASSETS))


def _any_rank(flag, device):
    """True when `flag` holds on any rank (all-reduce MAX: RCCL on a device tensor, gloo on the
    host)."""
    import torch
    import torch.distributed as dist
    dev = device if dist.get_backend() == 'nccl' else 'cpu'
    t = torch.tensor([1 if flag else 0], dtype=torch.int32, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return bool(t.item())


class _StageTimer:
    """Cumulative wall time per stage (device-synchronised), printed at the end of main."""

    def __init__(self, enabled):
        self.enabled, self.t, self.acc = enabled, None, {}

    def __call__(self, name):
        if not self.enabled:
            return
        import torch
        torch.cuda.current_stream().synchronize()  # (not the copy stream: it overlaps)
        now = time.perf_counter()
        if self.t is not None:
            self.acc[name] = self.acc.get(name, 0.0) + now - self.t
        self.t = now

    def mark(self):
        if self.enabled:
            self.t = time.perf_counter()


def _run_gpu_workers(args, n_workers, vocab, ctx0, batch_it, outdir, pool, copier, inflight,
                     timer=None):
    """The non-balanced batch loop over `n_workers` GPU worker threads (main's --gpu-workers).
    Worker 0 uses the main Context; the others create their own (a Context holds per-call state:
    the segmenter's count / fill pair). `inflight` is main's InflightWindow (n_workers + 1
    batches, with a lock): it counts the files written and is left empty."""
    import torch
    from ...context import Context
    lock = threading.Lock()  # the batch iterator's
    errors = []

    def worker(k):
        try:
            wctx = ctx0
            if k > 0:
                wctx = Context(vocab, do_lower_case=True, device=ctx0.device.index)
                if args.sentence_splitter == 'gpu':
                    from ... import punkt
                    punkt.set_params(wctx, getattr(ctx0, '_punkt_params', None))
            st = torch.cuda.Stream(device=wctx.device)
            wt = _StageTimer(args.profile_stages)  # this worker's stages (its own stream)
            timers.append(wt)
            with torch.cuda.device(wctx.device), torch.cuda.stream(st):
                while not errors:
                    with lock:
                        item = next(batch_it, None)
                    if item is None:
                        return
                    batch, corpus = item
                    _trace('batch_ready', batch[0][0] if batch else -1)
                    futs = []
                    wt.mark()
                    job = process_batch(wctx, args, batch, corpus, outdir, wt, pool, futs, copier)
                    inflight.push(job, futs, getattr(job, 'render_bytes', 0))
                    inflight.trim()
                st.synchronize()
        except BaseException as e:  # noqa: B902 - re-raised by the caller
            errors.append(e)

    timers = []
    threads = [threading.Thread(target=worker, args=(k,), name='gpu-worker-{}'.format(k))
               for k in range(n_workers)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    inflight.drain()
    if timer is not None and timer.enabled:  # per-stage seconds summed over the workers
        for wt in timers:
            for k, v in wt.acc.items():
                timer.acc[k] = timer.acc.get(k, 0.0) + v
        timer.acc['gpu_workers'] = n_workers


def main(args):
    if args.bin_size is not None:
        if args.bin_size > args.target_seq_length:
            raise ValueError('Please provide a bin size that is <= target-seq-length')
        if args.target_seq_length % args.bin_size != 0:
            raise ValueError('Please provide a bin size that can divide the target '
                             'sequence length.')
    if args.output_format not in ('parquet', 'txt'):
        raise ValueError('Format {} not supported!'.format(args.output_format))
    if args.num_shards is not None and args.output_format != 'parquet':
        raise ValueError('--num-shards writes balanced parquet shards only')
    if args.num_shards is not None and args.num_shards < 1:
        raise ValueError('--num-shards must be >= 1')
    if getattr(args, 'whole_word_masking', False) and not (
            args.masking and getattr(args, 'rng', 'replay') == 'native'):
        raise ValueError('--whole-word-masking needs --masking and --rng native (replay '
                         'reproduces the reference, which has no whole-word masking; without '
                         '--masking the loaders mask: whole_word_masking=True there)')
    world =int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    vocab = _resolve_vocab(args.vocab_file)
    tic = time.perf_counter()
    _trace('main', -1)
    outdir = expand_outdir_and_mkdir(args.sink)
    blocks = plan_partitions(args)
    args.n_partitions = len(blocks)
    _trace('planned', -1)
    if args.sentence_splitter == 'host':
        # host segmentation first: its process pool forks before this process touches the GPU
        batches = [(b, ('sentences',) + build_corpus(b, args.local_n_workers))
                   for b in iter_batches(args, rank, world, blocks)]
    else:
        # the host reader starts now, in its own thread, overlapping the device setup below
        batches = prefetch(iter_doc_batches(args, rank, world, blocks))
    from concurrent.futures import ThreadPoolExecutor
    pool = ThreadPoolExecutor(max_workers=max(1, args.write_threads))
    # pyarrow's parquet writer initialises lazily on its first file (~0.3-0.8 s, measured on the
    # box): one tiny write on a writer thread now overlaps that with the setup and the first batch
    pool.submit(_warm_parquet_writer, outdir)
    _trace('setup_start', -1)
    import torch
    import torch.distributed as dist
    if world > 1:
        if os.environ.get('LDDL_SHARE_DEVICE') == '1':
            # every rank on device 0, gloo collectives staged through host memory: a rehearsal
            # of the multi-rank path on a one-GPU machine (never how a node is run)
            torch.cuda.set_device(0)
            if not dist.is_initialized():
                dist.init_process_group('gloo')
        else:
            torch.cuda.set_device(local)
            if not dist.is_initialized():
                dist.init_process_group('nccl', device_id=torch.device('cuda', local))
    from ...context import Context
    ctx = Context(vocab, do_lower_case=True)  # BertTokenizerFast default, SURVEY H5
    if args.sentence_splitter == 'gpu':
        from ... import punkt
        punkt.set_params(ctx, punkt_params(args))
    # (only when the read outlasts the setup: with less than one GPU batch of input per rank the
    # warm-up would sit on the critical path; 1 GB seq 128: segment 0.06-0.09 -> 0.035 s, the run
    # 1.36-1.47 -> 1.26-1.39 s on one box, profiles/r05s_*)
    warm = os.environ.get('LDDL_CLI_WARMUP', '1') != '0' and \
        sum(b.nbytes for b in blocks) >= world * args.gpu_batch_bytes
    if args.sentence_splitter == 'gpu' and warm:
        _warm_gpu_path(ctx, args)
    timer = _StageTimer(args.profile_stages)
    _trace('setup_end', -1)
    timer.mark()
    stream = writers = None
    if args.num_shards is not None and args.balance_plan == 'stream':
        from ...balance import StreamBalancer
        binned = args.bin_size is not None
        bin_size = args.bin_size if binned else args.target_seq_length
        nbins = args.target_seq_length // bin_size
        stream = StreamBalancer(ctx, bin_size, nbins, num_shards=args.num_shards)
        from ...balance import shard_owner
        writers = ShardWriters(outdir, nbins, binned, args.masking, pool,
                               n_local_shards=int((shard_owner(args.num_shards, world) == rank).sum()),
                               max_open=args.max_open_files,
                               max_inflight_bytes=args.max_inflight_render_bytes)
    copier = ThreadPoolExecutor(max_workers=1)  # device -> host copies of rendered batches
    batch_it = iter(batches)
    gpu_workers = max(1, int(getattr(args, 'gpu_workers', 1) or 1))
    multi = stream is None and gpu_workers > 1
    # the batches not yet written: at most two rendered batches in host memory (one more than
    # the GPU workers when there are several), and no more pinned bytes than
    # --max-inflight-render-bytes (the newest batch always proceeds)
    inflight = InflightWindow(gpu_workers + 1 if multi else 2, args.max_inflight_render_bytes,
                              threading.Lock() if multi else None)
    if multi:
        # Several GPU batches in flight: a batch's replay planner is one sequential chain per
        # partition (~0.1 s for a 1 MiB partition whatever the batch size), so one batch of a few
        # hundred partitions leaves the GPU mostly idle while it runs. Each worker thread owns a
        # Context and a stream, takes the next batch from the reader and runs it through the
        # whole GPU path; batches are independent (files are named by partition), so they may
        # finish in any order.
        _run_gpu_workers(args, gpu_workers, vocab, ctx, batch_it, outdir, pool, copier, inflight,
                         timer)
        timer.mark()
        batch_it = iter(())
    while True:
        item = next(batch_it, None)
        if stream is not None and world > 1:
            # every rank steps the balancer until no rank has a batch left: the loop ends on the
            # iterators themselves (one tiny all-reduce per step), never on a separate count
            if not _any_rank(item is not None, ctx.device):
                break
            if item is None:  # this rank is out of batches: it still takes part in the exchange
                writers.add(ctx, stream.step(_empty_pairs(ctx, args.masking)), copier)
                continue
        elif item is None:
            break
        batch, corpus = item
        timer('read')
        _trace('batch_ready', batch[0][0] if batch else -1)
        if stream is None:
            futs = []
            job = process_batch(ctx, args, batch, corpus, outdir, timer, pool, futs, copier)
            # (a plain list of paths, txt output or no copier, holds no pinned bytes)
            inflight.push(job, futs, getattr(job, 'render_bytes', 0))
            inflight.trim()
            timer('write_wait')
        else:
            bb = stream.step(make_batch_pairs(ctx, args, batch, corpus, timer))
            timer('balance')
            writers.add(ctx, bb, copier)
            del bb
            timer('render')
        timer.mark()
    inflight.drain()
    n_files = inflight.n_files
    timer('write_wait')
    if stream is not None:
        n_files += len(writers.close())
        timer('write_wait')
        if rank == 0:
            with open(os.path.join(outdir, '.num_samples.json'), 'w') as f:
                json.dump(num_samples_of_shards(stream.all_shard_counts, binned), f)
    copier.shutdown()
    pool.shutdown()
    if world > 1:
        dist.barrier()
    if rank == 0 and stream is None and args.output_format == 'parquet':
        from ... import output
        output.write_dataset_metadata(outdir, len(blocks),
                                      None if args.bin_size is None else
                                      args.target_seq_length // args.bin_size)
    if args.num_shards is not None and args.balance_plan == 'reference':
        # the reference's second job over the part files: balance_dask_output in place
        # (load_balance.py:381-418), its exact shard layout, originals deleted
        from .. import load_balance as LB
        if world > 1:
            dist.barrier()
        LB.main(LB.attach_args().parse_args(['--indir', outdir, '--num-shards',
                                             str(args.num_shards)]))
    if rank == 0:
        print('Running the dask pipeline took {} s'.format(time.perf_counter() - tic))
        if args.profile_stages:
            print('stage seconds (rank 0{}): '.format(
                ', summed over {} GPU workers'.format(timer.acc['gpu_workers'])
                if 'gpu_workers' in timer.acc else '') + json.dumps(
                {k: round(v, 3) for k, v in timer.acc.items() if k != 'gpu_workers'}))
            hs = torch.cuda.host_memory_stats()  # torch's pinned host allocator
            print('pinned host memory peak (rank 0): {:.2f} GB'.format(max(
                [v for k, v in hs.items() if 'bytes' in k and k.endswith('peak')] or [0]) / 1e9))
    if world > 1:
        dist.barrier()
    return n_files


def attach_args(parser=None):
    parser = parser or argparse.ArgumentParser(
        'LDDL preprocessor for the BERT pretraining task (MI355X data plane): text shards under '
        "'source' directories -> parquet shards under --sink, input to the load balancer.")
    parser.add_argument('--schedule', type=str, default='mpi', choices=['mpi', 'local'],
                        help='mpi: one process per GPU under torchrun (partitions striped over '
                        'ranks); local: this process only. Default: mpi')
    parser.add_argument('--local-n-workers', type=int, default=min(os.cpu_count() or 1, 16),
                        help='host processes for sentence segmentation. Default: min(cpus, 16)')
    parser.add_argument('--local-threads-per-worker', type=int, default=1,
                        help='accepted for compatibility. Default: 1')
    parser.add_argument('--wikipedia', type=str, default=None,
                        help="path to the 'source' subdirectory of the Wikipedia corpus")
    parser.add_argument('--books', type=str, default=None,
                        help="path to the 'source' subdirectory of the books corpus")
    parser.add_argument('--common-crawl', type=str, default=None,
                        help="path to the 'source' subdirectory of the Common Crawl corpus")
    parser.add_argument('--sink', type=str, default=None, required=True,
                        help='output directory (parquet or txt files)')
    parser.add_argument('--output-format', type=str, default='parquet',
                        choices=['parquet', 'txt'], help='Default: parquet')
    parser.add_argument('--wikipedia-lang', type=str, default='en', choices=['en', 'zh'],
                        help='Default: en')
    parser.add_argument('--target-seq-length', type=int, default=128,
                        help='maximum tokens of [CLS] A [SEP] B [SEP]. Default: 128')
    parser.add_argument('--short-seq-prob', type=float, default=0.1,
                        help='probability of a shorter random target length. Default: 0.1')
    parser.add_argument('--block-size', type=functools.partial(parse_str_of_num_bytes,
                                                               return_str=False),
                        default=None, metavar='n[KMG]',
                        help='bytes per input block (= partition = output shard)')
    parser.add_argument('--num-blocks', type=int, default=None,
                        help='number of input blocks (alternative to --block-size)')
    parser.add_argument('--bin-size', type=int, default=None,
                        help='enable sequence binning with this stride of num_tokens')
    parser.add_argument('--sample-ratio', type=float, default=0.9,
                        help='fraction of documents kept. Default: 0.9')
    parser.add_argument('--seed', type=int, default=12345, help='Default: 12345')
    parser.add_argument('--duplicate-factor', type=int, default=5, help='Default: 5')
    parser.add_argument('--vocab-file', type=str, default='bert-large-uncased',
                        help='path to a BERT vocab.txt (offline: no model-name download)')
    attach_bool_arg(parser, 'masking', default=False,
                    help_str='static masking in the preprocessor (default: off = dynamic '
                    'masking in the data loader)')
    parser.add_argument('--masked-lm-ratio', type=float, default=0.15, help='Default: 0.15')
    attach_bool_arg(parser, 'whole-word-masking', default=False,
                    help_str='lddl_amd, with --masking and --rng native: mask whole words '
                    "(Google BERT's do_whole_word_mask); a pair gets at most the per-token "
                    "mode's number of masked positions")
    parser.add_argument('--gpu-batch-bytes', type=int, default=512 << 20,
                        help='lddl_amd: input text bytes per GPU batch of partitions (bounds HBM '
                             'use; consecutive batches overlap their GPU work, rendering and file '
                             'writes; does not change the part.* output). Default: 512 MiB '
                             '(1 GB end to end: 570 MB/s at 256 MiB, 618 at 512 MiB, 468 at 1 GiB)')
    parser.add_argument('--read-threads', type=int, default=min(os.cpu_count() or 1, 16),
                        help='lddl_amd: host threads of the input reader (GPU segmentation path). '
                             'Default: min(cpus, 16)')
    parser.add_argument('--shuffle-group-bytes', type=int, default=1 << 30,
                        help='lddl_amd: documents are shuffled across the partitions of runs of '
                             'this many input bytes (the reference shuffles globally, '
                             'pretrain.py:100-111; INTEGRATION.md)')
    parser.add_argument('--sentence-splitter', choices=['gpu', 'host'], default='gpu',
                        help='gpu: Punkt on the GPU (exact nltk PunktSentenceTokenizer); host: '
                             "nltk's sent_tokenize in host processes (requires nltk)")
    parser.add_argument('--punkt-params', type=str, default=None,
                        help='JSON PunktParameters (abbrev_types, collocations, sent_starters, '
                             'ortho_context); default: nltk English model if loadable, else '
                             'untrained')
    parser.add_argument('--rng', choices=['replay', 'native'], default='replay',
                        help="lddl_amd: 'replay' reproduces CPython random per partition "
                             "(random.seed(partition seed)), bit-exact with the reference; "
                             "'native' draws the same distributions from Philox counter streams "
                             "keyed by --seed (documents and pairs in parallel)")
    parser.add_argument('--num-shards', type=int, default=None,
                        help="lddl_amd: write the load balancer's layout (shard-<k>.parquet[_<b>] "
                             'with N or N+1 samples per bin + .num_samples.json) instead of '
                             'part.* files (see --balance-plan)')
    parser.add_argument('--balance-plan', choices=['stream', 'reference'], default='stream',
                        help="lddl_amd, with --num-shards: 'stream' balances each GPU batch in "
                             "HBM as it is produced (per-rank shard quotas from the all-gathered "
                             "bin counts: only each bin's surplus over a rank's quota crosses "
                             "ranks, and every shard ends each batch with N or N+1 rows per bin; "
                             "one batch resident); 'reference' writes "
                             "the part files and runs balance_dask_output over them, the "
                             "reference's exact shard layout")
    parser.add_argument('--max-inflight-render-bytes', type=int, default=_default_inflight_bytes(),
                        help='pinned host bytes of rendered batches waiting for their parquet '
                             'writes (default: 1/8 of host memory, 2-16 GiB); the GPU waits for '
                             'the writes beyond it; the newest batch always proceeds, so the peak is this '
                             'bound plus one rendered batch')
    parser.add_argument('--max-open-files', type=int, default=None,
                        help='--num-shards: most shard files kept open at once (default: as many '
                             'as RLIMIT_NOFILE allows, raised to its hard limit); above it, each '
                             'batch is written as a piece and the pieces are merged at the end')
    parser.add_argument('--gpu-workers', type=int, default=1,
                        help='lddl_amd: GPU batches processed concurrently, each by a host thread '
                             'with its own stream (without --num-shards; the balanced path keeps '
                             'batch order). Default: 1')
    parser.add_argument('--write-threads', type=int, default=min(os.cpu_count() or 1, 16),
                        help='lddl_amd: parquet files written concurrently (threads). Default: '
                             'min(cpus, 16)')
    attach_bool_arg(parser, 'profile-stages', default=False,
                    help_str='lddl_amd: print device-synchronised seconds per stage (read, h2d, '
                    'segment, tokenize, pairs, render, write, balance)')
    return parser


def console_script():
    main(attach_args().parse_args())


if __name__ == '__main__':
    console_script()
