"""Rendered batches of `preprocess_bert_pretrain` from the GPU to files: the device-to-host copy
(whole or in partition groups of `_D2H_CHUNK_BYTES`), the part-file and txt writers
(`process_batch`, `write_txt`), the balanced-shard writer (`ShardWriters`) and the one rule for
how many rendered batches may wait for their writes (`InflightWindow`)."""
import contextlib
import os

from .gpu_batch import _copy_stream, make_batch_pairs, render_batch
from .trace import trace as _trace

# rendered batches leave the GPU in partition groups of about this many MiB of strings (0: the
# whole batch in one pinned allocation per column, the round-4 behaviour)
_D2H_CHUNK_BYTES = int(os.environ.get('LDDL_D2H_CHUNK_MB', '128')) << 20


class InflightWindow:
    """FIFO of the rendered batches whose writes have not finished: entries (job, writes, nbytes)
    with `job` None, the list of a batch's paths or a future (of the paths, or of None) and
    `writes` the batch's write futures; `nbytes` are the pinned host bytes the batch holds until
    they finish. trim() waits for the oldest entries while more than `max_batches` are held, or
    more than one and more than `max_bytes` in all (the newest batch always proceeds). n_files
    counts the paths of the jobs. With a `lock` (several pushing threads) entries are popped
    under it and waited for outside it, so the other threads keep going."""

    def __init__(self, max_batches, max_bytes, lock=None):
        self.max_batches, self.max_bytes = max_batches, max_bytes
        self.lock = lock if lock is not None else contextlib.nullcontext()
        self.entries, self.n_files = [], 0

    def __len__(self):
        return len(self.entries)

    def push(self, job, writes, nbytes):
        with self.lock:
            if isinstance(job, list):
                self.n_files += len(job)
            self.entries.append((job, writes, nbytes))

    def trim(self, incoming=None):
        """Retire the oldest entries until the window, plus one more entry of `incoming` bytes
        when given (trimming before a push), is within its bounds."""
        more = 0 if incoming is None else 1
        self._retire(lambda n, nb: n + more > self.max_batches or (
            n + more > 1 and nb + (incoming or 0) > self.max_bytes))

    def drain(self):
        self._retire(lambda n, nb: n > 0)

    def _retire(self, over):
        while True:
            with self.lock:
                if not over(len(self.entries), sum(nb for _, _, nb in self.entries)):
                    return
                job, writes, _ = self.entries.pop(0)
            if job is not None and not isinstance(job, list):
                paths = job.result()
                if isinstance(paths, list):
                    with self.lock:
                        self.n_files += len(paths)
            for f in writes:
                f.result()


def process_batch(ctx, args, partitions, corpus, outdir, timer=None, executor=None, futures=None,
                  copier=None):
    """Run the GPU hot path over a group of partitions and write their files (concurrently on
    `executor` when given: the futures go to `futures`). With a `copier` (one host thread), the
    rendered columns are copied to the host and handed to the writers there, so this batch's
    copy and writes overlap the next batch's GPU work; the returned future yields the paths."""
    from ... import output
    tm = timer or (lambda name: None)
    index = [p for p, _ in partitions]
    _trace('gpu_start', index[0])
    pb = make_batch_pairs(ctx, args, partitions, corpus, timer)
    part_rows = pb.part_off.cpu().numpy()
    drd, nbins, counts = render_batch(ctx, args, pb)
    if counts is not None:
        counts = counts.cpu().numpy()
    del pb
    tm('render')

    _trace('render_device', index[0])

    def finish(stream=None):
        _trace('d2h_start', index[0])
        chunk = _D2H_CHUNK_BYTES
        if args.output_format == 'parquet' and chunk > 0:
            # string columns in partition groups of ~chunk bytes, each handed to the writers as
            # it lands (output.DeviceRendered.to_host_chunks)
            paths = []
            for p0, p1, rd in drd.to_host_chunks(part_rows, chunk, stream):
                paths += output.write_parquet(outdir, rd, part_rows[p0:p1 + 1], index[p0:p1],
                                              args.masking, nbins,
                                              None if counts is None else counts[p0:p1],
                                              executor=executor, futures=futures)
            _trace('d2h_end', index[0])
            return paths
        rd = drd.to_host(stream)
        _trace('d2h_end', index[0])
        if args.output_format == 'parquet':
            return output.write_parquet(outdir, rd, part_rows, index, args.masking, nbins,
                                        counts, executor=executor, futures=futures)
        return write_txt(outdir, rd, part_rows, index, args.masking, nbins, counts,
                         getattr(args, 'n_partitions', len(part_rows) - 1))
    if copier is not None and args.output_format == 'parquet':
        fut = copier.submit(finish, _copy_stream(ctx))
        fut.render_bytes = drd.nbytes  # pinned host bytes until the batch is written
        return fut
    paths = finish()
    tm('write')
    return paths


def _row_order(ranges):
    """The sharded writer's (shard, bin, r0, r1) row ranges in row order (the balanced table is
    bin-major, `ranges` shard-major), the chunk bounds over them and whether they tile the rows
    contiguously (then the copy leaves the GPU in groups of them, as process_batch does). Empty
    ranges sort before the non-empty range that starts at the same row (key (r0, r1)); sorting on
    r0 alone put an empty (R, R) after (R, R + k) and the check failed for any batch in which a
    shard received no rows of a bin."""
    srt = sorted(ranges, key=lambda x: (x[2], x[3]))
    bounds = [srt[0][2]] + [x[3] for x in srt] if srt else [0]
    return srt, bounds, all(srt[i][2] == bounds[i] for i in range(len(srt)))


def _txt_line(row, masking):
    """pretrain.py:508-527 line format."""
    from ...utils import deserialize_np_array
    if masking:
        return ('is_random_next: {} - [CLS] {} [SEP] {} [SEP] - masked_lm_positions: {} - '
                'masked_lm_labels: {} - {}').format(row['is_random_next'], row['A'], row['B'],
                                                    deserialize_np_array(
                                                        row['masked_lm_positions']),
                                                    row['masked_lm_labels'], row['num_tokens'])
    return 'is_random_next: {} - [CLS] {} [SEP] {} [SEP] - {}'.format(
        row['is_random_next'], row['A'], row['B'], row['num_tokens'])


def pad_name(n):
    """fsspec build_name_function(n - 1) (dask to_textfiles' default names): zero-padded to the
    width of the largest partition index."""
    import math
    w = int(math.ceil(math.log10(max(n - 1, 0) + 1e-8)))
    return lambda i: str(i).zfill(w)


def write_txt(outdir, rd, part_rows, index, masking, nbins, counts, n_part):
    """Debug output (`--output-format txt`, pretrain.py:501-531): dask's to_textfiles writes
    partition i to `<i>.txt` (i zero-padded to the width of n_part - 1); the binned writer
    (binning.py:439-509) names (i, b) `<i>_<b>.txt` and creates every bin's file. Lines are
    joined by '\n' without a trailing newline (last_endline=False)."""
    name = pad_name(n_part)
    paths = []
    for p in range(len(part_rows) - 1):
        r0, r1 = int(part_rows[p]), int(part_rows[p + 1])
        spans = [(None, r0, r1)] if nbins is None else []
        if nbins is not None:
            b0 = r0
            for b in range(nbins):
                spans.append((b, b0, b0 + int(counts[p, b])))
                b0 += int(counts[p, b])
        for b, a, z in spans:
            fn = os.path.join(outdir, '{}.txt'.format(name(index[p])) if b is None else
                              '{}_{}.txt'.format(index[p], b))
            with open(fn, 'w') as f:
                f.write('\n'.join(_txt_line(rd.row(r), masking) for r in range(a, z)))
            paths.append(fn)
    return paths


def _open_file_budget(needed, headroom=256):
    """Raise this process's soft RLIMIT_NOFILE so that `needed` parquet writers can stay open
    (plus headroom for pyarrow, sockets and libraries); False if the hard limit is too low."""
    import resource
    soft, hard = resource.getrlimit(resource.RLIMIT_NOFILE)
    want = needed + headroom
    if soft == resource.RLIM_INFINITY or want <= soft:
        return True
    if hard != resource.RLIM_INFINITY and want > hard:
        return False
    try:
        resource.setrlimit(resource.RLIMIT_NOFILE, (want, hard))
    except (ValueError, OSError):
        return False
    return True


class ShardWriters:
    """This rank's balanced shards, written as the batches stream through: one parquet file per
    (shard, bin) named like the load balancer's (`shard-<k>.parquet_<b>`, or `shard-<k>.parquet`
    unbinned, load_balance.py:90-92), one row group per batch in batch order. Each batch's
    writes run on the thread pool while the next batch is on the GPU; a writer is never
    appended from two threads (a batch's writes finish before the next batch's start).

    Every (shard, bin) file stays open until close() (the reference example's 4096 shards x 8
    bins are 32,768 files on one rank): the soft RLIMIT_NOFILE is raised for them. When the hard
    limit (or `max_open`) cannot hold them all, each batch's row group is written to a piece file
    and closed at once, and close() appends the pieces of each shard, in batch order, into its
    file (the same files, one more pass over the data)."""

    def __init__(self, outdir, nbins, binned, masking, pool, n_local_shards=None, max_open=None,
                 max_inflight_bytes=8 << 30):
        self.outdir, self.nbins, self.binned, self.masking, self.pool = (outdir, nbins, binned,
                                                                         masking, pool)
        # (copy job, write futures, pinned bytes) of the rendered batches not yet written
        self.window = InflightWindow(2, max_inflight_bytes)
        self.writers, self.pending, self.shards = {}, [], set()
        self.last_chunked = None  # the last batch left the GPU in row-range groups (tests)
        needed = (n_local_shards or 0) * nbins
        self.pieces = None  # {(shard, bin): [piece paths]} in piece mode
        if (max_open is not None and needed > max_open) or not _open_file_budget(needed):
            self.pieces = {}
            self.piece_dir = os.path.join(outdir, '.lddl_amd_pieces.{}'.format(os.getpid()))
            os.makedirs(self.piece_dir, exist_ok=True)

    def name(self, s, b):
        return os.path.join(self.outdir, 'shard-{}.parquet{}'.format(
            s, '_{}'.format(b) if self.binned else ''))

    def _append(self, key, rd, r0, r1):
        from ... import output
        self._write(key, output.table(rd, r0, r1, self.masking, self.binned))

    def _write(self, key, t):
        import pyarrow.parquet as pq
        from ... import output
        if self.pieces is not None:
            lst = self.pieces.setdefault(key, [])
            fn = os.path.join(self.piece_dir, '{}_{}.{}'.format(key[0], key[1], len(lst)))
            pq.write_table(t, fn, compression=output.DEFAULT_COMPRESSION)
            lst.append(fn)
            return
        w = self.writers.get(key)
        if w is None:
            w = self.writers[key] = pq.ParquetWriter(self.name(*key), t.schema,
                                                     compression=output.DEFAULT_COMPRESSION)
        w.write_table(t)

    def _merge(self, key):
        """Piece mode: the pieces of one (shard, bin), row group by row group, into its file."""
        import pyarrow.parquet as pq
        from ... import output
        w = None
        for fn in self.pieces.pop(key):
            pf = pq.ParquetFile(fn)
            for g in range(pf.num_row_groups):
                t = pf.read_row_group(g)
                if w is None:
                    w = pq.ParquetWriter(self.name(*key), t.schema,
                                         compression=output.DEFAULT_COMPRESSION)
                w.write_table(t)
            os.remove(fn)
        if w is not None:
            w.close()

    def add(self, ctx, bb, copier=None):
        """Render this batch's rows of the rank's shards (GPU) and queue their writes. With a
        `copier` thread, the host copy and the queueing run there (in batch order: a batch's
        appends are queued after the previous batch's have finished), overlapping the next
        batch's GPU work."""
        from ... import output
        self.shards.update(bb.shards)
        if bb.n_rows == 0:
            return
        drd = output.render_device(ctx, bb.table, bb.rows, bb.bin_ids() if self.binned else None)
        ranges = [(s, b) + tuple(bb.shard_range(m, b)) for m, s in enumerate(bb.shards)
                  for b in range(self.nbins)]

        writes = []  # this batch's write futures: its pinned copy lives until they finish
        srt, bounds, contiguous = _row_order(ranges)
        chunked = _D2H_CHUNK_BYTES > 0 and contiguous
        self.last_chunked = chunked

        def job(stream=None):
            if chunked:
                first = True
                for p0, p1, rd in drd.to_host_chunks(bounds, _D2H_CHUNK_BYTES, stream):
                    if first:  # appends stay in batch order per (shard, bin) writer
                        for f in self.pending:
                            f.result()
                        self.pending, first = [], False
                    new = [self.pool.submit(self._append, (s, b), rd, r0, r1)
                           for s, b, r0, r1 in srt[p0:p1] if r1 > r0]
                    self.pending += new
                    writes.extend(new)
                return
            rd = drd.to_host(stream)
            for f in self.pending:
                f.result()
            self.pending = [self.pool.submit(self._append, (s, b), rd, r0, r1)
                            for s, b, r0, r1 in ranges if r1 > r0]
            writes.extend(self.pending)
        if copier is None:
            job()
            return
        nb = drd.nbytes
        # a batch's bytes count until its WRITES have finished (not only its copy job), so the
        # pinned host copies held at once stay within max_inflight_bytes plus the newest batch:
        # the window is trimmed for this batch before its copy job is submitted
        self.window.trim(incoming=nb)
        self.window.push(copier.submit(job, _copy_stream(ctx)), writes, nb)

    def close(self):
        """Finish the writes; shards of a bin that received no rows get an empty file (every bin
        has all shards, as the loader requires)."""
        import pyarrow.parquet as pq
        from ... import output
        self.window.drain()
        for f in self.pending:
            f.result()
        self.pending = []
        merged = set()
        if self.pieces is not None:  # one writer open per pool thread at a time
            merged = set(self.pieces)
            for f in [self.pool.submit(self._merge, k) for k in list(self.pieces)]:
                f.result()
            os.rmdir(self.piece_dir)
        paths, done = [], []
        empty = output.schema(self.masking, self.binned).empty_table()
        for s in sorted(self.shards):
            for b in range(self.nbins):
                w = self.writers.pop((s, b), None)
                if w is not None:  # footers written on the pool (one writer per task)
                    done.append(self.pool.submit(w.close))
                elif (s, b) not in merged:  # (merged: written from its pieces above)
                    done.append(self.pool.submit(pq.write_table, empty, self.name(s, b),
                                                 compression=output.DEFAULT_COMPRESSION))
                paths.append(self.name(s, b))
        for f in done:
            f.result()
        return paths


def num_samples_of_shards(shard_counts, binned):
    """`.num_samples.json` content of the balanced layout (load_balance.py:372-378) from the
    int64[S, B] shard counts."""
    out = {}
    S, B = shard_counts.shape
    for b in range(B):
        for s in range(S):
            out['shard-{}.parquet{}'.format(s, '_{}'.format(b) if binned else '')] = int(
                shard_counts[s, b])
    return out


def _default_inflight_bytes():
    """1/8 of the host's memory, clamped to 2-16 GiB."""
    try:
        total = os.sysconf('SC_PAGE_SIZE') * os.sysconf('SC_PHYS_PAGES')
    except (ValueError, OSError):
        total = 64 << 30
    return int(max(2 << 30, min(16 << 30, total // 8)))


def _warm_parquet_writer(outdir):
    import pyarrow as pa
    import pyarrow.parquet as pq
    fn = os.path.join(outdir, '.lddl_amd_warmup.{}.parquet'.format(os.getpid()))
    try:
        pq.write_table(pa.table({'A': pa.array(['x'])}), fn)
    finally:
        if os.path.exists(fn):
            os.remove(fn)
