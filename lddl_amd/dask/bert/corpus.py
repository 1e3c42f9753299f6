"""Host input of `preprocess_bert_pretrain` (no GPU): partition planning, the per-group document
shuffle, reading GPU batches (lazily, optionally ahead in a thread) and the corpus layouts that
`gpu_batch.make_batch_pairs` uploads."""
import os
import random

import numpy as np

from .. import readers
from . import segment

ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
                      'assets')


def partition_seed(seed, p):
    """random.seed() value of partition p (documented replacement of the unseeded worker RNG)."""
    return int(seed) * 1000003 + int(p)


def plan_partitions(args):
    """Every partition of the corpus as an unread readers.Block, in the reference's partition
    order (wikipedia, books, common crawl; db.concat, pretrain.py:412-438)."""
    blocksize = args.block_size
    if args.num_blocks is not None:
        if blocksize is not None:
            raise ValueError('Only one of num_blocks or blocksize needs to be set!')
        blocksize = readers.estimate_block_size((args.wikipedia, args.books, args.common_crawl),
                                                args.num_blocks)
    blocks = []
    if args.wikipedia is not None:
        blocks += readers.plan_blocks(readers.wikipedia_dir(args.wikipedia, args.wikipedia_lang),
                                      blocksize, args.sample_ratio, args.seed)
    if args.books is not None:
        blocks += readers.plan_blocks(args.books, blocksize, args.sample_ratio, args.seed)
    if args.common_crawl is not None:
        blocks += readers.plan_blocks(args.common_crawl, blocksize, args.sample_ratio, args.seed)
    return blocks


def greedy(items, size_of, cap):
    """Consecutive runs of `items` of at most `cap` total size (at least one item each)."""
    out, cur, size = [], [], 0
    for it in items:
        b = size_of(it)
        if cur and size + b > cap:
            out.append(cur)
            cur, size = [], 0
        cur.append(it)
        size += b
    if cur:
        out.append(cur)
    return out


def rank_batches(args, blocks, rank=0, world=1):
    """This rank's partitions (p % world == rank) as GPU batches: lists of shuffle groups, each a
    list of partitions. Shuffle groups are runs of ~--shuffle-group-bytes of input and do not
    depend on --gpu-batch-bytes; a batch is a run of whole groups of <= --gpu-batch-bytes."""
    mine = [p for p in range(len(blocks)) if p % world == rank]
    groups = greedy(mine, lambda p: blocks[p].nbytes, args.shuffle_group_bytes)
    return greedy(groups, lambda g: sum(blocks[p].nbytes for p in g), args.gpu_batch_bytes)


def iter_batches(args, rank=0, world=1, blocks=None, as_bytes=False):
    """This rank's partitions in GPU batches, read lazily: yields [(p, lines)] per batch. The
    documents of each shuffle group are shuffled over the group's partitions (each keeps its
    document count) by Random(partition_seed(seed, -1 - first partition of the group)), so the
    output does not depend on the GPU batch size. as_bytes: lines as UTF-8 bytes (the GPU
    segmenter's input) instead of str."""
    blocks = plan_partitions(args) if blocks is None else blocks
    for batch in rank_batches(args, blocks, rank, world):
        out = []
        for g in batch:
            parts = [(p, readers.read_block(blocks[p], as_bytes=as_bytes)) for p in g]
            docs = [d for _, lines in parts for d in lines]
            random.Random(partition_seed(args.seed, -1 - g[0])).shuffle(docs)
            k = 0
            for p, lines in parts:
                out.append((p, docs[k:k + len(lines)]))
                k += len(lines)
        yield out


def iter_doc_batches(args, rank=0, world=1, blocks=None):
    """The GPU-segmentation path's input: this rank's partitions as (partitions, corpus) GPU
    batches, corpus = build_doc_corpus's ('documents', text, doc_off, part_doc_off). Whole shuffle
    groups are read by the library's host reader (readers.read_groups_native: the same lines,
    sampling, per-group document shuffle and split_id_text as iter_batches + build_doc_corpus, in
    C++ threads), then cut into GPU batches of <= --gpu-batch-bytes of input (whole partitions),
    so the GPU work, the rendering and the file writes of consecutive batches overlap."""
    blocks = plan_partitions(args) if blocks is None else blocks
    for batch in rank_batches(args, blocks, rank, world):
        rd = readers.NativeRead([[blocks[p] for p in g] for g in batch],
                                [partition_seed(args.seed, -1 - g[0]) for g in batch],
                                threads=getattr(args, 'read_threads', 16))
        parts = [p for g in batch for p in g]
        pdo = np.zeros(len(parts) + 1, np.int64)
        np.cumsum(rd.block_ndocs, out=pdo[1:])
        try:
            for sub in greedy(list(range(len(parts))), lambda i: blocks[parts[i]].nbytes,
                              args.gpu_batch_bytes):
                i0, i1 = sub[0], sub[-1] + 1
                d0, d1 = int(pdo[i0]), int(pdo[i1])
                text, doc_off = rd.fill(d0, d1)  # this GPU batch's documents only
                yield ([(parts[i], None) for i in range(i0, i1)],
                       ('documents', text, doc_off, pdo[i0:i1 + 1] - d0))
        finally:
            rd.close()


def get_partitions(args, rank=0, world=1):
    """Partitions (lists of raw document lines) owned by `rank`, after sampling and the shuffle."""
    return [pl for batch in iter_batches(args, rank, world) for pl in batch]


def _segment_docs(lines):
    out = []
    for raw in lines:
        if isinstance(raw, bytes):
            raw = raw.decode('utf-8')
        _, sents = segment.document_sentences(raw)
        out.append([s.encode('utf-8') for s in sents])
    return out


def build_corpus(partitions, workers=1):
    """Flatten partitions into the device corpus layout: text bytes, sentence byte offsets,
    document sentence offsets, partition document offsets (host segmentation)."""
    flat = [lines for _, lines in partitions]
    if workers > 1 and sum(len(x) for x in flat) > 2000:
        from multiprocessing import get_context
        with get_context('fork').Pool(workers) as pool:
            segd = pool.map(_segment_docs, flat, chunksize=1)
    else:
        segd = [_segment_docs(x) for x in flat]
    chunks, sent_len, doc_ns, part_nd = [], [], [], []
    for docs in segd:
        part_nd.append(len(docs))
        for sents in docs:
            doc_ns.append(len(sents))
            for s in sents:
                chunks.append(s)
                sent_len.append(len(s))
    text = np.frombuffer(b''.join(chunks), np.uint8) if chunks else np.zeros(0, np.uint8)
    sent_off = np.zeros(len(sent_len) + 1, np.int64)
    np.cumsum(sent_len, out=sent_off[1:])
    doc_sent_off = np.zeros(len(doc_ns) + 1, np.int64)
    np.cumsum(doc_ns, out=doc_sent_off[1:])
    part_doc_off = np.zeros(len(part_nd) + 1, np.int64)
    np.cumsum(part_nd, out=part_doc_off[1:])
    return text, sent_off, doc_sent_off, part_doc_off


def build_doc_corpus(partitions):
    """Raw document texts for the GPU segmenter: the text after each line's id
    (split_id_text, readers.py:131-136), documents back to back, plus document byte offsets and
    partition document offsets."""
    chunks, part_nd = [], []
    for _, lines in partitions:
        part_nd.append(len(lines))
        if lines and isinstance(lines[0], bytes):
            chunks += [readers.split_id_text_bytes(raw)[1] for raw in lines]
        else:
            chunks += [readers.split_id_text(raw)[1].encode('utf-8') for raw in lines]
    text = np.frombuffer(b''.join(chunks), np.uint8) if chunks else np.zeros(0, np.uint8)
    doc_off = np.zeros(len(chunks) + 1, np.int64)
    np.cumsum(np.fromiter(map(len, chunks), np.int64, len(chunks)), out=doc_off[1:])
    part_doc_off = np.zeros(len(part_nd) + 1, np.int64)
    np.cumsum(part_nd, out=part_doc_off[1:])
    return 'documents', text, doc_off, part_doc_off


def punkt_params(args):
    """--punkt-params JSON, else nltk's English model when nltk can load it locally (the
    reference's sent_tokenize), else the untrained parameters (what offline nltk runs)."""
    from ...punkt import PunktParams
    if getattr(args, 'punkt_params', None):
        return PunktParams.from_json(args.punkt_params)
    try:
        import nltk
        return PunktParams.from_nltk(nltk.data.load('tokenizers/punkt/english.pickle'))
    except Exception:  # nltk or its English model unavailable offline
        return PunktParams()


def prefetch(gen, depth=1):
    """Iterate `gen` in a background thread, `depth` items ahead (the host read / decode of batch
    k+1 overlaps the GPU work and the file writes of batch k). Exceptions are re-raised here."""
    import queue
    import threading
    q = queue.Queue(maxsize=depth)
    done = object()

    def run():
        try:
            for item in gen:
                q.put(item)
        except BaseException as e:  # noqa: B902 - handed to the consumer
            q.put(e)
            return
        q.put(done)
    threading.Thread(target=run, daemon=True).start()
    while True:
        item = q.get()
        if item is done:
            return
        if isinstance(item, BaseException):
            raise item
        yield item
