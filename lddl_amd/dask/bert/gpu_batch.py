"""One batch of partitions through the GPU for `preprocess_bert_pretrain`: upload, segment,
tokenize, pairs (`make_batch_pairs`), then bin and render (`render_batch`). Everything here
launches on the caller's current stream; the host copy and the files are writers.py's."""
import numpy as np

from .corpus import build_doc_corpus, partition_seed


def make_batch_pairs(ctx, args, partitions, corpus, timer=None):
    """The GPU hot path over one batch of partitions -> PairBatch (pairs in partition order)."""
    import torch
    from ...pairs import make_pairs
    dev = ctx.device
    tm = timer or (lambda name: None)
    if corpus[0] == 'documents':  # GPU Punkt: sentences of every document of the batch
        from ... import punkt
        _, text, doc_off, part_doc_off = corpus
        d_text = torch.from_numpy(text).to(dev) if len(text) else torch.zeros(
            1, dtype=torch.uint8, device=dev)[:0]
        d_doc = torch.from_numpy(doc_off).to(dev)
        tm('h2d')
        bad = punkt.utf8_first_invalid(d_text)
        if bad >= 0:  # dask.bag.read_text decodes strictly: the reference raises here too
            raise UnicodeDecodeError('utf-8', bytes(text[max(bad - 8, 0):bad + 8]), 0, 1,
                                     'invalid UTF-8 in the input documents (byte {} of the '
                                     'batch text)'.format(bad))
        d_so, d_dso = punkt.segment(ctx, d_text, d_doc)
        tm('segment')
    else:
        _, text, sent_off, doc_sent_off, part_doc_off = corpus
        d_text = torch.from_numpy(text).to(dev) if len(text) else torch.zeros(
            1, dtype=torch.uint8, device=dev)[:0]
        d_so = torch.from_numpy(sent_off).to(dev)
        d_dso = torch.from_numpy(doc_sent_off).to(dev)
        tm('h2d')
    ids, sent_len = ctx.tokenize(d_text, d_so, max_pieces=512)
    tm('tokenize')
    seeds = np.asarray([partition_seed(args.seed, p) for p, _ in partitions], np.int64)
    pb = make_pairs(ctx, d_so, ids, sent_len, d_dso,
                    torch.from_numpy(part_doc_off).to(dev), torch.from_numpy(seeds).to(dev),
                    seq=args.target_seq_length, dup=args.duplicate_factor, masking=args.masking,
                    short_seq_prob=args.short_seq_prob, masked_lm_ratio=args.masked_lm_ratio,
                    rng=getattr(args, 'rng', 'replay'), native_seed=args.seed,
                    whole_word=getattr(args, 'whole_word_masking', False))
    tm('pairs')
    return pb


def render_batch(ctx, args, pb):
    """Bin (with --bin-size) and render PairBatch `pb` on the device -> (DeviceRendered, nbins,
    counts): counts is the device int64[n_part, nbins] of rows per (partition, bin), nbins and
    counts None unbinned."""
    from ... import output
    if args.bin_size is None:
        return output.render_device(ctx, pb), None, None
    nbins = args.target_seq_length // args.bin_size
    perm, bin_id, counts = output.bin_partitions(ctx, None, pb.part_off, args.bin_size, nbins,
                                                 tok_off=pb.tok_off)
    return output.render_device(ctx, pb, perm, bin_id), nbins, counts


def _warm_gpu_path(ctx, args):
    """One tiny batch of made-up documents through segment -> tokenize -> pairs -> render, output
    discarded: the first launch of each kernel (code object loading) and the first allocations
    happen here, while the host reader is still reading, instead of in the first real batch."""
    import torch
    doc = ('The first sentence is here. A second one follows it! Then a third, with more words '
           'in it? The fourth ends the document.')
    lines = [('{} {}'.format(k, doc)).encode('utf-8') for k in range(8)]
    corpus = build_doc_corpus([(0, lines[:4]), (1, lines[4:])])
    pb = make_batch_pairs(ctx, args, [(0, None), (1, None)], corpus)
    render_batch(ctx, args, pb)
    torch.cuda.synchronize(ctx.device)


def _empty_pairs(ctx, masking):
    """A PairBatch without rows (a rank with fewer batches still takes part in the collectives)."""
    import torch
    from ...pairs import PairBatch
    dev = ctx.device
    e64 = torch.zeros(1, dtype=torch.int64, device=dev)
    pb = PairBatch(torch.zeros(0, dtype=ctx.id_dtype, device=dev), e64,
                   torch.zeros(0, dtype=torch.int32, device=dev),
                   torch.zeros(0, dtype=torch.uint8, device=dev))
    if masking:
        pb.pos = torch.zeros(0, dtype=torch.int16, device=dev)
        pb.labels = torch.zeros(0, dtype=ctx.id_dtype, device=dev)
        pb.pos_off = e64.clone()
    return pb


def _copy_stream(ctx):
    import torch
    s = getattr(ctx, '_copy_stream', None)
    if s is None:
        s = ctx._copy_stream = torch.cuda.Stream(device=ctx.device)
    return s
