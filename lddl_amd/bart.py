"""BART pretraining chunks on the GPU: the reference's `_aggregate_sentences`
(lddl/dask/bart/pretrain.py:88-128) for a whole batch of segmented documents at once
(csrc/bart.hip, C-ABI `lddl_bart_count` / `lddl_bart_fill`; whitespace is the class table of
csrc/punkt.hip read through csrc/punkt_classes.h).

Per document, sentences in order: `chunk += " " + sentence`, `num_tokens +=
len(sentence.split())`; the chunk is emitted and both reset when `num_tokens >=
target_seq_length - 3`, and what is left after the last sentence is emitted if it has a word.
"""
import ctypes

import numpy as np
import torch

from ._native import lib, check


def aggregate(ctx, text, sent_off, doc_sent_off, target_seq_length):
    """Chunks of every document of a device batch.

    text: uint8 cuda tensor; sent_off int64[n_sent+1], doc_sent_off int64[n_doc+1]: the layout
    `punkt.segment` returns (sentences contiguous, whitespace between sentences attached to the
    left one, a whitespace-only sentence = a dropped one). Returns device tensors
    (bytes uint8[n_out], chunk_off int64[n_chunks+1], num_tokens int32[n_chunks],
    doc_chunk_off int64[n_doc+1]): chunk c is bytes[chunk_off[c]:chunk_off[c+1]], document d's
    chunks are doc_chunk_off[d]:doc_chunk_off[d+1].
    """
    from . import punkt
    from .context import _ptr, _stream
    assert text.dtype == torch.uint8 and text.is_cuda
    assert sent_off.dtype == torch.int64 and doc_sent_off.dtype == torch.int64
    if not hasattr(ctx, '_punkt_params'):
        punkt.set_params(ctx)
    n_sent, n_doc = sent_off.numel() - 1, doc_sent_off.numel() - 1
    if n_sent < 0 or n_doc < 0:
        raise ValueError('sent_off and doc_sent_off need at least one entry')
    if n_sent > 0:  # the kernels trust the offsets: check them once, on the device
        ds, dd = sent_off[1:] - sent_off[:-1], doc_sent_off[1:] - doc_sent_off[:-1]
        lim = torch.stack([ds.min(), ds.max(), sent_off[0], sent_off[-1],
                           dd.min() if n_doc else doc_sent_off[0], doc_sent_off[0],
                           doc_sent_off[-1]]).cpu().tolist()
        if lim[0] < 0 or lim[1] >= 1 << 31 or lim[2] < 0 or lim[3] > text.numel():
            raise ValueError('sentences must be ordered, inside the text and < 2 GiB each')
        if lim[4] < 0 or lim[5] != 0 or lim[6] != n_sent:
            raise ValueError('doc_sent_off must rise from 0 to the number of sentences')
    elif n_doc > 0 and bool((doc_sent_off != 0).any()):
        raise ValueError('doc_sent_off must rise from 0 to the number of sentences')
    n_chunks, n_out = ctypes.c_int64(), ctypes.c_int64()
    check(lib.lddl_bart_count(ctx._h, _stream(), _ptr(text), text.numel(), _ptr(sent_off), n_sent,
                              _ptr(doc_sent_off), n_doc, int(target_seq_length) - 3,
                              ctypes.byref(n_chunks), ctypes.byref(n_out)))
    filled = False
    try:
        dev = ctx.device
        out = torch.empty(max(n_out.value, 1), dtype=torch.uint8, device=dev)
        chunk_off = torch.empty(n_chunks.value + 1, dtype=torch.int64, device=dev)
        num_tokens = torch.empty(max(n_chunks.value, 1), dtype=torch.int32, device=dev)
        doc_chunk_off = torch.empty(n_doc + 1, dtype=torch.int64, device=dev)
        check(lib.lddl_bart_fill(ctx._h, _stream(), _ptr(out), _ptr(chunk_off), _ptr(num_tokens),
                                 _ptr(doc_chunk_off)))
        filled = True
    finally:
        if not filled:  # e.g. an allocation failed: cancel, so the context stays usable
            lib.lddl_bart_fill(ctx._h, _stream(), None, None, None, None)
    return out[:n_out.value], chunk_off, num_tokens[:n_chunks.value], doc_chunk_off


def chunk_strings(out, chunk_off, doc_chunk_off=None):
    """Host helper (tests, debugging): the chunks as str, flat or per document."""
    data = bytes(np.asarray(out, np.uint8))
    co = np.asarray(chunk_off)
    flat = [data[co[k]:co[k + 1]].decode('utf-8') for k in range(len(co) - 1)]
    if doc_chunk_off is None:
        return flat
    dc = np.asarray(doc_chunk_off)
    return [flat[dc[d]:dc[d + 1]] for d in range(len(dc) - 1)]
