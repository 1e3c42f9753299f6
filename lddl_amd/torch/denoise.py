"""BART denoising on the device (past the reference): `bart_denoise`, one
lddl_bart_denoise launch over the output of `ctx.tokenize` (sentence permutation and text
infilling, include/lddl_amd.h), and `get_bart_pretrain_data_loader`, which feeds it from the
shards `preprocess_bart_pretrain` writes. The kernel is csrc/denoise.hip; this module checks
arguments, allocates the outputs and cuts batches. Every argument error is raised before the
native library is imported.
"""
import glob
import math
import numbers
import os

import numpy as np

from .online import _roundup, mix_seed

_M64 = (1 << 64) - 1
MAX_N = 16  # LDDL_SPAN_MAX_N: the longest span, in words
OUTPUTS = ('input_ids', 'attention_mask', 'decoder_input_ids', 'labels')
SPECIAL_KEYS = {'bos_id', 'eos_id', 'pad_id', 'mask_id', 'decoder_start_id', 'vocab_len'}


def poisson_weights(lam=3.0, n=10):
    """Poisson(lam) on 0 .. n, renormalised: fairseq's span length distribution."""
    w = [math.exp(-lam) * lam ** k / math.factorial(k) for k in range(n + 1)]
    s = sum(w)
    return [x / s for x in w]


def _ratio(name, v):
    if not isinstance(v, numbers.Real) or isinstance(v, bool) or not 0 <= v <= 1:
        raise ValueError('{} must be a number in [0, 1], not {!r}'.format(name, v))
    return float(v)


def check_noise(mask, poisson_lambda=3.0, span_weights=None, permute_sentence_ratio=1.0,
                random_ratio=0.1, sequence_length_alignment=8, seq_len=None):
    """The argument errors of bart_denoise (ValueError) -> (mask_ratio, seed, counter, weights).
    weights: P(len = k) up to a factor, k = 0 .. n with n <= MAX_N."""
    try:
        ratio, seed, counter = mask
    except (TypeError, ValueError):
        raise ValueError('mask must be (mask_ratio, seed, counter), not {!r}'.format(mask)) from None
    _ratio('mask_ratio', ratio)
    _ratio('permute_sentence_ratio', permute_sentence_ratio)
    _ratio('random_ratio', random_ratio)
    if span_weights is None:
        if not isinstance(poisson_lambda, numbers.Real) or not 0 < poisson_lambda < math.inf:
            raise ValueError('poisson_lambda must be a positive number')
        weights = poisson_weights(float(poisson_lambda))
    else:
        try:
            weights = [float(w) for w in span_weights]
        except (TypeError, ValueError):
            raise ValueError('span_weights must be a sequence of numbers') from None
        if not 2 <= len(weights) <= MAX_N + 1:
            raise ValueError('span_weights: lengths 0 .. n with 1 <= n <= {}, not {} '
                             'entries'.format(MAX_N, len(weights)))
        if any(not (w >= 0 and w < math.inf) for w in weights) or not sum(weights) > 0:
            raise ValueError('span_weights must be finite, >= 0 and not all zero')
    if not isinstance(sequence_length_alignment, int) or sequence_length_alignment < 1:
        raise ValueError('sequence_length_alignment must be an int >= 1')
    if seq_len is not None and (not isinstance(seq_len, int) or isinstance(seq_len, bool) or
                                seq_len < 2):
        raise ValueError('seq_len must be an int >= 2 (bos and eos), not {!r}'.format(seq_len))
    return float(ratio), int(seed) & _M64, int(counter) & _M64, weights


def make_params(mask_ratio, weights):
    """lddl_denoise_params_make: the DenoiseParams of the weights (lengths 0 .. n) at mask_ratio.
    NativeError if p_start = 1 cannot reach the ratio."""
    import ctypes
    from .._native import DenoiseParams, check, lib
    dp = DenoiseParams()
    w = (ctypes.c_double * len(weights))(*weights)
    check(lib.lddl_denoise_params_make(float(mask_ratio), len(weights) - 1, w, ctypes.byref(dp)))
    return dp


def sample_lengths(sent_len, doc_sent_off):
    """Pieces per document (int64 cuda tensor [n_docs]) of a tokenized batch; no sync."""
    import torch
    from ..context import LEN_MASK
    cs = torch.zeros(sent_len.numel() + 1, dtype=torch.int64, device=sent_len.device)
    cs[1:] = torch.cumsum((sent_len & LEN_MASK).to(torch.int64), 0)
    return cs[doc_sent_off[1:]] - cs[doc_sent_off[:-1]]


def bart_denoise(ctx, ids, sent_off, sent_len, doc_sent_off, rows=None, seq_len=None,
                 mask=(0.3, 0, 0), poisson_lambda=3.0, span_weights=None,
                 permute_sentence_ratio=1.0, random_ratio=0.1, sequence_length_alignment=8,
                 ignore_index=-100, *, check=True, bos_id=None, eos_id=None, pad_id=None,
                 mask_id=None, decoder_start_id=None, vocab_len=None, draw_stride=None,
                 params=None):
    """BART's noise on rows `rows` (int64 cuda tensor of document indices, None = all) of the
    tokenized batch (ids, sent_len) = ctx.tokenize(text, sent_off) with doc_sent_off of
    punkt.segment: sentences permuted (each takes part with permute_sentence_ratio), spans of
    whole words with Poisson(poisson_lambda) lengths on 0 .. 10 (or span_weights[k] for length
    k) replaced by one mask token each, a span of length 0 inserting one; a deep word is deleted
    or replaced with probability mask_ratio; a noise token is a random id with random_ratio.
    mask = (mask_ratio, seed, counter): equal triples give equal noise. Returns the dict of
    int64 [B, L] input_ids, attention_mask, decoder_input_ids, labels and int32 [B] src_lengths
    (the untruncated source length: > L tells that insertions pushed ids out of the row).

    A sample keeps its first L - 2 pieces. seq_len=None makes L the longest sample + 2, rounded
    up to sequence_length_alignment, which costs the one device sync; check=True refuses a row
    index outside the batch (IndexError; the same sync). The special ids default to the
    context's [CLS], [SEP], [PAD] and [MASK] (a `BpeContext` in place of the `Context`: <s>,
    </s>, <pad> and <mask>, and a word begins at a piece that opens with a space),
    decoder_start_id to eos_id, vocab_len to len(ctx). params: a DenoiseParams made by hand in place of the one of mask_ratio and the
    weights (e.g. p_start = 1 and cum all 1: an inserted token before every word)."""
    ratio, seed, counter, weights = check_noise(mask, poisson_lambda, span_weights,
                                                permute_sentence_ratio, random_ratio,
                                                sequence_length_alignment, seq_len)
    import ctypes
    import torch
    from .._native import check as _check, lib
    from ..context import _ptr, _stream
    sp = ctx.special_ids
    from ..bpe import BpeContext
    # a BpeContext: its bitmap goes to the _bits entry
    bits = ctx.cont_bits if isinstance(ctx, BpeContext) else None
    names = ('[CLS]', '[SEP]', '[PAD]', '[MASK]') if bits is None else \
        ('<s>', '</s>', '<pad>', '<mask>')
    bos, eos, pad, msk = (sp[n] if v is None else int(v)
                          for n, v in zip(names, (bos_id, eos_id, pad_id, mask_id)))
    if min(bos, eos, pad, msk) < 0:
        raise ValueError('the vocab lacks {}, {}, {} or {}: pass bos_id, eos_id, pad_id and '
                         'mask_id'.format(*names))
    dec = eos if decoder_start_id is None else int(decoder_start_id)
    if params is None:
        params = make_params(ratio, weights)
    for t, dt in ((ids, torch.int32), (sent_len, torch.int32), (sent_off, torch.int64),
                  (doc_sent_off, torch.int64)) + (() if rows is None else ((rows, torch.int64),)):
        assert t.dtype == dt and t.is_cuda and t.is_contiguous()
    n_docs = doc_sent_off.numel() - 1
    B = n_docs if rows is None else rows.numel()
    if B and not n_docs:
        raise IndexError('rows given, the batch has no documents')
    if B and (seq_len is None or (check and rows is not None)):
        stat = [] if rows is None else [rows.min(), rows.max()]
        if seq_len is None:
            n = sample_lengths(sent_len, doc_sent_off)
            stat.append((n if rows is None else n[rows.clamp(0, n_docs - 1)]).max())
        stat = torch.stack(stat).tolist()  # the one sync
        if rows is not None and (stat[0] < 0 or stat[1] >= n_docs):
            raise IndexError('rows hold {}..{}, the batch has {} documents'.format(
                stat[0], stat[1], n_docs))
        if seq_len is None:
            seq_len = _roundup(stat[-1] + 2, sequence_length_alignment)
    L = int(seq_len or 2)
    dev = ctx.device
    out = {k: torch.empty(B, L, dtype=torch.long, device=dev) for k in OUTPUTS}
    out['src_lengths'] = torch.empty(B, dtype=torch.int32, device=dev)
    entry, owner = (lib.lddl_bart_denoise, (ctx.handle,)) if bits is None else \
        (lib.lddl_bart_denoise_bits, bits)
    _check(entry(
        *owner, _stream(), _ptr(ids), _ptr(sent_off), _ptr(sent_len), _ptr(doc_sent_off),
        _ptr(rows), B, L, *[_ptr(out[k]) for k in OUTPUTS], _ptr(out['src_lengths']), bos, eos,
        pad, msk, dec, int(ignore_index), len(ctx) if vocab_len is None else int(vocab_len), seed,
        counter, L if draw_stride is None else int(draw_stride), float(permute_sentence_ratio),
        float(random_ratio), ctypes.cast(ctypes.pointer(params), ctypes.c_void_p)))
    return out


# ---- the loader ------------------------------------------------------------------------------
def shard_files(path):
    """The shards of a preprocess_bart_pretrain output directory in partition order, and their
    format: part.<i>.parquet, else <i>.txt."""
    if not isinstance(path, str) or not os.path.isdir(path):
        raise FileNotFoundError('path {!r} is not a directory'.format(path))
    for fmt, pat in (('parquet', 'part.*.parquet'), ('txt', '*.txt')):
        files = glob.glob(os.path.join(path, pat))
        if files:
            num = lambda f: int(''.join(c for c in os.path.basename(f) if c.isdigit()) or 0)  # noqa: E731
            return sorted(files, key=lambda f: (num(f), f)), fmt
    raise FileNotFoundError('no part.*.parquet or *.txt shards under {!r}'.format(path))


def validate_args(path=None, vocab_file=None, batch_size=None, max_seq_length=512,
                  mask_ratio=0.3, rank=None, world=None, round_bytes=32 << 20, bpe=None,
                  bpe_tables=None, **kw):
    """Every argument error of get_bart_pretrain_data_loader, raised before the GPU is touched.
    Returns (files, format). bpe_tables: a list that takes the parsed (tokens, vocab, merges,
    keywords) of bpe= (`lddl_amd.bpe.load_bpe_arg`), so that the loader does not read the two files again."""
    shards = shard_files(path)
    if bpe is not None:
        if vocab_file is not None:
            raise ValueError('pass vocab_file (WordPiece) or bpe=, not both')
        from ..bpe import load_bpe_arg
        tables = load_bpe_arg(bpe)
        if bpe_tables is not None:
            bpe_tables[:] = tables
    elif not isinstance(vocab_file, str) or not os.path.isfile(vocab_file):
        raise FileNotFoundError('vocab_file {!r}: a local vocab.txt is required'.format(vocab_file))
    if not isinstance(batch_size, int) or isinstance(batch_size, bool) or batch_size < 1:
        raise ValueError('batch_size must be a positive int')
    check_noise((mask_ratio, 0, 0), kw['poisson_lambda'], kw['span_weights'],
                kw['permute_sentence_ratio'], kw['random_ratio'],
                kw['sequence_length_alignment'], max_seq_length)
    if (rank is None) != (world is None):
        raise ValueError('pass both rank and world, or neither')
    if rank is not None and not 0 <= rank < world:
        raise ValueError('rank must be in [0, world)')
    if not isinstance(round_bytes, int) or round_bytes < 1:
        raise ValueError('round_bytes must be a positive int')
    unknown = set(kw['special_ids'] or ()) - SPECIAL_KEYS
    if unknown:
        raise ValueError('special_ids: unknown keys {}'.format(sorted(unknown)))
    return shards


def read_chunks(fn, fmt):
    """The chunks (bytes) of one shard."""
    if fmt == 'parquet':
        import pyarrow.parquet as pq
        col = pq.read_table(fn, columns=['sentences']).column('sentences')
        return [s.encode('utf-8') for s in col.to_pylist()]
    with open(fn, 'rb') as f:
        return [ln for ln in f.read().split(b'\n') if ln]


class BartPretrainLoader:
    """The iterable get_bart_pretrain_data_loader returns; each iter() is one epoch."""

    def __init__(self, **kw):
        self._bpe_tables = []
        self.files, self.format = validate_args(bpe_tables=self._bpe_tables, **kw)
        self._kw = kw
        self._epoch = kw['start_epoch']
        self._ctx = None

    def _setup(self):
        from .. import punkt
        from ..context import Context
        from ..dask.bert.corpus import punkt_params
        from .utils import get_rank, get_world_size
        from types import SimpleNamespace
        kw = self._kw
        self.rank, self.world = (get_rank(), get_world_size()) if kw['rank'] is None else \
            (kw['rank'], kw['world'])
        # Punkt's tables live in a Context. With bpe= it is one of the packaged WordPiece
        # vocabulary that only segments: its 30 k-entry tokenizer tables are built and never
        # read, the price of not giving Punkt an owner of its own here.
        self._bpe = None
        if kw['bpe'] is not None:
            from ..bpe import BpeContext
            from ..context import ASSETS
            self._bpe = BpeContext.from_tables(self._bpe_tables[0], self._bpe_tables[2],
                                               vocab=self._bpe_tables[1], **self._bpe_tables[3])
        self._ctx = Context(kw['vocab_file'] if self._bpe is None else os.path.join(
            ASSETS, 'vocab_synth_uncased_30522.txt'), do_lower_case=kw['do_lower_case'])
        pp = kw['punkt_params']
        if pp is None or isinstance(pp, str):
            pp = punkt_params(SimpleNamespace(punkt_params=pp))
        punkt.set_params(self._ctx, pp)
        self._params = make_params(kw['mask_ratio'], check_noise(
            (kw['mask_ratio'], 0, 0), kw['poisson_lambda'], kw['span_weights'])[3])
        self.seed = mix_seed(kw['base_seed'], self.rank)

    def rounds(self):
        """This rank's shards (files[rank::world]) in runs of at most round_bytes of file size,
        one shard at least."""
        run, size = [], 0
        for f in self.files[self.rank::self.world]:
            n = os.path.getsize(f)
            if run and size + n > self._kw['round_bytes']:
                yield run
                run, size = [], 0
            run.append(f)
            size += n
        if run:
            yield run

    def tokenize_round(self, files):
        """One round on the device: (ids, sent_off, sent_len, doc_sent_off) and, on the host,
        the pieces of every chunk (the round's one sync)."""
        import torch
        from .. import punkt
        chunks = [c for f in files for c in read_chunks(f, self.format)]
        ctx = self._ctx
        text = torch.from_numpy(np.frombuffer(b''.join(chunks) or b' ', np.uint8).copy()).to(ctx.device)
        doc_off = np.zeros(len(chunks) + 1, np.int64)
        np.cumsum([len(c) for c in chunks], out=doc_off[1:])
        sent_off, doc_sent_off = punkt.segment(ctx, text, torch.from_numpy(doc_off).to(ctx.device))
        if self._bpe is None:
            ids, sent_len = ctx.tokenize(text, sent_off, self._kw['max_pieces'])
        else:  # per document: a pre-token goes to the sentence of its last byte
            ids, sent_len = self._bpe.tokenize(text, sent_off, doc_sent_off, self._kw['max_pieces'])
        table = (ids, sent_off, sent_len, doc_sent_off)
        return table, sample_lengths(sent_len, doc_sent_off).cpu().numpy()

    def order(self, epoch, rnd, n):
        """The seeded shuffle of a round's n chunks."""
        return np.random.Generator(np.random.PCG64(mix_seed(
            self._kw['base_seed'], epoch, self.rank, rnd))).permutation(n).astype(np.int64)

    def denoise(self, table, rows, L, epoch, step):
        kw = self._kw
        return bart_denoise(
            self._bpe or self._ctx, *table, rows=rows, seq_len=L, mask=(kw['mask_ratio'], self.seed,
                                                           (epoch << 32) | step),
            permute_sentence_ratio=kw['permute_sentence_ratio'], random_ratio=kw['random_ratio'],
            ignore_index=kw['ignore_index'], check=False, params=self._params,
            **(kw['special_ids'] or {}))

    def __iter__(self):
        if self._ctx is None:
            self._setup()
        epoch = self._epoch
        self._epoch += 1
        return self._run_epoch(epoch)

    def _run_epoch(self, epoch):
        import torch
        kw = self._kw
        bs, a, step = kw['batch_size'], kw['sequence_length_alignment'], 0
        for rnd, files in enumerate(self.rounds()):
            table, n_pieces = self.tokenize_round(files)
            perm = self.order(epoch, rnd, len(n_pieces))
            d_perm = torch.from_numpy(perm).to(self._ctx.device)
            for r0 in range(0, len(perm), bs):
                r1 = min(r0 + bs, len(perm))
                if r1 - r0 < bs and kw['drop_last']:
                    break
                L = min(_roundup(int(n_pieces[perm[r0:r1]].max()) + 2, a), kw['max_seq_length'])
                with torch.no_grad():
                    yield self.denoise(table, d_perm[r0:r1], L, epoch, step)
                step += 1


def get_bart_pretrain_data_loader(path, vocab_file=None, batch_size=None, max_seq_length=512,
                                  mask_ratio=0.3, poisson_lambda=3.0, span_weights=None,
                                  permute_sentence_ratio=1.0, random_ratio=0.1,
                                  sequence_length_alignment=8, ignore_index=-100,
                                  base_seed=12345, start_epoch=0, rank=None, world=None,
                                  drop_last=False, round_bytes=32 << 20, max_pieces=512,
                                  do_lower_case=True, punkt_params=None, special_ids=None,
                                  bpe=None):
    """BART pretraining batches from the shards of `preprocess_bart_pretrain` (parquet or txt)
    under `path` (past the reference, which has no BART loader). One process, one
    stream, no DataLoader workers: a round of shards (at most round_bytes; this rank's are
    files[rank::world]) goes to the device as one text buffer, through punkt.segment and
    ctx.tokenize; a seeded shuffle cuts its chunks into batches, and each step is one
    bart_denoise call on batch_size chunks with counter = (epoch << 32) | step. Yields
    bart_denoise's dicts with L = the batch's longest chunk + 2, aligned, at most
    max_seq_length (a longer chunk keeps its first max_seq_length - 2 pieces). special_ids:
    bos_id, eos_id, pad_id, mask_id, decoder_start_id and vocab_len as bart_denoise takes them.
    bpe=(vocab_json, merges_txt) in place of vocab_file: the chunks are tokenized by the
    byte-level BPE of a GPT-2 / RoBERTa / BART checkpoint (`lddl_amd.bpe.BpeContext`, DESIGN
    §29), per chunk, and bos / eos / pad / mask are the vocabulary's <s>, </s>, <pad>, <mask>.
    The ranks do not agree on a number of steps: each yields what its shards hold."""
    return BartPretrainLoader(**dict(locals()))
