"""RoBERTa input on the device (past the reference): rows of contiguous whole
sentences without NSP, FULL-SENTENCES or DOC-SENTENCES, with dynamic masking. `roberta_blocks`
cuts a tokenized round into blocks (lddl_blocks_plan), `collate_blocks` writes rows from them
(lddl_collate_blocks / lddl_collate_blocks_masked) and `get_roberta_pretrain_data_loader` feeds
both from text files. include/lddl_amd.h states the semantics; the kernels are
csrc/blocks_plan.hip and csrc/blocks_collate.hip. Every argument error is raised before the
native library is imported.
"""
import glob
import numbers
import os

import numpy as np

from .online import mix_seed

_M64 = (1 << 64) - 1
MODES = {'full': 0, 'doc': 1}  # LDDL_BLOCKS_FULL, LDDL_BLOCKS_DOC
TILE = 2048                    # LDDL_BLOCKS_TILE
LDS_SENTS = 256                # LDDL_BLOCKS_LDS_SENTS
SPECIAL_KEYS = {'bos_id', 'eos_id', 'pad_id', 'mask_id', 'vocab_len'}


def _seq_len(seq_len):
    if not isinstance(seq_len, int) or isinstance(seq_len, bool) or not 3 <= seq_len <= 1 << 24:
        raise ValueError('seq_len must be an int in [3, 2^24] (bos, a piece, eos), not '
                         '{!r}'.format(seq_len))
    return seq_len


def _mode(mode):
    if mode not in MODES:
        raise ValueError("mode must be 'full' or 'doc', not {!r}".format(mode))
    return MODES[mode]


def check_mask(mask, whole_word=False, span=None, special_ids=None):
    """The argument errors of collate_blocks' masking (ValueError) -> None or (p, seed, counter)."""
    unknown = set(special_ids or ()) - SPECIAL_KEYS
    if unknown:
        raise ValueError('special_ids: unknown keys {}'.format(sorted(unknown)))
    if whole_word and span is not None:
        raise ValueError('pass whole_word=True or span=, not both (span=1 is whole-word masking)')
    if mask is None:
        if whole_word or span is not None:
            raise ValueError('whole_word and span need mask=(p, seed, counter)')
        return None
    try:
        p, seed, counter = mask
    except (TypeError, ValueError):
        raise ValueError('mask must be None or (p, seed, counter), not {!r}'.format(mask)) from None
    if not isinstance(p, numbers.Real) or isinstance(p, bool) or not 0 <= p <= 1:
        raise ValueError('mask: p must be a number in [0, 1], not {!r}'.format(p))
    return float(p), int(seed) & _M64, int(counter) & _M64


class BlockPlan:
    """lddl_blocks_plan's outputs on the device: piece_off int64 [n_sent + 1], sent_sep uint8
    [n_sent], block_sent int64 and block_len int32 [n_sent + 1] (n_blocks entries are blocks,
    block_sent[n_blocks] = n_sent), n_blocks int64 [1]."""
    __slots__ = ('piece_off', 'sent_sep', 'block_sent', 'block_len', 'n_blocks', 'seq_len', 'mode')

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def roberta_blocks(table, seq_len, mode='full'):
    """The blocks of the token table (ids, sent_off, sent_len, doc_sent_off) of `ctx.tokenize`
    / `BpeContext.tokenize` and `punkt.segment` at rows of seq_len slots: whole sentences up to
    seq_len - 2 pieces, across documents with one separator at each crossing (mode='full') or
    within a document (mode='doc'). Returns (BlockPlan, n_blocks); reading n_blocks is the one
    device sync."""
    L, m = _seq_len(seq_len), _mode(mode)
    import torch
    from .._native import check, lib
    from ..context import _ptr, _stream
    _, _, sent_len, doc_sent_off = table
    assert sent_len.dtype == torch.int32 and sent_len.is_cuda and sent_len.is_contiguous()
    assert doc_sent_off.dtype == torch.int64 and doc_sent_off.is_cuda and doc_sent_off.is_contiguous()
    n, dev = sent_len.numel(), sent_len.device
    plan = BlockPlan(piece_off=torch.empty(n + 1, dtype=torch.int64, device=dev),
                     sent_sep=torch.empty(max(n, 1), dtype=torch.uint8, device=dev),
                     block_sent=torch.empty(n + 1, dtype=torch.int64, device=dev),
                     block_len=torch.empty(n + 1, dtype=torch.int32, device=dev),
                     n_blocks=torch.empty(1, dtype=torch.int64, device=dev), seq_len=L, mode=mode)
    check(lib.lddl_blocks_plan(_stream(), _ptr(sent_len), n, _ptr(doc_sent_off),
                               doc_sent_off.numel() - 1, L, m, _ptr(plan.piece_off),
                               _ptr(plan.sent_sep), _ptr(plan.block_sent), _ptr(plan.block_len),
                               _ptr(plan.n_blocks)))
    return plan, int(plan.n_blocks.item())


def collate_blocks(bpe_or_ctx, table, plan, rows=None, seq_len=None, mask=None, whole_word=False,
                   span=None, ignore_index=-100, special_ids=None):
    """Rows `rows` (int64 cuda tensor of block indices, None = every block, which reads
    n_blocks; the indices are the caller's to check) of the plan: dict of int64 [B, seq_len]
    input_ids (<s>, the sentences' pieces with </s> behind a document's end, </s>, <pad>) and
    attention_mask, and labels when masked, special_tokens_mask when not. mask=(p, seed,
    counter): per-token dynamic masking; whole_word=True masks whole words (a word begins at a
    sentence's first piece and at an id that is no continuation id), span=N or a list of N
    probabilities masks runs of up to N words (`lddl_amd.torch.span`). Equal triples give equal
    masks. special_ids: bos_id, eos_id, pad_id, mask_id, vocab_len in place of the
    vocabulary's. seq_len must be the plan's."""
    m = check_mask(mask, whole_word, span, special_ids)
    L = plan.seq_len if seq_len is None else _seq_len(seq_len)
    if L != plan.seq_len:
        raise ValueError('seq_len {} is not the plan\'s {}'.format(L, plan.seq_len))
    import torch
    from .._native import check, lib
    from ..bpe import BpeContext
    from ..context import _ptr, _stream
    from ..unigram import UnigramContext
    ctx, sp = bpe_or_ctx, dict(special_ids or {})
    names = ('<s>', '</s>', '<pad>', '<mask>') if isinstance(ctx, (BpeContext, UnigramContext)) else \
        ('[CLS]', '[SEP]', '[PAD]', '[MASK]')
    bos, eos, pad, msk = (int(sp[k]) if k in sp else ctx.special_ids.get(n, -1)
                          for k, n in zip(('bos_id', 'eos_id', 'pad_id', 'mask_id'), names))
    if min(bos, eos, pad) < 0 or (m is not None and msk < 0):
        raise ValueError('the vocab lacks {}, {}, {} or {}: pass special_ids'.format(*names))
    ids, sent_off = table[0], table[1]
    for t, dt in ((ids, torch.int32), (sent_off, torch.int64)) + \
            (() if rows is None else ((rows, torch.int64),)):
        assert t.dtype == dt and t.is_cuda and t.is_contiguous()
    B = int(plan.n_blocks.item()) if rows is None else rows.numel()
    dev = ids.device
    out = {k: torch.empty(B, L, dtype=torch.long, device=dev) for k in (
        'input_ids', 'attention_mask', 'special_tokens_mask' if m is None else 'labels')}
    head = (_stream(), _ptr(ids), _ptr(sent_off), _ptr(plan.piece_off), _ptr(plan.sent_sep),
            _ptr(plan.block_sent), _ptr(rows), B, L)
    if m is None:
        check(lib.lddl_collate_blocks(*head, *[_ptr(v) for v in out.values()], bos, eos, pad))
        return out
    params, bits = None, (None, len(ctx))
    if whole_word or span is not None:
        from . import span as span_mod
        params = span_mod.parse(1 if whole_word else span).ptr(m[0])
        bits = getattr(ctx, 'cont_bits', None)
        if bits is None:
            raise ValueError('word masking needs a context with a continuation bitmap '
                             '(a BpeContext)')
    check(lib.lddl_collate_blocks_masked(
        *bits, *head, *[_ptr(v) for v in out.values()], bos, eos, pad, msk, m[0],
        int(ignore_index), int(sp.get('vocab_len', len(ctx))), m[1], m[2], params))
    return out


# ---- the loader ------------------------------------------------------------------------------
def text_files(path):
    if not isinstance(path, str) or not os.path.isdir(path):
        raise FileNotFoundError('path {!r} is not a directory'.format(path))
    files = sorted(glob.glob(os.path.join(path, '*.txt')))
    if not files:
        raise FileNotFoundError('no *.txt files under {!r}'.format(path))
    return files


def validate_args(path=None, bpe=None, batch_size=None, max_seq_length=512, mode='full',
                  mlm_probability=0.15, whole_word_masking=False, span=None, rank=None,
                  world=None, round_bytes=32 << 20, special_ids=None, bpe_tables=None,
                  unigram=None, unigram_tables=None, **kw):
    """Every argument error of get_roberta_pretrain_data_loader, raised before the GPU is
    touched. Returns the files. bpe_tables takes the parsed (tokens, vocab, merges, keywords) of bpe=
    (`lddl_amd.bpe.load_bpe_arg`: the two files, the two and a dict, or a tokenizer.json),
    unigram_tables what `lddl_amd.unigram.load_model` reads from unigram=."""
    files = text_files(path)
    if unigram is not None:
        if bpe is not None:
            raise ValueError('pass bpe= or unigram=, not both')
        from ..unigram import load_model
        tables = load_model(unigram)
        if unigram_tables is not None:
            unigram_tables[:] = tables
    else:
        from ..bpe import load_bpe_arg
        tables = load_bpe_arg(bpe)
        if bpe_tables is not None:
            bpe_tables[:] = tables
    if not isinstance(batch_size, int) or isinstance(batch_size, bool) or batch_size < 1:
        raise ValueError('batch_size must be a positive int')
    _seq_len(max_seq_length)
    _mode(mode)
    check_mask((mlm_probability, 0, 0), whole_word_masking, span, special_ids)
    if (rank is None) != (world is None):
        raise ValueError('pass both rank and world, or neither')
    if rank is not None and not 0 <= rank < world:
        raise ValueError('rank must be in [0, world)')
    if not isinstance(round_bytes, int) or round_bytes < 1:
        raise ValueError('round_bytes must be a positive int')
    return files


class RobertaPretrainLoader:
    """The iterable get_roberta_pretrain_data_loader returns; each iter() is one epoch."""

    def __init__(self, **kw):
        self._bpe_tables, self._unigram_tables = [], []
        self.files = validate_args(bpe_tables=self._bpe_tables,
                                   unigram_tables=self._unigram_tables, **kw)
        self._kw = kw
        self._epoch = kw['start_epoch']
        self._ctx = None

    def _setup(self):
        from types import SimpleNamespace
        from .. import punkt
        from ..bpe import BpeContext
        from ..context import ASSETS, Context
        from ..dask.bert.corpus import punkt_params
        from . import span as span_mod
        from .utils import get_rank, get_world_size
        kw = self._kw
        self.rank, self.world = (get_rank(), get_world_size()) if kw['rank'] is None else \
            (kw['rank'], kw['world'])
        if self._unigram_tables:  # the tokenizer's context, whichever of the two it is
            from ..unigram import UnigramContext, load_normalizer
            p, sc, ty, unk, ws = self._unigram_tables
            keys, repls, byte_pieces = load_normalizer(kw['unigram'])
            self.bpe = UnigramContext.from_tables(p, sc, ty, unk, ws, byte_pieces=byte_pieces,
                                                  normalizer=(keys, repls) if keys else None)
        else:
            self.bpe = BpeContext.from_tables(self._bpe_tables[0], self._bpe_tables[2],
                                              vocab=self._bpe_tables[1], **self._bpe_tables[3])
        # Punkt's tables live in a Context of the packaged WordPiece vocabulary, which here only
        # segments (as in the BART loader with bpe=)
        self._ctx = Context(os.path.join(ASSETS, 'vocab_synth_uncased_30522.txt'))
        pp = kw['punkt_params']
        if pp is None or isinstance(pp, str):
            pp = punkt_params(SimpleNamespace(punkt_params=pp))
        punkt.set_params(self._ctx, pp)
        self._span = span_mod.parse(kw['span'])
        self.seed = mix_seed(kw['base_seed'], self.rank)

    def rounds(self):
        """This rank's files (files[rank::world]) in runs of at most round_bytes, one at least."""
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

    def plan_round(self, files):
        """One round on the device: the token table, its block plan and n_blocks (the round's
        one sync). A line of a file is a document."""
        import torch
        from .. import punkt
        docs = []
        for f in files:
            with open(f, 'rb') as fh:
                docs += [ln for ln in fh.read().split(b'\n') if ln.strip()]
        dev = self._ctx.device
        text = torch.from_numpy(np.frombuffer(b''.join(docs) or b' ', np.uint8).copy()).to(dev)
        doc_off = np.zeros(len(docs) + 1, np.int64)
        np.cumsum([len(d) for d in docs], out=doc_off[1:])
        sent_off, doc_sent_off = punkt.segment(self._ctx, text, torch.from_numpy(doc_off).to(dev))
        if getattr(self.bpe, 'rules', 0):  # a unigram model's normaliser: the text it tokenizes
            text, sent_off = self.bpe.normalize(text, sent_off)
        ids, sent_len = self.bpe.tokenize(text, sent_off, doc_sent_off, self._kw['max_pieces'])
        table = (ids, sent_off, sent_len, doc_sent_off)
        plan, n = roberta_blocks(table, self.plan_seq_len(), self._kw['mode'])
        return table, plan, n

    def plan_seq_len(self):
        """The seq_len the round's blocks are cut for; with `collate`, what a subclass replaces
        (the T5 loader of t5.py)."""
        return self._kw['max_seq_length']

    def order(self, epoch, rnd, n):
        """The seeded shuffle of a round's n blocks."""
        return np.random.Generator(np.random.PCG64(mix_seed(
            self._kw['base_seed'], epoch, self.rank, rnd))).permutation(n).astype(np.int64)

    def collate(self, table, plan, rows, epoch, step):
        kw = self._kw
        return collate_blocks(self.bpe, table, plan, rows,
                              mask=(kw['mlm_probability'], self.seed, (epoch << 32) | step),
                              whole_word=kw['whole_word_masking'], span=self._span,
                              ignore_index=kw['ignore_index'], special_ids=kw['special_ids'])

    def __iter__(self):
        if self._ctx is None:
            self._setup()
        epoch = self._epoch
        self._epoch += 1
        return self._run_epoch(epoch)

    def _run_epoch(self, epoch):
        import torch
        bs, step = self._kw['batch_size'], 0
        for rnd, files in enumerate(self.rounds()):
            table, plan, n = self.plan_round(files)
            perm = torch.from_numpy(self.order(epoch, rnd, n)).to(self._ctx.device)
            for r0 in range(0, n, bs):
                if n - r0 < bs and self._kw['drop_last']:
                    break
                with torch.no_grad():
                    yield self.collate(table, plan, perm[r0:r0 + bs], epoch, step)
                step += 1


def get_roberta_pretrain_data_loader(path, bpe=None, batch_size=None, max_seq_length=512,
                                     mode='full', mlm_probability=0.15, whole_word_masking=False,
                                     span=None, ignore_index=-100, base_seed=12345, start_epoch=0,
                                     rank=None, world=None, drop_last=False, round_bytes=32 << 20,
                                     max_pieces=512, punkt_params=None, special_ids=None,
                                     unigram=None):
    """RoBERTa pretraining batches from the text files (*.txt, one document per line) under
    `path` (past the reference, which has no RoBERTa loader). One process, one
    stream, no DataLoader workers: a round of files (at most round_bytes; this rank's are
    files[rank::world]) goes to the device as one buffer, through punkt.segment,
    BpeContext.tokenize of bpe=(vocab_json, merges_txt) and roberta_blocks (mode='full':
    FULL-SENTENCES, 'doc': DOC-SENTENCES); n_blocks is the round's one sync; a seeded
    permutation cuts the blocks into batches, and each step is one collate_blocks call with
    counter = (epoch << 32) | step. Yields dicts of int64 [batch, max_seq_length] input_ids,
    attention_mask and labels; the specials are the vocabulary's <s>, </s>, <pad> and <mask>
    (special_ids overrides them). unigram=model_file in place of bpe=: the sentences are
    tokenized by the SentencePiece unigram model of an XLM-R / T5 checkpoint
    (`lddl_amd.unigram.UnigramContext`); exactly one of the two is given. The
    ranks do not agree on a number of steps."""
    return RobertaPretrainLoader(**dict(locals()))
