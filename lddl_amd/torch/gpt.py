"""GPT input on the device (past the reference): rows for causal language modelling
cut from one endless stream doc, eos, doc, eos, ... of a tokenized round, with optional
document-level fill-in-the-middle (Bavarian et al. 2022). `stream_plan` lays the documents out
in the stream (lddl_stream_plan), `collate_stream` writes rows from it (lddl_stream_rows,
lddl_stream_cu_seqlens) and `get_gpt_pretrain_data_loader` feeds both from text files.
include/lddl_amd.h states the semantics; the kernels are csrc/stream_plan.hip and
csrc/stream_rows.hip. Every argument error is raised before the native library is imported.
"""
import math
import numbers

import numpy as np

from .online import mix_seed
from .roberta import _M64, RobertaPretrainLoader
from .roberta import validate_args as _roberta_args

TILE = 1024      # LDDL_STREAM_TILE
LDS_DOCS = 256   # LDDL_STREAM_LDS_DOCS
SPECIAL_KEYS = {'eos_id', 'fim_prefix_id', 'fim_middle_id', 'fim_suffix_id'}
FIM_NAMES = {'fim_prefix_id': '<fim_prefix>', 'fim_middle_id': '<fim_middle>',
             'fim_suffix_id': '<fim_suffix>'}


def _seq_len(seq_len):
    if not isinstance(seq_len, int) or isinstance(seq_len, bool) or not 1 <= seq_len <= 1 << 20:
        raise ValueError('seq_len must be an int in [1, 2^20], not {!r}'.format(seq_len))
    return seq_len


def _rate(name, v):
    if not isinstance(v, numbers.Real) or isinstance(v, bool) or not 0 <= v <= 1:
        raise ValueError('{} must be a number in [0, 1], not {!r}'.format(name, v))
    return int(math.floor(v * 65536 + 0.5))


def check_fim(fim):
    """The argument errors of fim= (ValueError) -> (fim_q, spm_q, seed, counter): the two rates
    in 16.16 fixed point, rounded half up. None is no transform."""
    if fim is None:
        return 0, 0, 0, 0
    try:
        rate, spm_rate, seed, counter = fim
        seed, counter = int(seed) & _M64, int(counter) & _M64
    except (TypeError, ValueError):
        raise ValueError('fim must be None or (rate, spm_rate, seed, counter), not '
                         '{!r}'.format(fim)) from None
    return _rate('fim: rate', rate), _rate('fim: spm_rate', spm_rate), seed, counter


def check_collate(ignore_index=-100, max_seqs=None, special_ids=None):
    """The argument errors of collate_stream that need no plan (ValueError)."""
    unknown = set(special_ids or ()) - SPECIAL_KEYS
    if unknown:
        raise ValueError('special_ids: unknown keys {}'.format(sorted(unknown)))
    for k, v in (special_ids or {}).items():
        if not isinstance(v, int) or isinstance(v, bool) or v < 0:
            raise ValueError('special_ids: {} must be a non-negative int, not {!r}'.format(k, v))
    if not isinstance(ignore_index, int) or isinstance(ignore_index, bool):
        raise ValueError('ignore_index must be an int, not {!r}'.format(ignore_index))
    if max_seqs is not None and (not isinstance(max_seqs, int) or isinstance(max_seqs, bool)
                                 or not 1 <= max_seqs < 1 << 31):
        raise ValueError('max_seqs must be None or an int in [1, 2^31), not {!r}'.format(max_seqs))


class StreamPlan:
    """lddl_stream_plan's outputs on the device: sent_tok_off int64 [n_sent + 1], doc_off int64
    [n_doc + 1], counts int64 [2] (n_rows, the stream's length); with the knobs the rows must
    repeat: seq_len, doc_order, fim = (fim_q, spm_q, seed, counter); n_rows as read."""
    __slots__ = ('sent_tok_off', 'doc_off', 'counts', 'seq_len', 'doc_order', 'fim', 'n_rows')

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def stream_plan(table, seq_len, doc_order=None, fim=None):
    """The stream of the token table (ids, sent_off, sent_len, doc_sent_off) of `ctx.tokenize` /
    `BpeContext.tokenize` at rows of seq_len slots: document doc_order[j] (an int64 cuda
    permutation; None = the table's order) at place j, each followed by its terminator;
    fim=(rate, spm_rate, seed, counter) applies the fill-in-the-middle transform to a share
    `rate` of the documents, `spm_rate` of those in the SPM layout, drawn per document id under
    (seed, counter). Returns (StreamPlan, n_rows); reading n_rows is the one device sync."""
    L, q = _seq_len(seq_len), check_fim(fim)
    import torch
    from .._native import check, lib
    from ..context import _ptr, _stream
    _, _, sent_len, doc_sent_off = table
    assert sent_len.dtype == torch.int32 and sent_len.is_cuda and sent_len.is_contiguous()
    assert doc_sent_off.dtype == torch.int64 and doc_sent_off.is_cuda and doc_sent_off.is_contiguous()
    n, n_doc, dev = sent_len.numel(), doc_sent_off.numel() - 1, doc_sent_off.device
    if doc_order is not None:
        assert doc_order.dtype == torch.int64 and doc_order.is_cuda and doc_order.is_contiguous()
        if doc_order.numel() != n_doc:
            raise ValueError('doc_order holds {} entries for {} documents'.format(
                doc_order.numel(), n_doc))
    plan = StreamPlan(sent_tok_off=torch.empty(n + 1, dtype=torch.int64, device=dev),
                      doc_off=torch.empty(n_doc + 1, dtype=torch.int64, device=dev),
                      counts=torch.empty(2, dtype=torch.int64, device=dev), seq_len=L,
                      doc_order=doc_order, fim=q, n_rows=0)
    check(lib.lddl_stream_plan(_stream(), _ptr(sent_len), n, _ptr(doc_sent_off), n_doc,
                               _ptr(doc_order), L, *q, _ptr(plan.sent_tok_off),
                               _ptr(plan.doc_off), _ptr(plan.counts)))
    plan.n_rows = int(plan.counts[0].item())
    return plan, plan.n_rows


def _vocab_id(ctx, name):
    """The id of a token string in a BpeContext, UnigramContext or Context, or -1."""
    v = getattr(ctx, 'special_ids', {}).get(name, -1)
    if v < 0 and isinstance(getattr(ctx, 'vocab', None), dict):
        v = ctx.vocab.get(name, -1)
    if v < 0 and name.encode() in getattr(ctx, 'pieces', ()):
        v = list(ctx.pieces).index(name.encode())
    return int(v)


def special_ids_of(ctx, special_ids, fim):
    """(eos, prefix, middle, suffix): special_ids first, then the vocabulary's <|endoftext|> or
    </s> (the larger id where it has both), and only where it has neither <|end_of_text|> (Llama
    3); <fim_prefix>, <fim_middle>, <fim_suffix>, the sentinels only when `fim`. A missing id is
    a ValueError naming it."""
    sp = dict(special_ids or {})
    eos = sp['eos_id'] if 'eos_id' in sp else max(_vocab_id(ctx, '<|endoftext|>'),
                                                   _vocab_id(ctx, '</s>'))
    if eos < 0 and 'eos_id' not in sp:
        eos = _vocab_id(ctx, '<|end_of_text|>')
    if eos < 0:
        raise ValueError('the vocab has neither <|endoftext|> nor </s>: pass special_ids '
                         'with eos_id')
    out = [eos]
    for k, name in FIM_NAMES.items():
        v = sp[k] if k in sp else (_vocab_id(ctx, name) if fim else 0)
        if v < 0:
            raise ValueError('the vocab lacks {}: pass special_ids with {}'.format(name, k))
        out.append(v)
    return tuple(out)


def collate_stream(bpe_or_ctx, table, plan, rows=None, eod_mask_loss=False,
                   reset_position_ids=True, ignore_index=-100, max_seqs=None, special_ids=None):
    """Rows `rows` (int64 cuda tensor of row indices below n_rows, None = every row) of the
    plan: dict of int64 [B, seq_len] input_ids (stream tokens r * L + y), labels (the next
    token; ignore_index behind a document's terminator with eod_mask_loss), position_ids
    (restarting behind a terminator unless reset_position_ids=False) and sequence_ids (the
    terminators before the slot in its row), and for variable-length attention cu_seqlens int32
    [max_seqs + 1] (the flat offset of every sequence start, then B * L) with n_seqs int32 [1],
    the untruncated count. max_seqs defaults to a bound that cannot overflow. The terminator is
    special_ids' eos_id, else the vocabulary's <|endoftext|>, else </s>; a plan with fim= needs
    fim_prefix_id, fim_middle_id and fim_suffix_id or the vocabulary's <fim_prefix>,
    <fim_middle>, <fim_suffix>."""
    check_collate(ignore_index, max_seqs, special_ids)
    eos, pre, mid, suf = special_ids_of(bpe_or_ctx, special_ids, plan.fim[0] > 0)
    import torch
    from .._native import check, lib
    from ..context import _ptr, _stream
    ids, sent_off, sent_len, doc_sent_off = table
    for t, dt in ((ids, torch.int32), (sent_off, torch.int64)) + \
            (() if rows is None else ((rows, torch.int64),)):
        assert t.dtype == dt and t.is_cuda and t.is_contiguous()
    L, n_doc, dev = plan.seq_len, doc_sent_off.numel() - 1, ids.device
    B = plan.n_rows if rows is None else rows.numel()
    if B * L >= 1 << 31:
        raise ValueError('{} rows of {} slots: the offsets of cu_seqlens are int32'.format(B, L))
    if max_seqs is None:  # a document starts once in the stream, so once per copy of a row
        max_seqs = max(1, min(B * L, B + n_doc * (1 if rows is None else B)))
    out = {k: torch.empty(B, L, dtype=torch.long, device=dev)
           for k in ('input_ids', 'labels', 'position_ids', 'sequence_ids')}
    check(lib.lddl_stream_rows(_stream(), _ptr(ids), _ptr(sent_off), sent_len.numel(),
                               _ptr(doc_sent_off), n_doc, _ptr(plan.doc_order),
                               _ptr(plan.sent_tok_off), _ptr(plan.doc_off), _ptr(rows), B, L,
                               *plan.fim, eos, pre, mid, suf, int(bool(eod_mask_loss)),
                               int(bool(reset_position_ids)), ignore_index,
                               *[_ptr(v) for v in out.values()]))
    out['cu_seqlens'] = torch.empty(max_seqs + 1, dtype=torch.int32, device=dev)
    out['n_seqs'] = torch.empty(1, dtype=torch.int32, device=dev)
    check(lib.lddl_stream_cu_seqlens(_stream(), _ptr(plan.doc_off), n_doc, _ptr(rows), B, L,
                                     max_seqs, _ptr(out['cu_seqlens']), _ptr(out['n_seqs'])))
    return out


# ---- the loader ------------------------------------------------------------------------------
def validate_args(max_seq_length=1024, fim_rate=0.0, fim_spm_rate=0.5, eod_mask_loss=False,
                  reset_position_ids=True, ignore_index=-100, special_ids=None, **kw):
    """Every argument error of get_gpt_pretrain_data_loader, raised before the GPU is touched.
    Returns the files."""
    _seq_len(max_seq_length)
    check_fim((fim_rate, fim_spm_rate, 0, 0))
    check_collate(ignore_index, None, special_ids)
    return _roberta_args(**dict(kw, max_seq_length=512, mode='full', span=None, special_ids=None,
                                whole_word_masking=False, mlm_probability=0.15))


class GptPretrainLoader(RobertaPretrainLoader):
    """RobertaPretrainLoader's rounds with a line as a document of one sentence, stream_plan as
    the plan and collate_stream as the collate; each iter() is one epoch."""

    def __init__(self, **kw):
        self._bpe_tables, self._unigram_tables = [], []
        self.files = validate_args(bpe_tables=self._bpe_tables,
                                   unigram_tables=self._unigram_tables, **kw)
        self._kw = kw
        self._epoch = kw['start_epoch']
        self._ctx = None

    def _setup(self):
        from ..bpe import BpeContext
        from .utils import get_rank, get_world_size
        kw = self._kw
        self.rank, self.world = (get_rank(), get_world_size()) if kw['rank'] is None else \
            (kw['rank'], kw['world'])
        if self._unigram_tables:
            from ..unigram import UnigramContext, load_normalizer
            p, sc, ty, unk, ws = self._unigram_tables
            keys, repls, byte_pieces = load_normalizer(kw['unigram'])
            self.bpe = UnigramContext.from_tables(p, sc, ty, unk, ws, byte_pieces=byte_pieces,
                                                  normalizer=(keys, repls) if keys else None)
        else:
            self.bpe = BpeContext.from_tables(self._bpe_tables[0], self._bpe_tables[2],
                                              vocab=self._bpe_tables[1], **self._bpe_tables[3])
        self._ctx = self.bpe  # no Punkt pass: the tokenizer's context is the device's owner
        self.seed = mix_seed(kw['base_seed'], self.rank)
        special_ids_of(self.bpe, kw['special_ids'], kw['fim_rate'] > 0)  # missing ids, up front

    def tokenize_round(self, files):
        """The round's token table: a line is a document and one sentence, kept whole
        (max_pieces is the longest document's byte count)."""
        import torch
        docs = []
        for f in files:
            with open(f, 'rb') as fh:
                docs += [ln for ln in fh.read().split(b'\n') if ln.strip()]
        dev = self.bpe.device
        text = torch.from_numpy(np.frombuffer(b''.join(docs) or b' ', np.uint8).copy()).to(dev)
        off = np.zeros(len(docs) + 1, np.int64)
        np.cumsum([len(d) for d in docs], out=off[1:])
        sent_off = torch.from_numpy(off).to(dev)
        doc_sent_off = torch.arange(len(docs) + 1, dtype=torch.int64, device=dev)
        if getattr(self.bpe, 'rules', 0):  # a unigram model's normaliser: the text it tokenizes
            text, sent_off = self.bpe.normalize(text, sent_off)
        ids, sent_len = self.bpe.tokenize(text, sent_off, doc_sent_off,
                                          max(map(len, docs), default=1))
        return ids, sent_off, sent_len, doc_sent_off

    def doc_order(self, epoch, rnd, n_doc):
        """The seeded shuffle of a round's documents, None with shuffle_docs=False."""
        if not self._kw['shuffle_docs']:
            return None
        return np.random.Generator(np.random.PCG64(mix_seed(
            self._kw['base_seed'], epoch, self.rank, rnd, 1))).permutation(n_doc).astype(np.int64)

    def plan_round(self, files, epoch=0, rnd=0, table=None):
        """One round of one epoch on the device: the token table, its stream plan and n_rows
        (the round's one sync). The FIM counter is the epoch."""
        import torch
        table = self.tokenize_round(files) if table is None else table
        order = self.doc_order(epoch, rnd, table[3].numel() - 1)
        kw = self._kw
        plan, n = stream_plan(
            table, kw['max_seq_length'],
            None if order is None else torch.from_numpy(order).to(self.bpe.device),
            (kw['fim_rate'], kw['fim_spm_rate'], self.seed, epoch) if kw['fim_rate'] > 0 else None)
        return table, plan, n

    def collate(self, table, plan, rows, epoch, step):
        kw = self._kw
        return collate_stream(self.bpe, table, plan, rows, kw['eod_mask_loss'],
                              kw['reset_position_ids'], kw['ignore_index'],
                              special_ids=kw['special_ids'])

    def _run_epoch(self, epoch):
        import torch
        bs, step = self._kw['batch_size'], 0
        for rnd, files in enumerate(self.rounds()):
            table, plan, n = self.plan_round(files, epoch, rnd)
            perm = torch.from_numpy(self.order(epoch, rnd, n)).to(self.bpe.device)
            for r0 in range(0, n, bs):
                if n - r0 < bs and self._kw['drop_last']:
                    break
                with torch.no_grad():
                    yield self.collate(table, plan, perm[r0:r0 + bs], epoch, step)
                step += 1


def get_gpt_pretrain_data_loader(path, bpe=None, unigram=None, batch_size=None,
                                 max_seq_length=1024, fim_rate=0.0, fim_spm_rate=0.5,
                                 eod_mask_loss=False, reset_position_ids=True, ignore_index=-100,
                                 shuffle_docs=True, base_seed=12345, start_epoch=0, rank=None,
                                 world=None, drop_last=False, round_bytes=32 << 20,
                                 special_ids=None):
    """GPT pretraining batches from the text files (*.txt, one document per line) under `path`
    (past the reference, which has no GPT loader). get_roberta_pretrain_data_loader's
    rounds and ranks; a line is a document of one sentence (no Punkt pass), tokenized whole by
    BpeContext.tokenize of bpe=(vocab_json, merges_txt), of that pair and a dict of BpeContext's
    pattern / digit_group / ignore_merges, or of bpe=tokenizer_json (Llama 3, GPT-4, Qwen2:
    DESIGN §35), or by the unigram model of unigram=model_file, so its ids are `encode(line)`
    (as are, with bpe=, those of the RoBERTa, T5 and BART loaders). Per epoch and round a seeded permutation
    orders the documents in the stream (shuffle_docs=False keeps the files' order), stream_plan
    packs them across rows of max_seq_length slots with fim=(fim_rate, fim_spm_rate, the rank's
    seed, epoch), n_rows is the round's one sync, a second seeded permutation cuts the rows into
    batches, and each step is one collate_stream call. Yields its dicts: int64 [batch,
    max_seq_length] input_ids, labels, position_ids, sequence_ids, and cu_seqlens / n_seqs.
    special_ids: eos_id, fim_prefix_id, fim_middle_id, fim_suffix_id in place of the
    vocabulary's. The ranks do not agree on a number of steps."""
    return GptPretrainLoader(**dict(locals()))
