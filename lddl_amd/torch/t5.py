"""T5 span corruption on the device (past the reference): exactly N noise tokens in
exactly k spans per row, written as the encoder input and the target with matching sentinels.
`t5_corrupt` writes rows from the blocks of `roberta_blocks` (lddl_t5_corrupt), `t5_lengths` and
`t5_tokens_length` give the fixed widths, and `get_t5_pretrain_data_loader` feeds them from text
files. include/lddl_amd.h states the semantics; the kernel is csrc/t5_corrupt.hip. Every
argument error is raised before the native library is imported.
"""
import math
import numbers

from .roberta import _M64, RobertaPretrainLoader, _mode, _seq_len

MAX_SPANS = 256  # LDDL_T5_MAX_SPANS
MAX_TOKENS = (1 << 24) - 2
SPECIAL_KEYS = {'eos_id', 'pad_id', 'sentinel_first', 'decoder_start_id'}


def _int(name, v, lo, hi):
    if not isinstance(v, int) or isinstance(v, bool) or not lo <= v <= hi:
        raise ValueError('{} must be an int in [{}, {}], not {!r}'.format(name, lo, hi, v))
    return v


def fixed_point(noise_density=0.15, mean_noise_span_length=3.0, n_sentinels=100):
    """The argument errors of the three noise knobs (ValueError) -> (dq, iq, n_sentinels): the
    density and the inverse of the mean span length in 16.16 fixed point, rounded half up. The
    device and the oracle count with these integers alone."""
    for name, v in (('noise_density', noise_density),
                    ('mean_noise_span_length', mean_noise_span_length)):
        if not isinstance(v, numbers.Real) or isinstance(v, bool) or not v > 0 or v != v:
            raise ValueError('{} must be a positive number, not {!r}'.format(name, v))
    dq = int(math.floor(noise_density * 65536 + 0.5))
    iq = int(math.floor(65536 / mean_noise_span_length + 0.5))
    if not 1 <= dq <= 65535:
        raise ValueError('noise_density {!r} is not inside (0, 1)'.format(noise_density))
    if not 1 <= iq <= 65536:
        raise ValueError('mean_noise_span_length {!r} is not in [1, 65536]'.format(
            mean_noise_span_length))
    return dq, iq, _int('n_sentinels', n_sentinels, 1, MAX_SPANS)


def _lengths(tokens, q):
    import ctypes
    from .._native import check, lib
    a, b = ctypes.c_int64(), ctypes.c_int64()
    check(lib.lddl_t5_lengths(tokens, *q, ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def t5_lengths(tokens, noise_density=0.15, mean_noise_span_length=3.0, n_sentinels=100):
    """(in_len, tgt_len) of a row of `tokens` tokens: tokens - N + k + 1 and N + k + 1 for its N
    noise tokens in k spans (lddl_t5_lengths). Both are non-decreasing in `tokens`, so they are
    the widths that no row of a plan with seq_len = tokens + 2 overflows."""
    q = fixed_point(noise_density, mean_noise_span_length, n_sentinels)
    return _lengths(_int('tokens', tokens, 1, MAX_TOKENS), q)


def t5_tokens_length(max_seq_length, noise_density=0.15, mean_noise_span_length=3.0,
                     n_sentinels=100):
    """The largest `tokens` whose in_len is at most max_seq_length (T5's
    compute_input_and_target_lengths turned round): the block length to plan with."""
    q = fixed_point(noise_density, mean_noise_span_length, n_sentinels)
    _int('max_seq_length', max_seq_length, 2, 1 << 24)  # in_len(1) = 2
    lo, hi = 1, MAX_TOKENS  # in_len(lo) <= max_seq_length throughout
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if _lengths(mid, q)[0] <= max_seq_length else (lo, mid - 1)
    return lo


def check_args(noise=(0, 0), noise_density=0.15, mean_noise_span_length=3.0, n_sentinels=100,
               in_len=None, tgt_len=None, special_ids=None):
    """The argument errors of t5_corrupt (ValueError) -> (dq, iq, n_sentinels, seed, counter)."""
    unknown = set(special_ids or ()) - SPECIAL_KEYS
    if unknown:
        raise ValueError('special_ids: unknown keys {}'.format(sorted(unknown)))
    try:
        seed, counter = noise
        seed, counter = int(seed) & _M64, int(counter) & _M64
    except (TypeError, ValueError):
        raise ValueError('noise must be (seed, counter), not {!r}'.format(noise)) from None
    for name, v in (('in_len', in_len), ('tgt_len', tgt_len)):
        if v is not None:
            _int(name, v, 1, 1 << 24)
    return fixed_point(noise_density, mean_noise_span_length, n_sentinels) + (seed, counter)


def t5_corrupt(bpe_or_ctx, table, plan, rows=None, noise=(0, 0), noise_density=0.15,
               mean_noise_span_length=3.0, n_sentinels=100, in_len=None, tgt_len=None,
               ignore_index=-100, special_ids=None):
    """Rows `rows` (int64 cuda tensor of block indices, None = every block, which reads
    n_blocks; the indices are the caller's to check) of a `roberta_blocks` plan under T5's span
    corruption: a row of n tokens (the block's pieces, </s> where the plan put a separator) has
    exactly N = round(n * noise_density) of them noised in exactly k = round(N /
    mean_noise_span_length) spans (at most n_sentinels), both segmentations drawn uniformly under
    noise=(seed, counter); equal pairs give equal rows. Returns a dict of int64 tensors:
    input_ids and attention_mask [B, in_len] (the clean segments, sentinel g behind segment g,
    </s>, <pad>), labels and decoder_input_ids [B, tgt_len] (sentinel g and the noise behind it,
    </s>, ignore_index; shifted right behind decoder_start_id), and src_lengths / tgt_lengths
    [B], untruncated. The widths default to t5_lengths(plan.seq_len - 2), which no row
    overflows. Sentinel g is sentinel_first - g; by default the sentinels sit above the
    vocabulary (sentinel_first = len(ctx) + n_sentinels - 1), and decoder_start_id is <pad>.
    special_ids: eos_id, pad_id, sentinel_first, decoder_start_id."""
    dq, iq, ns, seed, counter = check_args(noise, noise_density, mean_noise_span_length,
                                           n_sentinels, in_len, tgt_len, special_ids)
    import torch
    from .._native import check, lib
    from ..bpe import BpeContext
    from ..context import _ptr, _stream
    from ..unigram import UnigramContext
    ctx, sp = bpe_or_ctx, dict(special_ids or {})
    names = ('</s>', '<pad>') if isinstance(ctx, (BpeContext, UnigramContext)) else \
        ('[SEP]', '[PAD]')
    eos, pad = (int(sp[k]) if k in sp else ctx.special_ids.get(n, -1)
                for k, n in zip(('eos_id', 'pad_id'), names))
    if min(eos, pad) < 0:
        raise ValueError('the vocab lacks {} or {}: pass special_ids'.format(*names))
    first = int(sp.get('sentinel_first', len(ctx) + ns - 1))
    start = int(sp.get('decoder_start_id', pad))
    widths = _lengths(plan.seq_len - 2, (dq, iq, ns))
    in_len, tgt_len = (d if v is None else v for v, d in zip((in_len, tgt_len), widths))
    ids, sent_off = table[0], table[1]
    for t, dt in ((ids, torch.int32), (sent_off, torch.int64)) + \
            (() if rows is None else ((rows, torch.int64),)):
        assert t.dtype == dt and t.is_cuda and t.is_contiguous()
    B = int(plan.n_blocks.item()) if rows is None else rows.numel()
    new = lambda *shape: torch.empty(*shape, dtype=torch.long, device=ids.device)  # noqa: E731
    out = {'input_ids': new(B, in_len), 'attention_mask': new(B, in_len),
           'labels': new(B, tgt_len), 'decoder_input_ids': new(B, tgt_len),
           'src_lengths': new(B), 'tgt_lengths': new(B)}
    check(lib.lddl_t5_corrupt(_stream(), _ptr(ids), _ptr(sent_off), _ptr(plan.piece_off),
                              _ptr(plan.sent_sep), _ptr(plan.block_sent), _ptr(rows), B,
                              plan.seq_len, in_len, tgt_len, dq, iq, ns, first, eos, pad, start,
                              int(ignore_index), seed, counter, *[_ptr(v) for v in out.values()]))
    return out


class T5PretrainLoader(RobertaPretrainLoader):
    """RobertaPretrainLoader with the plan length of the noise knobs and t5_corrupt as its
    collate; each iter() is one epoch."""

    def __init__(self, **kw):
        self._noise = {k: kw[k] for k in ('noise_density', 'mean_noise_span_length',
                                          'n_sentinels')}
        self._special = kw['special_ids']
        check_args(special_ids=self._special, **self._noise)
        _mode(kw['mode'])
        _seq_len(kw['max_seq_length'])
        # the loader's own checks see no masking knobs and the vocabulary's specials
        super().__init__(**dict(kw, span=None, special_ids=None))
        self.tokens = t5_tokens_length(kw['max_seq_length'], **self._noise)
        self.in_len, self.tgt_len = t5_lengths(self.tokens, **self._noise)

    def plan_seq_len(self):
        return self.tokens + 2

    def collate(self, table, plan, rows, epoch, step):
        return t5_corrupt(self.bpe, table, plan, rows, noise=(self.seed, (epoch << 32) | step),
                          ignore_index=self._kw['ignore_index'], special_ids=self._special,
                          **self._noise)


def get_t5_pretrain_data_loader(path, bpe=None, batch_size=None, max_seq_length=512, mode='full',
                                noise_density=0.15, mean_noise_span_length=3.0, n_sentinels=100,
                                ignore_index=-100, base_seed=12345, start_epoch=0, rank=None,
                                world=None, drop_last=False, round_bytes=32 << 20, max_pieces=512,
                                punkt_params=None, special_ids=None, unigram=None):
    """T5 pretraining batches from the text files (*.txt, one document per line) under `path`
    (past the reference): get_roberta_pretrain_data_loader's rounds, tokenizer and
    block cut, with blocks of t5_tokens_length(max_seq_length) tokens, so that the encoder input
    of a full block is max_seq_length wide, and one t5_corrupt call per step with noise =
    (the rank's seed, (epoch << 32) | step). Yields t5_corrupt's dicts at the fixed widths
    t5_lengths gives for that block length: every batch of a run has the same two shapes.
    unigram=model_file in place of bpe=: the ids are those of a T5 checkpoint's spiece.model
    (DESIGN §32), and on its 32,000 pieces the default sentinels end at <extra_id_0> = 32099."""
    return T5PretrainLoader(**dict(locals()))
