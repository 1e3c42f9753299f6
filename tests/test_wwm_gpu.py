"""Whole-word dynamic masking against an expectation built from the plain entry
points, which draw the same Philox stream:

* plain at p = 0.15: `labels != ignore` is every slot's own u01(r.x) < p;
* plain at p = 1.0: every non-special slot is masked, so `input_ids` shows each slot's own
  80 / 10 / 10 outcome and random id;
* head(x) on the host, in numpy, from the vocab lines;

then masked = own[head] & ~special, out = where(masked, out_p1, ids), labels = where(masked, ids,
ignore), and the whole-word run at p = 0.15 with the same seed and counter must equal these bit
for bit."""
import logging
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, VOCAB_CASED, VOCAB_UNCASED
from loader_data import make_loader_dataset

pytestmark = pytest.mark.gpu

IGN = -1
SEED, COUNTER = 1234567, (3 << 32) + 5


@pytest.fixture(scope='module')
def ctx_u():
    from lddl_amd.context import Context
    return Context(VOCAB_UNCASED, True)


@pytest.fixture(scope='module')
def ctx_c():
    from lddl_amd.context import Context
    return Context(VOCAB_CASED, False)


def cont_ids(ctx):
    """[vocab] bool: the vocab line starts with '##' and is longer than 2 bytes."""
    return np.array([t.startswith('##') and len(t.encode('utf-8')) > 2 for t in ctx.tokens])


def heads(ids, special, ctx):
    """ids, special: [B, L] numpy. Returns (cont [B, L] bool, head [B, L] index)."""
    cv = cont_ids(ctx)
    V = len(cv)
    ok = (ids >= 0) & (ids < V)
    idc = np.zeros(ids.shape, bool)
    idc[ok] = cv[ids[ok]]
    prev_sp = np.ones_like(special)  # slot 0 has no slot before it
    prev_sp[:, 1:] = special[:, :-1]
    cont = ~special & ~prev_sp & idc
    x = np.broadcast_to(np.arange(ids.shape[1]), ids.shape)
    return cont, np.maximum.accumulate(np.where(cont, 0, x), axis=1)


def special_from_ids(ids, ctx):
    return np.isin(ids, [i for i in ctx.special_ids.values() if i >= 0])


def expectation(ids, stm, ctx, seed=SEED, counter=COUNTER):
    """ids: [B, L] cuda long; stm: the special_tokens_mask tensor given to _mask_tokens or None.
    Returns numpy (exp_out, exp_labels, exp_masked, cont, special) from two plain runs."""
    from lddl_amd.torch.bert import _mask_tokens
    _, lab015 = _mask_tokens(ids.clone(), stm, ctx, 0.15, IGN, seed=seed, counter=counter)
    out_p1, _ = _mask_tokens(ids.clone(), stm, ctx, 1.0, IGN, seed=seed, counter=counter)
    h_ids = ids.cpu().numpy()
    special = special_from_ids(h_ids, ctx) if stm is None else stm.cpu().numpy() != 0
    cont, head = heads(h_ids, special, ctx)
    own = lab015.cpu().numpy() != IGN
    masked = np.take_along_axis(own, head, axis=1) & ~special
    return (np.where(masked, out_p1.cpu().numpy(), h_ids), np.where(masked, h_ids, IGN), masked,
            cont, special)


def assert_whole_words(masked, cont):
    """Inside every word `masked` is constant: a continuation equals the slot before it."""
    assert (masked[:, 1:][cont[:, 1:]] == masked[:, :-1][cont[:, 1:]]).all()


# ---- hand-built rows --------------------------------------------------------------------------
def hand_rows(ctx):
    """[5, 192] and [1, 72] ids with their special_tokens_mask (numpy int64)."""
    cv = cont_ids(ctx)
    V = len(ctx)
    sp = ctx.special_ids
    cls, sep, unk = sp['[CLS]'], sp['[SEP]'], sp['[UNK]']
    W = np.array([i for i in range(1000, V) if not cv[i] and not ctx.tokens[i].startswith('[')])
    C = np.flatnonzero(cv)
    rng = np.random.default_rng(11)
    w = lambda n=None: rng.choice(W, n)  # noqa: E731
    c = lambda n=None: rng.choice(C, n)  # noqa: E731
    L = 192
    ids = np.zeros((5, L), np.int64)
    stm = np.zeros((5, L), np.int64)
    # row 0: a word over slots 62-66; '##x' right after the middle [SEP]; [UNK] between pieces;
    # ids >= len(ctx) between pieces
    r = ids[0]
    r[:150] = w(150)
    r[0], r[100], r[150] = cls, sep, sep
    r[63:67] = c(4)
    r[101:104] = c(3)
    r[110:114] = [w(), c(), unk, c()]
    r[120:125] = [w(), c(), V + 5, c(), V]
    stm[0, [0, 100]] = 1
    stm[0, 150:] = 1
    # row 1: a head in window 0 followed by 70 continuations (over two window boundaries)
    r = ids[1]
    r[:180] = w(180)
    r[0], r[140], r[180] = cls, sep, sep
    r[61:131] = c(70)
    stm[1, [0, 140]] = 1
    stm[1, 180:] = 1
    # row 2: nothing but continuation ids after [CLS] ('##x' right after [CLS] is a head)
    ids[2, 0] = cls
    ids[2, 1:] = c(L - 1)
    stm[2, 0] = 1
    # row 3: special slots (given mask only) inside would-be words, also at the window boundary
    r = ids[3]
    r[:191] = w(191)
    r[0], r[96], r[191] = cls, sep, sep
    r[11:16] = c(5)
    r[60:70] = c(10)
    r[126:131] = c(5)
    stm[3, [0, 96, 191]] = 1
    stm[3, [12, 63, 64, 128]] = 1
    # row 4: a random mix, half of the ids continuations
    r = ids[4]
    r[:170] = np.where(rng.random(170) < 0.5, c(170), w(170))
    r[0], r[77], r[170] = cls, sep, sep
    stm[4, [0, 77]] = 1
    stm[4, 170:] = 1
    # [1, 72]: one full window and a tail of 8; a word over slots 62-66
    ids1 = np.zeros((1, 72), np.int64)
    stm1 = np.zeros((1, 72), np.int64)
    r = ids1[0]
    r[:70] = np.where(rng.random(70) < 0.4, c(70), w(70))
    r[62] = w()
    r[63:67] = c(4)
    r[67] = w()
    r[0], r[30], r[70] = cls, sep, sep
    stm1[0, [0, 30, 70, 71]] = 1
    return [(ids, stm), (ids1, stm1)]


@pytest.fixture(scope='module')
def hand(ctx_u):
    """Per shape and per way of deriving the special slots: ids, the mask given, the expectation."""
    out = {}
    for ids, stm in hand_rows(ctx_u):
        d_ids = torch.from_numpy(ids).cuda()
        for given in (True, False):
            d_stm = torch.from_numpy(stm).cuda() if given else None
            out[ids.shape, given] = (d_ids, d_stm, expectation(d_ids, d_stm, ctx_u))
    return out


def test_hand_rows_hold_the_edge_cases(hand):
    """The fixture's rows contain what they are meant to (checked on the host expectation)."""
    _, _, (_, _, _, cont, special) = hand[(5, 192), True]
    assert cont[0, 63:67].all() and not cont[0, 62] and not cont[0, 67]   # word over 62-66
    assert not cont[0, 101] and cont[0, 102:104].all()                   # '##x' after [SEP]
    assert not cont[0, 112] and cont[0, 113]       # [UNK] is a head; the piece after continues
    assert not cont[0, 122] and not cont[0, 124] and cont[0, 123]        # ids >= len(ctx)
    assert cont[1, 61:131].all() and not cont[1, 60]
    assert not cont[2, 1] and cont[2, 2:].all()
    assert cont[3, 11] and not cont[3, 12] and not cont[3, 13] and cont[3, 14]
    assert not cont[3, 63] and not cont[3, 64] and not cont[3, 65] and cont[3, 66]
    assert not cont[3, 128] and not cont[3, 129] and cont[3, 130]
    _, _, (_, _, _, cont_n, special_n) = hand[(5, 192), False]
    assert special_n[0, 112] and not cont_n[0, 113]  # by id [UNK] is special: the next is a head
    assert cont_n[3, 12] and cont_n[3, 64]           # no given mask: these stay inside the word


@pytest.mark.parametrize('shape', [(5, 192), (1, 72)])
@pytest.mark.parametrize('given', [True, False], ids=['stm', 'stm_none'])
def test_hand_rows_standalone(ctx_u, hand, shape, given):
    from lddl_amd.torch.bert import _mask_tokens
    ids, stm, (exp_out, exp_lab, exp_masked, cont, special) = hand[shape, given]
    out, lab = _mask_tokens(ids.clone(), stm, ctx_u, 0.15, IGN, seed=SEED, counter=COUNTER,
                            whole_word=True)
    np.testing.assert_array_equal(lab.cpu().numpy(), exp_lab)
    np.testing.assert_array_equal(out.cpu().numpy(), exp_out)
    assert_whole_words(exp_masked, cont)
    assert exp_masked.any() and not (exp_masked & special).any()


# ---- the golden dynamic batch -----------------------------------------------------------------
@pytest.fixture(scope='module')
def dyn_batch(ctx_c):
    from lddl_amd.torch.bert import PackedBatch
    with np.load(os.path.join(GOLDEN, 'collate.npz')) as z:
        g = dict(z)

    def strings(flat, off):
        return [' '.join(ctx_c.tokens[i] for i in flat[off[k]:off[k + 1]])
                for k in range(len(off) - 1)]
    A = strings(g['dyn_a'], g['dyn_a_off'])
    B = strings(g['dyn_b'], g['dyn_b_off'])
    return PackedBatch([(a, b, bool(r)) for a, b, r in zip(A, B, g['dyn_is_random_next'])])


@pytest.fixture(scope='module')
def golden_ww(ctx_c, dyn_batch):
    """Per alignment: the unmasked collate, its expectation, and the fused whole-word collate."""
    from lddl_amd.torch.bert import encode_packed
    out = {}
    for align in (8, 1, 64):
        enc = encode_packed(dyn_batch, ctx_c, align)
        exp = expectation(enc['input_ids'], enc['special_tokens_mask'], ctx_c)
        one = encode_packed(dyn_batch, ctx_c, align, mask=(0.15, SEED, COUNTER), whole_word=True)
        out[align] = (enc, exp, one)
    return out


@pytest.mark.parametrize('align', [8, 1, 64])
def test_fused_equals_two_pass(ctx_c, golden_ww, align):
    from lddl_amd.torch.bert import _mask_tokens
    enc, (exp_out, exp_lab, exp_masked, cont, special), one = golden_ww[align]
    ids, lab = _mask_tokens(enc['input_ids'].clone(), enc['special_tokens_mask'], ctx_c, 0.15, IGN,
                            seed=SEED, counter=COUNTER, whole_word=True)
    assert set(one) == {'input_ids', 'token_type_ids', 'attention_mask', 'labels',
                        'next_sentence_labels'}
    assert torch.equal(one['input_ids'], ids) and torch.equal(one['labels'], lab)
    for k in ('token_type_ids', 'attention_mask', 'next_sentence_labels'):
        assert torch.equal(one[k], enc[k]), k
    np.testing.assert_array_equal(one['labels'].cpu().numpy(), exp_lab)
    np.testing.assert_array_equal(one['input_ids'].cpu().numpy(), exp_out)
    assert cont.sum() > 1000 and exp_masked.any()


def test_properties_on_golden_batch(ctx_c, dyn_batch, golden_ww):
    from lddl_amd.torch.bert import encode_packed
    enc, (_, _, _, cont, special), one = golden_ww[8]
    ids = enc['input_ids'].cpu().numpy()
    out, lab = one['input_ids'].cpu().numpy(), one['labels'].cpu().numpy()
    masked = lab != IGN
    assert_whole_words(masked, cont)
    assert (masked[:, 1:] & cont[:, 1:]).any()               # whole words of several pieces exist
    assert (out[~masked] == ids[~masked]).all()              # unmasked slots untouched
    assert (lab[masked] == ids[masked]).all()
    assert not (masked & special).any()
    again = encode_packed(dyn_batch, ctx_c, 8, mask=(0.15, SEED, COUNTER), whole_word=True)
    other = encode_packed(dyn_batch, ctx_c, 8, mask=(0.15, SEED, COUNTER + 1), whole_word=True)
    assert torch.equal(again['input_ids'], one['input_ids'])
    assert torch.equal(again['labels'], one['labels'])
    assert not torch.equal(other['labels'], one['labels'])


def test_rows_without_continuations_equal_plain(ctx_u):
    """No continuation id in the batch: whole-word output is the plain output, on both paths."""
    from lddl_amd.torch.bert import PackedBatch, _mask_tokens, encode_packed
    cv = cont_ids(ctx_u)
    W = [i for i in range(1000, len(ctx_u)) if not cv[i] and not ctx_u.tokens[i].startswith('[')]
    rng = np.random.default_rng(5)
    batch = []
    for _ in range(6):
        na, nb = rng.integers(1, 90, 2)
        batch.append((' '.join(ctx_u.tokens[i] for i in rng.choice(W, na)),
                      ' '.join(ctx_u.tokens[i] for i in rng.choice(W, nb)), False))
    pk = PackedBatch(batch)
    plain = encode_packed(pk, ctx_u, 8, mask=(0.15, SEED, COUNTER))
    ww = encode_packed(pk, ctx_u, 8, mask=(0.15, SEED, COUNTER), whole_word=True)
    for k in plain:
        assert torch.equal(plain[k], ww[k]), k
    enc = encode_packed(pk, ctx_u, 8)
    assert not cv[enc['input_ids'].cpu().numpy()].any()
    for stm in (enc['special_tokens_mask'], None):
        a = _mask_tokens(enc['input_ids'].clone(), stm, ctx_u, 0.15, IGN, seed=SEED, counter=7)
        b = _mask_tokens(enc['input_ids'].clone(), stm, ctx_u, 0.15, IGN, seed=SEED, counter=7,
                         whole_word=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert bool((a[1] != IGN).any())


# ---- refusals ---------------------------------------------------------------------------------
def test_whole_word_with_replay_raises(ctx_u):
    from lddl_amd.torch.bert import _mask_tokens
    ids = torch.full((2, 8), 1500, dtype=torch.long, device='cuda')
    z = torch.zeros(2, 8, dtype=torch.uint8)
    rep = dict(masked=z, replaced=z, random=z, words=torch.zeros(2, 8, dtype=torch.long))
    with pytest.raises(ValueError, match='whole_word'):
        _mask_tokens(ids.clone(), None, ctx_u, replay=rep, whole_word=True)
    assert bool((ids == 1500).all())


def test_entry_points_refuse_null_context():
    from lddl_amd._native import lib
    assert lib.lddl_mask_dynamic_ww(None, None, None, None, None, None, None, 1, 8, 0.15, IGN,
                                    100, 1, 2) == -1
    assert b'null ctx' in lib.lddl_last_error()
    assert lib.lddl_collate_encode_masked_ww(None, None, None, None, None, None, None, 1, 8, None,
                                             None, None, None, 0.15, IGN, 100, 1, 2) == -1
    assert b'null ctx' in lib.lddl_last_error()


# ---- loaders ----------------------------------------------------------------------------------
DL_KWARGS = {'batch_size': 4, 'num_workers': 2}


def _stop_workers(dl):
    for gl in getattr(dl, '_dataloaders', [dl]):
        it = gl._loader._iterator
        if it is not None:
            it._shutdown_workers()


def _assert_batch_whole_words(batch, cv, sp):
    """The original ids are the labels where masked and the input_ids elsewhere."""
    lab = batch['labels'].cpu().numpy()
    masked = lab != IGN
    orig = np.where(masked, lab, batch['input_ids'].cpu().numpy())
    special = (orig == sp['[CLS]']) | (orig == sp['[SEP]']) | \
        (batch['attention_mask'].cpu().numpy() == 0)
    prev_sp = np.ones_like(special)
    prev_sp[:, 1:] = special[:, :-1]
    cont = ~special & ~prev_sp & cv[orig]
    assert_whole_words(masked, cont)
    assert not (masked & special).any()
    return int(cont.sum()), int((masked & cont).sum())


def test_loader_whole_word_masking(tmp_path, ctx_u):
    from lddl_amd.torch import get_bert_pretrain_data_loader
    d = str(tmp_path / 'dyn')
    make_loader_dataset(d, VOCAB_UNCASED, binned=True, static=False)
    dl = get_bert_pretrain_data_loader(
        d, vocab_file=VOCAB_UNCASED, data_loader_kwargs=dict(DL_KWARGS),
        log_level=logging.WARNING, whole_word_masking=True)
    cv = cont_ids(ctx_u)
    n = n_cont = n_masked_cont = 0
    for batch in dl:
        assert set(batch) == {'input_ids', 'token_type_ids', 'attention_mask', 'labels',
                              'next_sentence_labels'}
        a, b = _assert_batch_whole_words(batch, cv, ctx_u.special_ids)
        n_cont += a
        n_masked_cont += b
        n += batch['input_ids'].size(0)
    _stop_workers(dl)
    assert n == sum(len(x.dataset) for x in dl._dataloaders)
    assert n_cont > 100 and n_masked_cont > 0


def test_loader_refuses_static_dataset(tmp_path):
    from lddl_amd.torch import get_bert_pretrain_data_loader
    d = str(tmp_path / 'static')
    make_loader_dataset(d, VOCAB_UNCASED, binned=True, static=True)
    dl = get_bert_pretrain_data_loader(
        d, vocab_file=VOCAB_UNCASED, data_loader_kwargs=dict(DL_KWARGS),
        log_level=logging.WARNING, whole_word_masking=True)
    with pytest.raises(ValueError, match='whole_word_masking'):
        next(iter(dl))
    _stop_workers(dl)


def test_mp_loader_two_local_ranks_same_batches(tmp_path, ctx_u):
    """Two local ranks of one data-parallel group: the key is the group's, so the whole-word
    masks agree step by step."""
    from lddl_amd.torch_mp import get_bert_pretrain_data_loader
    d = str(tmp_path / 'dyn')
    make_loader_dataset(d, VOCAB_UNCASED, binned=True, static=False)
    cv = cont_ids(ctx_u)
    res = []
    for local_rank in (0, 1):
        dl = get_bert_pretrain_data_loader(
            d, local_rank=local_rank, dp_rank=0, vocab_file=VOCAB_UNCASED,
            data_loader_kwargs=dict(DL_KWARGS), log_level=logging.WARNING,
            whole_word_masking=True)
        steps = []
        for batch in dl:
            _assert_batch_whole_words(batch, cv, ctx_u.special_ids)
            steps.append({k: v.cpu().numpy() for k, v in batch.items()})
        _stop_workers(dl)
        res.append(steps)
    assert len(res[0]) == len(res[1]) > 0
    masked = 0
    for a, b in zip(*res):
        assert set(a) == set(b)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        masked += int((a['labels'] != IGN).sum())
    assert masked > 0
