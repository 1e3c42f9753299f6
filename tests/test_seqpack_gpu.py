"""The sequence-packed collate against the unpacked collate on the same batch with
the same (seed, counter): sample i's segment of its row is bit for bit row i of `encode_packed`,
the rest of every [R, L] tensor is the padding the header specifies, and the per-sample outputs
are the host arrays in packed order. The row plan is recomputed here from the lengths."""
import logging
import os
from io import BytesIO

import numpy as np
import pytest
import torch

from conftest import GOLDEN, VOCAB_CASED, VOCAB_UNCASED
from loader_data import make_loader_dataset
from test_collate_gpu import batch_dyn, batch_static

pytestmark = pytest.mark.gpu

IGN = -1
SEED, COUNTER = 1234567, (3 << 32) + 5
MASK = (0.15, SEED, COUNTER)
ROW_KEYS = ('input_ids', 'token_type_ids', 'attention_mask', 'position_ids', 'sequence_ids')
SAMPLE_KEYS = ('next_sentence_labels', 'cls_positions', 'seq_lens')


@pytest.fixture(scope='module')
def g():
    with np.load(os.path.join(GOLDEN, 'collate.npz')) as z:
        return dict(z)


@pytest.fixture(scope='module')
def ctx_c():
    from lddl_amd.context import Context
    return Context(VOCAB_CASED, False)


@pytest.fixture(scope='module')
def ctx_u():
    from lddl_amd.context import Context
    return Context(VOCAB_UNCASED, True)


def expected(unp, lens, nsl, L, ignore=IGN):
    """The packed batch built on the host from the unpacked one (numpy dict) and the lengths."""
    from lddl_amd.torch.seqpack import plan_rows
    plan = plan_rows(lens, L)
    last = 'labels' if 'labels' in unp else 'special_tokens_mask'
    exp = {k: np.zeros((plan.R, L), np.int64) for k in ROW_KEYS}
    exp[last] = np.full((plan.R, L), ignore if last == 'labels' else 1, np.int64)
    for i, n in enumerate(lens):
        r, s = plan.row[i], plan.start[i]
        for k in ('input_ids', 'token_type_ids', 'attention_mask', last):
            exp[k][r, s:s + n] = unp[k][i, :n]
        exp['position_ids'][r, s:s + n] = np.arange(n)
        exp['sequence_ids'][r, s:s + n] = plan.seq_in_row[i]
    flat = plan.row.astype(np.int64) * L + plan.start
    exp['next_sentence_labels'] = np.asarray(nsl)[plan.order]
    exp['cls_positions'] = flat[plan.order]
    exp['seq_lens'] = np.asarray(lens, np.int32)[plan.order]
    return exp, plan


def assert_packed(got, unp, lens, nsl, L, ignore=IGN):
    unp = {k: v.cpu().numpy() for k, v in unp.items()}
    assert (unp['attention_mask'].sum(1) == lens).all()
    exp, plan = expected(unp, lens, nsl, L, ignore)
    assert set(got) == set(exp)
    for k in exp:
        assert got[k].is_cuda and tuple(got[k].shape) == exp[k].shape, k
        assert got[k].dtype == (torch.int32 if k == 'seq_lens' else torch.int64), k
        np.testing.assert_array_equal(got[k].cpu().numpy(), exp[k], err_msg=k)
    real = got['attention_mask'].cpu().numpy() == 1  # the NSP head's gather finds every [CLS]
    assert real.sum() == sum(lens)
    assert real.reshape(-1)[exp['cls_positions']].all()
    assert (got['position_ids'].cpu().numpy().reshape(-1)[exp['cls_positions']] == 0).all()
    return plan


def both(batch, ctx, L, align=8, mask=None, whole_word=False, ignore=IGN):
    """The batch through encode_packed and encode_seqpacked; returns the plan checked against."""
    from lddl_amd.torch.bert import PackedBatch, encode_packed, encode_seqpacked
    from lddl_amd.torch.seqpack import SeqPackedBatch
    pk = PackedBatch(batch)
    kw = dict(mask=mask, whole_word=whole_word) if mask is not None else {}
    unp = encode_packed(pk, ctx, align, ignore, **kw)
    got = encode_seqpacked(SeqPackedBatch(batch, L), ctx, L, align, ignore, **kw)
    lens = (pk.na + pk.nb + 3).tolist()
    return assert_packed(got, unp, lens, pk.nsl, L, ignore), got, unp


def _shortest(batch, n):
    lens = [len(s[0].split()) + len(s[1].split()) for s in batch]
    return [batch[i] for i in sorted(np.argsort(lens, kind='stable')[:n])]


# ---- the golden batches -----------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['fused', 'unmasked', 'whole_word'])
@pytest.mark.parametrize('align', [8, 64])
def test_golden_dynamic_batch(g, ctx_c, mode, align):
    """48 samples of 18 .. 512 tokens into rows of 512: 22 samples of 512 fill a row alone."""
    mask = None if mode == 'unmasked' else MASK
    plan, got, _ = both(batch_dyn(g, ctx_c), ctx_c, 512, align, mask, mode == 'whole_word')
    assert 22 < plan.R < 48 and plan.seq_in_row.max() > 2
    if mask is not None:
        assert int((got['labels'] != IGN).sum()) > 100


@pytest.mark.parametrize('mode', ['fused', 'unmasked', 'whole_word'])
@pytest.mark.parametrize('B', [1, 5, 7])
def test_partly_filled_blocks(g, ctx_c, mode, B):
    """The B shortest golden samples (18 .. 127 tokens) into rows of 128."""
    mask = None if mode == 'unmasked' else MASK
    plan, _, _ = both(_shortest(batch_dyn(g, ctx_c), B), ctx_c, 128, 8, mask, mode == 'whole_word')
    assert plan.R == {1: 1, 5: 2, 7: 4}[B]


def test_golden_static_batch(g, ctx_u):
    """40 static-masking samples of 33 .. 128 tokens into rows of 128."""
    plan, got, _ = both(batch_static(g, ctx_u), ctx_u, 128)
    assert plan.R < 40 and plan.start.max() > 0
    assert int((got['labels'] != IGN).sum()) > 100


def test_ignore_index_reaches_the_padding(g, ctx_c):
    both(_shortest(batch_dyn(g, ctx_c), 5), ctx_c, 128, mask=MASK, ignore=-100)


# ---- hand-made samples ------------------------------------------------------------------------
def _words(ctx):
    return [t for t in ctx.tokens[1000:6000] if not t.startswith('[') and not t.startswith('##')]


def _sample(rng, words, n, nsl=False):
    """A sample of n slots (n - 3 tokens)."""
    na = int(rng.integers(1, n - 3))
    pick = lambda k: ' '.join(words[j] for j in rng.integers(0, len(words), k))  # noqa: E731
    return (pick(na), pick(n - 3 - na), nsl)


@pytest.mark.parametrize('mode', ['fused', 'unmasked', 'whole_word'])
def test_lengths_around_half_a_row(ctx_u, mode):
    """Capacity 128, lengths 128, 65, 65, 64, 64, 64: one full row of one sample, two rows of one
    short sample each (63 slots of tail), one row of two halves without a tail, and a row of 64
    with a tail of exactly one window."""
    rng = np.random.default_rng(3)
    w = _words(ctx_u)
    batch = [_sample(rng, w, n, k % 2 == 0) for k, n in enumerate([64, 65, 128, 64, 65, 64])]
    mask = None if mode == 'unmasked' else MASK
    plan, _, _ = both(batch, ctx_u, 128, 8, mask, mode == 'whole_word')
    assert plan.R == 5
    assert plan.fill.tolist() == [64, 128, 128, 64, 128, 128]
    assert plan.start.tolist() == [0, 0, 0, 64, 0, 0]


def test_whole_word_straddles_a_window_at_an_offset(ctx_u):
    """Rows of 256: a sample of 140 slots, then one of 100 whose slots 62 .. 66 are one word (a
    head and four '##' pieces over the sample's window boundary 63 / 64, row slots 203 / 204),
    and a third sample behind it whose slot 1 is a '##' piece (a head: nothing continues across
    samples)."""
    rng = np.random.default_rng(9)
    w = _words(ctx_u)
    cont = [t for t in ctx_u.tokens if t.startswith('##') and len(t) > 2][:500]
    c = lambda: cont[int(rng.integers(0, len(cont)))]  # noqa: E731
    a = [w[j] for j in rng.integers(0, len(w), 80)]    # slots 1 .. 80
    a[61:66] = [a[61], c(), c(), c(), c()]             # slots 62 .. 66
    b = [w[j] for j in rng.integers(0, len(w), 17)]
    third = (' '.join([c(), c()] + [w[5], c()]), w[7], False)
    batch = [(' '.join(a), ' '.join(b), True), _sample(rng, w, 140), third,
             _sample(rng, w, 140), (' '.join(a), ' '.join(b), False)]
    for counter in range(COUNTER, COUNTER + 4):
        plan, got, unp = both(batch, ctx_u, 256, 8, (0.15, SEED, counter), True)
    assert plan.start.tolist() == [140, 0, 240, 0, 140] and plan.row.tolist() == [0, 0, 0, 1, 1]
    # the case holds what it is meant to: whole-word differs from plain on this batch
    plain = both(batch, ctx_u, 256, 8, (0.5, SEED, COUNTER), False)[1]
    ww = both(batch, ctx_u, 256, 8, (0.5, SEED, COUNTER), True)[1]
    lab = ww['labels'][0, 140 + 62:140 + 67].cpu().numpy() != IGN
    assert lab.all() or not lab.any()
    assert not torch.equal(plain['labels'], ww['labels'])


def _static(sample, positions, labels):
    bio = BytesIO()
    np.save(bio, np.asarray(positions, np.uint16))
    return (sample[0], sample[1], sample[2], bio.getvalue(), ' '.join(labels))


def test_static_position_on_the_last_slot_is_accepted(ctx_u):
    rng = np.random.default_rng(4)
    w = _words(ctx_u)
    s = [_sample(rng, w, n) for n in (20, 30, 10)]
    batch = [_static(s[0], [3, 19], [w[1], w[2]]), _static(s[1], [1, 29], [w[3], w[4]]),
             _static(s[2], [9], [w[5]])]
    plan, got, _ = both(batch, ctx_u, 64)
    assert plan.R == 1 and plan.start.tolist() == [30, 0, 50]
    lab = got['labels'].cpu().numpy()[0]
    want = {30 + 3: w[1], 30 + 19: w[2], 1: w[3], 29: w[4], 50 + 9: w[5]}
    assert {int(x): ctx_u.tokens[lab[x]] for x in np.flatnonzero(lab != IGN)} == want


def test_static_position_at_the_sample_length_raises(ctx_u):
    """Position 20 of a sample of 20 slots: inside the unpacked row (32 slots, accepted there),
    but in a packed row it is the next sample's [CLS]."""
    from lddl_amd.torch.bert import PackedBatch, encode_packed, encode_seqpacked
    from lddl_amd.torch.seqpack import SeqPackedBatch
    rng = np.random.default_rng(4)
    w = _words(ctx_u)
    s = [_sample(rng, w, n) for n in (30, 20)]
    batch = [_static(s[0], [1], [w[3]]), _static(s[1], [3, 20], [w[1], w[2]])]
    encode_packed(PackedBatch(batch), ctx_u)
    with pytest.raises(IndexError, match='20'):
        encode_seqpacked(SeqPackedBatch(batch, 64), ctx_u, 64)


def test_plan_for_another_capacity_is_refused(ctx_u):
    from lddl_amd.torch.bert import encode_seqpacked
    from lddl_amd.torch.seqpack import SeqPackedBatch
    w = _words(ctx_u)
    with pytest.raises(ValueError, match='64'):
        encode_seqpacked(SeqPackedBatch([(w[0], w[1], False)], 64), ctx_u, 128)


def test_entry_points_refuse(ctx_u):
    from lddl_amd._native import lib
    from lddl_amd.context import _ptr
    n = (None,)
    assert lib.lddl_collate_seqpack(*n * 7, 1, *n * 3, 128, *n * 9, IGN, *n * 2) == -1
    assert b'null ctx' in lib.lddl_last_error()
    assert lib.lddl_collate_seqpack_masked(*n * 7, 1, *n * 3, 128, 128, *n * 6, 0.15, IGN, 100, 1,
                                           2, 0) == -1
    assert b'null ctx' in lib.lddl_last_error()
    h = (ctx_u.handle,)
    assert lib.lddl_collate_seqpack(*h, *n * 6, 1, *n * 3, 128, *n * 9, IGN, *n * 2) == -1
    assert b'null output' in lib.lddl_last_error()
    assert lib.lddl_collate_seqpack_masked(*h, *n * 6, 1, *n * 3, 128, 128, *n * 6, 0.15, IGN, 100,
                                           1, 2, 1) == -1
    assert b'null output' in lib.lddl_last_error()
    # rows too long for the LDS staging: refused before anything is launched or read
    p = (_ptr(torch.zeros(8, dtype=torch.long, device='cuda')),)
    assert lib.lddl_collate_seqpack_masked(*h, None, *p * 5, 1, *p * 3, 1 << 14, 128, *p * 6, 0.15,
                                           IGN, 100, 1, 2, 0) == -1
    assert b'too long' in lib.lddl_last_error()
    assert lib.lddl_collate_seqpack(*h, None, *p * 5, 1, *p * 3, 1 << 14, *p * 4, *n * 5, IGN,
                                    *p * 2) == -1
    assert b'too long' in lib.lddl_last_error()


# ---- the loader -------------------------------------------------------------------------------
def _stop_workers(dl):
    for gl in getattr(dl, '_dataloaders', [dl]):
        it = gl._loader._iterator
        if it is not None:
            it._shutdown_workers()


@pytest.mark.parametrize('binned', [False, True], ids=['unbinned', 'binned'])
def test_loader_yields_the_unpacked_loaders_batches_rearranged(tmp_path, binned):
    from lddl_amd.torch import (get_bert_pretrain_data_loader,
                                get_bert_pretrain_packed_data_loader)
    d = str(tmp_path / 'dyn')
    make_loader_dataset(d, VOCAB_UNCASED, binned=binned, static=False)
    kw = dict(shuffle_buffer_size=8, shuffle_buffer_warmup_factor=2, vocab_file=VOCAB_UNCASED,
              data_loader_kwargs={'batch_size': 4, 'num_workers': 1}, base_seed=77,
              log_level=logging.WARNING)
    plain = get_bert_pretrain_data_loader(d, **kw)
    unpacked = [{k: v.cpu() for k, v in b.items()} for b in plain]
    _stop_workers(plain)
    dl = get_bert_pretrain_packed_data_loader(d, 128, **kw)
    stager = (dl._dataloaders[0] if binned else dl)._stager
    steps = rows = 0
    for got, unp in zip(dl, unpacked):  # Binned asserts sum(remaining) == 0 when it runs out
        lens = unp['attention_mask'].sum(1).tolist()
        plan = assert_packed(got, unp, lens, unp['next_sentence_labels'].numpy(), 128)
        steps += 1
        rows += plan.R
        if steps == 4:  # the ring's four slots have each been filled once
            warm = stager.allocations
    _stop_workers(dl)
    assert steps == len(unpacked) == len(dl) and steps > 8
    n = sum(len(x.dataset) for x in getattr(dl, '_dataloaders', [dl]))  # what the shards balance to
    assert sum(len(u['next_sentence_labels']) for u in unpacked) == n > 60
    assert stager.allocations == warm <= 4
    assert rows < n  # samples did share rows
