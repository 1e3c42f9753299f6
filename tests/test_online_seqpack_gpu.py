"""The packed online loader. The collate from a pair table with the plan made on the
device (collate_pairs_seqpacked over plan_rows_device) against the unpacked collate_pairs of
the same rows with seq_len = draw_stride: sample i's segment is bit for bit row i, the rest is
the padding the header specifies, the per-sample outputs are in packed order (assert_packed,
which recomputes the plan with seqpack.plan_rows). Then the loader: step k's batch is step k's
batch of the unpacked online loader, rearranged."""
import numpy as np
import pytest
import torch

from conftest import VOCAB_UNCASED
from test_online_loader_gpu import BASE, _epoch, _make, _write_corpus, src  # noqa: F401
from test_seqpack_gpu import assert_packed

pytestmark = pytest.mark.gpu

IGN = -1
SEED, COUNTER = 0x1234_5678_9ABC, (3 << 32) | 7
MASK = (0.15, SEED, COUNTER)
MODES = ['plain', 'static', 'fused', 'whole_word']


@pytest.fixture(scope='module')
def ctx():
    from lddl_amd.context import Context
    return Context(VOCAB_UNCASED)


@pytest.fixture(scope='module')
def ids(ctx):
    """(ids of whole words, ids of '##' pieces) of the vocab."""
    toks = ctx.tokens
    words = [i for i in range(1000, 6000) if not toks[i].startswith(('[', '##'))]
    cont = [i for i, t in enumerate(toks) if t.startswith('##') and len(t) > 2][:500]
    return np.array(words), np.array(cont)


def _sample(rng, words, n, nsl=None, na=None):
    """A pair of n slots (n - 3 made-up ids): (A ids, B ids, is_random_next)."""
    na = int(rng.integers(1, n - 3)) if na is None else na
    t = words[rng.integers(0, len(words), n - 3)]
    return [t[:na], t[na:], bool(rng.integers(0, 2)) if nsl is None else nsl]


def _with_static(rng, words, s, positions=None):
    n = len(s[0]) + len(s[1]) + 3
    if positions is None:
        positions = np.sort(rng.choice(n, min(n, int(rng.integers(0, 6))), replace=False))
    positions = np.asarray(positions, np.int64)
    return s[:3] + [positions, words[rng.integers(0, len(words), len(positions))]]


def _pair_batch(ctx, samples):
    """The PairBatch of hand-made samples (static masking iff they carry positions)."""
    from lddl_amd.pairs import PairBatch
    dt = np.int16 if ctx.id_bytes == 2 else np.int32
    cat = lambda xs, d: torch.from_numpy(  # noqa: E731
        np.concatenate([np.asarray(x, np.int64) for x in xs] + [np.zeros(0, np.int64)])
        .astype(d)).cuda()
    off = lambda ns: torch.from_numpy(  # noqa: E731
        np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)).cuda()
    args = [cat([np.concatenate([s[0], s[1]]) for s in samples], dt),
            off([len(s[0]) + len(s[1]) for s in samples]),
            torch.tensor([len(s[0]) for s in samples], dtype=torch.int32).cuda(),
            torch.tensor([int(s[2]) for s in samples], dtype=torch.uint8).cuda()]
    if len(samples[0]) > 3:  # uint16 positions in int16 storage
        args += [cat([s[3] for s in samples], np.int16), cat([s[4] for s in samples], dt),
                 off([len(s[3]) for s in samples])]
    return PairBatch(*args)


def _scatter(rng, ctx, words, samples, static):
    """A table three times as large with `samples` scattered over it; returns (pb, rows)."""
    n = len(samples)
    size = 3 * n + 2
    pick = rng.permutation(size)[:n]
    table = [_sample(rng, words, int(rng.integers(5, 60))) for _ in range(size)]
    if static:
        table = [_with_static(rng, words, s) for s in table]
    for r, s in zip(pick, samples):
        table[r] = s
    return _pair_batch(ctx, table), torch.from_numpy(pick.astype(np.int64)).cuda()


def both(ctx, pb, rows, L, mode, mask=MASK, ignore=IGN):
    """rows of pb through collate_pairs and, planned on the device, collate_pairs_seqpacked."""
    from lddl_amd.torch.online import collate_pairs, collate_pairs_seqpacked, plan_rows_device
    kw = dict(mask=mask, whole_word=mode == 'whole_word') if mode in ('fused', 'whole_word') \
        else {}
    ntok = pb.num_tokens if rows is None else pb.num_tokens[rows]
    lens = ntok.tolist()
    nsl = (pb.is_random_next if rows is None else pb.is_random_next[rows]).cpu().numpy()
    stride = (max(lens) - 1) // 8 * 8 + 8
    unp = collate_pairs(ctx, pb, rows, 8, ignore, seq_len=stride, **kw)
    plan = plan_rows_device(ctx, pb, rows, [0, len(lens)], L)
    got = collate_pairs_seqpacked(ctx, pb, rows, plan, 0, None, L, stride, ignore, **kw)
    assert ('labels' in got) == (mode != 'plain')
    return assert_packed(got, unp, lens, nsl.astype(np.int64), L, ignore), got, unp


def _batch(rng, ctx, words, lengths, mode):
    samples = [_sample(rng, words, n) for n in lengths]
    if mode == 'static':
        samples = [_with_static(rng, words, s) for s in samples]
    return _scatter(rng, ctx, words, samples, mode == 'static')


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('B', [1, 5, 7, 9])
def test_partly_filled_blocks(ctx, ids, mode, B):
    """B samples of 8 .. 127 slots, scattered over a larger table, into rows of 128."""
    rng = np.random.default_rng(B)
    pb, rows = _batch(rng, ctx, ids[0], rng.integers(8, 128, B), mode)
    plan, got, _ = both(ctx, pb, rows, 128, mode)
    assert plan.R <= B
    if mode != 'plain' and B > 1:
        assert int((got['labels'] != IGN).sum()) > 0


@pytest.mark.parametrize('mode', MODES)
def test_lengths_around_half_a_row(ctx, ids, mode):
    """Capacity 128, lengths 64, 65, 128, 64, 65, 64: a full row of one sample, two rows of a 65
    with 63 slots of tail, a row of two halves without a tail, a row of 64 with a tail of
    exactly one window."""
    rng = np.random.default_rng(3)
    pb, rows = _batch(rng, ctx, ids[0], [64, 65, 128, 64, 65, 64], mode)
    plan, _, _ = both(ctx, pb, rows, 128, mode)
    assert plan.R == 5
    assert plan.fill.tolist() == [64, 128, 128, 64, 128, 128]
    assert plan.start.tolist() == [0, 0, 0, 64, 0, 0]


def edge_samples(rng, words, cont):
    """Five samples of at most 70 slots that put the layout's edges on the edge of a 64-slot
    window, and the (sample, slot) of every '##' piece that is the first token of its A or B:
      0  na = 62: the first [SEP] on slot 63, B begins on slot 64; 70 slots
      1  na = 63: the first [SEP] on slot 64; 70 slots
      2  64 slots: the last [SEP] on slot 63
      3  65 slots: the last [SEP] on slot 64
      4  na = nb = 1: the smallest pair, 5 slots
    A and B of 0, 1 and 4 and A of 2 begin with a '##' piece. Directly behind [CLS] / [SEP] it
    continues nothing: it is a word head. The one behind it is a word of its own."""
    w = lambda k: words[rng.integers(0, len(words), k)]  # noqa: E731
    c = lambda: cont[rng.integers(0, len(cont), 1)]  # noqa: E731
    samples = [[np.concatenate([c(), w(61)]), np.concatenate([c(), w(4)]), True],
               [np.concatenate([c(), w(62)]), np.concatenate([c(), w(3)]), False],
               [np.concatenate([c(), w(29)]), w(31), False],
               [w(40), w(22), True],
               [c(), c(), False]]
    heads = [(0, 1), (0, 64), (1, 1), (1, 65), (2, 1), (4, 1), (4, 3)]
    return samples, heads


@pytest.mark.parametrize('mode', MODES)
def test_separators_and_pieces_on_the_window_edge(ctx, ids, mode):
    """edge_samples (B = 5: a partly filled block) into rows of 128, unpacked against packed."""
    rng = np.random.default_rng(11)
    words, cont = ids
    samples, heads = edge_samples(rng, words, cont)
    assert [len(s[0]) + len(s[1]) + 3 for s in samples] == [70, 70, 64, 65, 5]
    assert [len(s[0]) for s in samples[:2]] == [62, 63]
    if mode == 'static':  # labels on the slots beside and on the separators' neighbours
        at = [[1, 62, 64, 68], [1, 63, 65], [1, 62], [63], [1, 3]]
        samples = [_with_static(rng, words, s, p) for s, p in zip(samples, at)]
    pb, rows = _scatter(rng, ctx, words, samples, mode == 'static')
    both(ctx, pb, rows, 128, mode)
    if mode != 'whole_word':
        return
    # a head's decision is its own draw: on these slots whole-word equals per-token masking
    seen = set()
    for counter in range(COUNTER, COUNTER + 4):
        m = (0.5, SEED, counter)
        ww = both(ctx, pb, rows, 128, 'whole_word', m)[2]['labels'].cpu().numpy()
        tok = both(ctx, pb, rows, 128, 'fused', m)[2]['labels'].cpu().numpy()
        for i, x in heads:
            assert ww[i, x] == tok[i, x], (counter, i, x)
            seen.add(bool(ww[i, x] != IGN))
    assert seen == {True, False}


def test_identity_rows_and_unaligned_capacity(ctx, ids):
    """rows=None over a table of its own, and a capacity that is no multiple of 8 or 64."""
    rng = np.random.default_rng(8)
    pb = _pair_batch(ctx, [_sample(rng, ids[0], n) for n in (30, 99, 5, 61, 40, 17)])
    for mode in ('plain', 'fused', 'whole_word'):
        both(ctx, pb, None, 101, mode)


def test_whole_word_straddles_a_window_at_an_offset(ctx, ids):
    """Rows of 256: a sample of 140 slots, behind it one of 100 whose slots 62 .. 66 are one word
    (a head and four '##' pieces over the sample's window boundary 63 / 64; row slots 202 ..
    206, the sample starts at slot 140), and a third whose slot 1 is a '##' piece (a head:
    nothing continues across samples)."""
    rng = np.random.default_rng(9)
    words, cont = ids
    c = lambda k: cont[rng.integers(0, len(cont), k)]  # noqa: E731
    a = words[rng.integers(0, len(words), 80)]  # slots 1 .. 80
    a[62:66] = c(4)                             # slots 63 .. 66 continue slot 62
    b = words[rng.integers(0, len(words), 17)]
    third = [np.concatenate([c(2), words[5:6], c(1)]), words[7:8], False]
    samples = [[a, b, True], _sample(rng, words, 140), third, _sample(rng, words, 140),
               [a.copy(), b.copy(), False]]
    pb, rows = _scatter(rng, ctx, words, samples, False)
    for counter in range(COUNTER, COUNTER + 4):
        plan, _, _ = both(ctx, pb, rows, 256, 'whole_word', (0.15, SEED, counter))
    assert plan.start.tolist() == [140, 0, 240, 0, 140] and plan.row.tolist() == [0, 0, 0, 1, 1]
    # the case holds what it is meant to: whole-word differs from per-token on this batch
    plain = both(ctx, pb, rows, 256, 'fused', (0.5, SEED, COUNTER))[1]
    ww = both(ctx, pb, rows, 256, 'whole_word', (0.5, SEED, COUNTER))[1]
    lab = ww['labels'][0, 140 + 62:140 + 67].cpu().numpy() != IGN
    assert lab.all() or not lab.any()
    assert not torch.equal(plain['labels'], ww['labels'])


def test_static_position_on_the_last_slot_is_kept(ctx, ids):
    rng = np.random.default_rng(4)
    w = ids[0]
    s = [_sample(rng, w, n) for n in (20, 30, 10)]
    samples = [_with_static(rng, w, s[0], [3, 19]), _with_static(rng, w, s[1], [1, 29]),
               _with_static(rng, w, s[2], [9])]
    pb = _pair_batch(ctx, samples)
    plan, got, _ = both(ctx, pb, None, 64, 'static')
    assert plan.R == 1 and plan.start.tolist() == [30, 0, 50]
    lab = got['labels'].cpu().numpy()[0]
    want = {30 + 3: samples[0][4][0], 30 + 19: samples[0][4][1], 1: samples[1][4][0],
            29: samples[1][4][1], 50 + 9: samples[2][4][0]}
    assert {int(x): int(lab[x]) for x in np.flatnonzero(lab != IGN)} == want


def test_host_checks(ctx, ids):
    """What the string path refuses: a static position at its own sample's length (inside the
    unpacked row, accepted there; in a packed row it is the next sample's [CLS]), a row outside
    the table, a pair longer than a row, a plan for another capacity."""
    from lddl_amd.torch.online import collate_pairs, collate_pairs_seqpacked, plan_rows_device
    rng = np.random.default_rng(4)
    w = ids[0]
    s = [_sample(rng, w, n) for n in (30, 20)]
    pb = _pair_batch(ctx, [_with_static(rng, w, s[0], [1]), _with_static(rng, w, s[1], [3, 20])])
    collate_pairs(ctx, pb, None, seq_len=32)
    plan = plan_rows_device(ctx, pb, None, [0, 2], 64)
    with pytest.raises(IndexError, match='20'):
        collate_pairs_seqpacked(ctx, pb, None, plan, 0, None, 64, 32)
    first = torch.tensor([0], device='cuda')
    plan1 = plan_rows_device(ctx, pb, first, [0, 1], 64)  # the other sample alone: fine
    out = collate_pairs_seqpacked(ctx, pb, first, plan1, 0, None, 64, 32)
    assert out['input_ids'].shape == (1, 64)
    for bad in ([0, 2], [-1, 1]):
        rows = torch.tensor(bad, device='cuda')
        p = plan_rows_device(ctx, pb, rows, [0, 2], 64)  # clamped on the device: reads the table
        with pytest.raises(IndexError, match='the table has'):
            collate_pairs_seqpacked(ctx, pb, rows, p, 0, None, 64, 32)
    short = plan_rows_device(ctx, pb, first, [0, 1], 16)
    assert short.dst.tolist() == [-1] and short.num_rows.tolist() == [0]
    with pytest.raises(ValueError, match='does not fit'):
        collate_pairs_seqpacked(ctx, pb, first, short, 0, None, 16, 32)
    with pytest.raises(ValueError, match='64'):
        collate_pairs_seqpacked(ctx, pb, first, plan1, 0, None, 128, 32)
    with pytest.raises(ValueError, match='rows'):  # R that is not the plan's
        collate_pairs_seqpacked(ctx, pb, first, plan1, 0, 2, 64, 32)
    # an empty batch: empty tensors of the asked width
    empty = plan_rows_device(ctx, pb, torch.zeros(0, dtype=torch.int64, device='cuda'), [0, 0], 64)
    e = collate_pairs_seqpacked(ctx, pb, torch.zeros(0, dtype=torch.int64, device='cuda'), empty,
                                0, None, 64, 8)
    assert e['input_ids'].shape == (0, 64) and e['seq_lens'].shape == (0,)


@pytest.mark.parametrize('mode', ['static', 'fused'])
def test_ignore_index_reaches_the_padding(ctx, ids, mode):
    rng = np.random.default_rng(12)
    pb, rows = _batch(rng, ctx, ids[0], [20, 90, 33, 70, 12], mode)
    _, got, _ = both(ctx, pb, rows, 128, mode, ignore=-100)
    lab, att = got['labels'].cpu().numpy(), got['attention_mask'].cpu().numpy()
    assert (att == 0).any() and (lab[att == 0] == -100).all() and not (lab == -1).any()


def test_four_byte_ids(tmp_path, ids):
    """A vocab of more than 65,534 lines: 4-byte ids in the table (lddl_ctx_id_bytes)."""
    from lddl_amd.context import Context
    with open(VOCAB_UNCASED) as f:
        lines = f.read().splitlines()
    big = tmp_path / 'vocab_big.txt'
    big.write_text('\n'.join(lines + ['[extra{}]'.format(i) for i in range(40000)]) + '\n')
    wide = Context(str(big))
    assert wide.id_bytes == 4
    rng = np.random.default_rng(13)
    words = np.concatenate([ids[0], np.arange(len(lines), len(lines) + 40000)])  # above 65,535 too
    for mode in MODES:
        pb, rows = _batch(rng, wide, words, [64, 9, 128, 77, 64, 30, 5, 101, 64], mode)
        assert pb.tokens.dtype == torch.int32
        _, got, _ = both(wide, pb, rows, 128, mode)
        assert int(got['input_ids'].max()) > 65535
    from lddl_amd.torch.online import collate_pairs_seqpacked, plan_rows_device
    narrow = Context(VOCAB_UNCASED)
    with pytest.raises(ValueError, match='4-byte'):
        collate_pairs_seqpacked(narrow, pb, rows, plan_rows_device(narrow, pb, rows, [0, 9], 128),
                                0, None, 128, 128)


def test_abi_refusals(ctx, ids):
    """-1 before anything is launched: NULL context, table array, plan array or required output,
    static inputs in part, rows too long for the static LDS slab; batch <= 0 returns 0."""
    from lddl_amd._native import lib
    from lddl_amd.context import _ptr, _stream
    rng = np.random.default_rng(14)
    w = ids[0]
    pb = _pair_batch(ctx, [_with_static(rng, w, _sample(rng, w, n), [1]) for n in (10, 6)])
    o = [torch.full((1, 16), 77, dtype=torch.long, device='cuda') for _ in range(6)]
    per = [torch.full((2,), 77, dtype=torch.long, device='cuda') for _ in range(2)]
    lens = torch.full((2,), 77, dtype=torch.int32, device='cuda')
    tab = [_ptr(pb.tokens), _ptr(pb.tok_off), _ptr(pb.len_a), _ptr(pb.is_random_next)]
    st = [_ptr(pb.pos), _ptr(pb.labels), _ptr(pb.pos_off)]
    held = [torch.tensor([0, 10], device='cuda')] + [
        torch.tensor(x, dtype=torch.int32, device='cuda') for x in ([10, 6], [1, 2], [0, 1])]
    plan = [_ptr(t) for t in held]  # dst, fill, seq_in_row, packed_idx
    rowo = [_ptr(t) for t in o]  # input_ids, token_type_ids, attention_mask, labels, pos, seq
    samp = [_ptr(per[0]), _ptr(per[1]), _ptr(lens)]

    def plain(c=ctx.handle, tab=tab, st=st, plan=plan, n=2, L=16, stm=None, rowo=rowo, samp=samp):
        return lib.lddl_collate_pairs_seqpack(c, _stream(), *tab, *st, None, n, *plan, 1, L,
                                              *rowo[:3], stm, rowo[3], *rowo[4:], *samp, -1)

    def masked(c=ctx.handle, tab=tab, plan=plan, n=2, rowo=rowo, samp=samp, ww=0):
        return lib.lddl_collate_pairs_seqpack_masked(c, _stream(), *tab, None, n, *plan, 1, 16,
                                                     16, *rowo, *samp, 0.15, -1, len(ctx), 1, 2,
                                                     ww)

    def without(xs, k):
        return xs[:k] + [None] + xs[k + 1:]
    for f in (plain, masked):
        assert f(c=None) == -1
        assert b'null ctx' in lib.lddl_last_error()
        for k in range(4):
            assert f(tab=without(tab, k)) == -1
            assert b'null pair table' in lib.lddl_last_error()
            assert f(plan=without(plan, k)) == -1
            assert b'null plan' in lib.lddl_last_error()
        for k in range(6):
            assert f(rowo=without(rowo, k)) == -1
            assert b'null output' in lib.lddl_last_error()
        for k in range(3):
            assert f(samp=without(samp, k)) == -1
            assert b'null output' in lib.lddl_last_error()
        assert f(n=0) == 0 and f(n=-3) == 0
    for k in range(3):  # static inputs in part
        assert plain(st=without(st, k)) == -1
    assert plain(st=[None] * 3) == -1  # unmasked: special_tokens_mask is required
    assert b'null output' in lib.lddl_last_error()
    assert plain(L=1 << 14) == -1
    assert b'too long' in lib.lddl_last_error()
    torch.cuda.synchronize()
    assert all(int((t != 77).sum()) == 0 for t in o + per + [lens])  # nothing was launched


# ---- the loader -------------------------------------------------------------------------------
def _make_packed(src, **kw):
    from lddl_amd.torch import get_bert_pretrain_online_packed_data_loader
    args = dict(BASE, books=src, rank=0, world=1)
    args.update(kw)
    return get_bert_pretrain_online_packed_data_loader(128, **args)


MASKING = {'dynamic': dict(), 'whole_word': dict(whole_word_masking=True),
           'static': dict(static_masking=True)}


@pytest.mark.parametrize('drop_last', [False, True])
@pytest.mark.parametrize('bin_size', [None, 32], ids=['unbinned', 'binned'])
@pytest.mark.parametrize('masking', list(MASKING))
def test_loader_yields_the_unpacked_loaders_batches_rearranged(src, masking, bin_size, drop_last):
    """Several rounds and a batch size that leaves short flush batches (drop_last off) or
    dropped samples (on): batch k of the packed loader is batch k of the unpacked one."""
    kw = dict(batch_size=37, gpu_batch_bytes=100_000, bin_size=bin_size, drop_last=drop_last,
              ignore_index=-100, **MASKING[masking])
    plain = _make(src, **kw)
    unpacked = _epoch(plain)
    packed = _make_packed(src, **kw)
    rows = samples = 0
    steps = 0
    for got, unp in zip(packed, unpacked):
        lens = unp['attention_mask'].sum(1).tolist()
        plan = assert_packed(got, unp, lens, unp['next_sentence_labels'].numpy(), 128, -100)
        rows += plan.R
        samples += len(lens)
        steps += 1
    assert steps == len(unpacked) > 8
    assert packed.dropped_samples == plain.dropped_samples
    assert packed.dropped_per_bin.tolist() == plain.dropped_per_bin.tolist()
    assert packed.num_rounds == plain.num_rounds >= 3
    assert (plain.dropped_samples > 0) == drop_last
    if not drop_last:
        assert any(len(u['next_sentence_labels']) < 37 for u in unpacked)  # short flush batches
    assert rows < samples  # samples did share rows
    assert sum(int((u['labels'] != -100).sum()) for u in unpacked) > 100


def test_packed_loader_is_deterministic_and_rows_may_be_longer(src):
    kw = dict(batch_size=32, gpu_batch_bytes=150_000, bin_size=None)
    a, b = _epoch(_make_packed(src, **kw)), _epoch(_make_packed(src, **kw))
    assert len(a) == len(b) > 8
    for x, y in zip(a, b):
        assert set(x) == set(y) and all(torch.equal(x[k], y[k]) for k in x)
    # rows of 256 slots for pairs of at most 128 tokens: fewer rows, the same samples
    from lddl_amd.torch import get_bert_pretrain_online_packed_data_loader
    wide = _epoch(get_bert_pretrain_online_packed_data_loader(
        256, **dict(BASE, books=src, rank=0, world=1, **kw)))
    assert len(wide) == len(a)
    for x, y in zip(wide, a):
        assert x['input_ids'].shape[1] == 256 and x['input_ids'].shape[0] <= y['input_ids'].shape[0]
        assert sorted(x['seq_lens'].tolist()) == sorted(y['seq_lens'].tolist())
