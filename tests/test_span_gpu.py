"""N-gram (span) dynamic masking against an expectation built from the plain entry
point, which draws the same Philox stream (span_oracle.expectation):

* plain at p = p_start: `labels != ignore` is every non-special slot's start decision;
* plain under the key seed ^ LDDL_SPAN_SEED_XOR at p = c_k: the slot's u01(r2.x) < c_k, hence
  its length;
* plain at p = 1: each slot's own 80 / 10 / 10 outcome and random id;
* numpy: the words and which of them a span covers.

The span run must equal where(masked, out_p1, ids), and the labels likewise, bit for bit. Every
fused entry point must equal its two-pass form."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, VOCAB_CASED, VOCAB_UNCASED
from span_oracle import IGN, assert_whole_words, expectation, hand_rows, spans

pytestmark = pytest.mark.gpu

SEED, COUNTER = 1234567, (3 << 32) + 5
ONE_HOT_16 = [0.0] * 15 + [1.0]
SPANS = {'n1': 1, 'n3': 3, 'onehot16': ONE_HOT_16}
PROBS = [0.0, 0.15, 0.5, 1.0]


@pytest.fixture(scope='module')
def ctx_u():
    from lddl_amd.context import Context
    return Context(VOCAB_UNCASED, True)


@pytest.fixture(scope='module')
def ctx_c():
    from lddl_amd.context import Context
    return Context(VOCAB_CASED, False)


@pytest.fixture(scope='module')
def parsed():
    from lddl_amd.torch import span as S
    return {k: S.parse(v) for k, v in SPANS.items()}


@pytest.fixture(scope='module')
def rows(ctx_u):
    return {shape: (torch.from_numpy(ids).cuda(), torch.from_numpy(stm).cuda())
            for shape, (ids, stm) in hand_rows(ctx_u).items()}


def _run(ids, stm, ctx, span, p, seed=SEED, counter=COUNTER):
    from lddl_amd.torch.bert import _mask_tokens
    out, lab = _mask_tokens(ids.clone(), stm, ctx, p, IGN, seed=seed, counter=counter, span=span)
    return out.cpu().numpy(), lab.cpu().numpy()


# ---- the ids-only kernel on the hand rows -------------------------------------------------------
@pytest.mark.parametrize('p', PROBS)
@pytest.mark.parametrize('name', list(SPANS))
def test_hand_rows(ctx_u, rows, parsed, name, p):
    span = parsed[name]
    assert set(rows) == {(5, 192), (1, 72), (3, 100), (9, 8)}
    for shape, (ids, stm) in rows.items():
        for given in (stm, None):
            e = expectation(ids, given, ctx_u, span, p, SEED, COUNTER)
            out, lab = _run(ids, given, ctx_u, span, p)
            np.testing.assert_array_equal(lab, e['labels'], err_msg=str(shape))
            np.testing.assert_array_equal(out, e['out'], err_msg=str(shape))
            assert_whole_words(e['masked'], e['cont'])
            assert not (e['masked'] & e['special']).any()
            if p == 0.0:
                assert not e['masked'].any()
            if p == 1.0:
                assert (e['masked'] == ~e['special']).all()
            if p == 0.5 and shape[1] > 8:
                assert e['masked'].any() and (~e['masked'] & ~e['special']).any()


def _edge_cases(e, stm):
    """Which of the five edge cases the expectation of the [5, 192] rows holds."""
    special, cont = e['special'], e['cont']
    sep_at = {0: 100, 1: 140, 3: 96, 4: 66}  # the middle [SEP] of the rows that have one
    found = set()
    for b, row in enumerate(spans(special, cont, e['start'], e['length'])):
        for k, (j, n, s0, s1, words) in enumerate(row):
            if s0 <= 63 and s1 >= 64:
                found.add('crosses 63 -> 64')
            if s0 <= 63 and s1 >= 128:
                found.add('crosses two window boundaries')
            if b in sep_at and s0 < sep_at[b] < s1:
                found.add('runs over [SEP] from A into B')
            if j + n > words:
                found.add('cut by the row end')
            if k + 1 < len(row) and row[k + 1][0] < j + n:
                found.add('two overlapping spans')
    return found


def test_edge_cases_at_a_counter_chosen_by_the_oracle(ctx_u, rows, parsed):
    """The counter is the first of a small fixed range at which the expectation alone (plain
    entry points and numpy) holds every edge case; the span run must reproduce it."""
    ids, stm = rows[(5, 192)]
    want = {'crosses 63 -> 64', 'crosses two window boundaries', 'runs over [SEP] from A into B',
            'cut by the row end', 'two overlapping spans'}
    span, p = parsed['n3'], 0.5
    seen = []
    for counter in range(100, 116):
        e = expectation(ids, stm, ctx_u, span, p, SEED, counter)
        seen.append(_edge_cases(e, stm))
        if seen[-1] == want:
            break
    assert seen[-1] == want, seen
    # the words of every span are masked, over the special slots between them too
    masked = e['masked']
    for b, row in enumerate(spans(e['special'], e['cont'], e['start'], e['length'])):
        for j, n, s0, s1, words in row:
            inside = ~e['special'][b, s0:s1 + 1]
            assert masked[b, s0:s1 + 1][inside].all()
    out, lab = _run(ids, stm, ctx_u, span, p, counter=counter)
    np.testing.assert_array_equal(lab, e['labels'])
    np.testing.assert_array_equal(out, e['out'])


@pytest.mark.parametrize('p', PROBS)
def test_n1_is_whole_word_masking_bit_for_bit(ctx_u, rows, parsed, p):
    from lddl_amd.torch.bert import _mask_tokens
    for shape, (ids, stm) in rows.items():
        for given in (stm, None):
            a = _mask_tokens(ids.clone(), given, ctx_u, p, IGN, seed=SEED, counter=COUNTER,
                             whole_word=True)
            b = _mask_tokens(ids.clone(), given, ctx_u, p, IGN, seed=SEED, counter=COUNTER,
                             span=parsed['n1'])
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), shape
            c = _mask_tokens(ids.clone(), given, ctx_u, p, IGN, seed=SEED, counter=COUNTER,
                             span=[1.0], whole_word=True)  # whole_word beside it changes nothing
            assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]), shape


def test_rows_without_continuations_at_n1_equal_plain(ctx_u, rows, parsed):
    from lddl_amd.torch.bert import _mask_tokens
    ids, stm = rows[(3, 100)]
    a = _mask_tokens(ids.clone(), stm, ctx_u, 0.15, IGN, seed=SEED, counter=COUNTER)
    b = _mask_tokens(ids.clone(), stm, ctx_u, 0.15, IGN, seed=SEED, counter=COUNTER,
                     span=parsed['n1'])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and bool((a[1] != IGN).any())


# ---- the string collate: fused against two passes -----------------------------------------------
@pytest.fixture(scope='module')
def dyn_samples(ctx_c):
    with np.load(os.path.join(GOLDEN, 'collate.npz')) as z:
        g = dict(z)

    def strings(flat, off):
        return [' '.join(ctx_c.tokens[i] for i in flat[off[k]:off[k + 1]])
                for k in range(len(off) - 1)]
    A = strings(g['dyn_a'], g['dyn_a_off'])
    B = strings(g['dyn_b'], g['dyn_b_off'])
    return [(a, b, bool(r)) for a, b, r in zip(A, B, g['dyn_is_random_next'])]


@pytest.mark.parametrize('name', list(SPANS))
@pytest.mark.parametrize('align', [8, 1, 64])
def test_string_collate_fused_equals_two_pass(ctx_c, dyn_samples, parsed, align, name):
    from lddl_amd.torch.bert import PackedBatch, _mask_tokens, encode_packed
    span = parsed[name]
    assert len(dyn_samples) >= 9
    n_masked = 0
    for B in (1, 5, 9):  # kEncWaves is 4: a block of one wave, blocks with a partly filled last
        pk = PackedBatch(dyn_samples[-B:])
        enc = encode_packed(pk, ctx_c, align)
        for p in (0.15, 0.5):
            one = encode_packed(pk, ctx_c, align, mask=(p, SEED, COUNTER), span=span)
            ids, lab = _mask_tokens(enc['input_ids'].clone(), enc['special_tokens_mask'], ctx_c, p,
                                    IGN, seed=SEED, counter=COUNTER, span=span)
            assert set(one) == {'input_ids', 'token_type_ids', 'attention_mask', 'labels',
                                'next_sentence_labels'}
            assert torch.equal(one['input_ids'], ids) and torch.equal(one['labels'], lab)
            for k in ('token_type_ids', 'attention_mask', 'next_sentence_labels'):
                assert torch.equal(one[k], enc[k]), k
            e = expectation(enc['input_ids'], enc['special_tokens_mask'], ctx_c, span, p, SEED,
                            COUNTER)
            np.testing.assert_array_equal(lab.cpu().numpy(), e['labels'])
            np.testing.assert_array_equal(ids.cpu().numpy(), e['out'])
            n_masked += int(e['masked'].sum())
    # (a batch of one row at p_start = 0.01 may hold no span: the count is over all of them)
    assert n_masked > 0 and e['cont'].sum() > 100


# ---- the pair-table kernels ---------------------------------------------------------------------
def _ascii_ids(ctx):
    toks = ctx.tokens
    words = np.array([i for i in range(1000, 6000) if toks[i].isascii() and toks[i].isalpha()])
    cont = np.array([i for i, t in enumerate(toks)
                     if t.startswith('##') and t.isascii() and t[2:].isalnum()][:500])
    return words, cont


def _samples(rng, words, cont, B):
    """B hand-made pairs of up to 150 slots, a third of the ids '##' pieces; the first is 150
    slots with its middle [SEP] on slot 64, the rest have random shapes."""
    out = []
    for i in range(B):
        n = 150 if i == 0 else int(rng.integers(5, 150))
        na = 63 if i == 0 else int(rng.integers(1, n - 3))
        t = np.where(rng.random(n - 3) < 0.33, cont[rng.integers(0, len(cont), n - 3)],
                     words[rng.integers(0, len(words), n - 3)])
        out.append([t[:na], t[na:], bool(rng.integers(0, 2))])
    return out


def _tuples(ctx, pb):
    from lddl_amd import output
    rd = output.render(ctx, pb, None)
    return [(d['A'], d['B'], d['is_random_next']) for d in (rd.row(r) for r in range(rd.n))]


def _check_pairs(ctx, parsed):
    from lddl_amd.torch.bert import PackedBatch, encode_packed
    from lddl_amd.torch.online import collate_pairs, collate_pairs_seqpacked, plan_rows_device
    from test_online_seqpack_gpu import _pair_batch
    from test_seqpack_gpu import assert_packed
    words, cont = _ascii_ids(ctx)
    rng = np.random.default_rng(21)
    n_masked = 0
    for B in (1, 5, 9):
        pb = _pair_batch(ctx, _samples(rng, words, cont, B))
        pk = PackedBatch(_tuples(ctx, pb))
        for name, p in (('n3', 0.15), ('n3', 0.5), ('onehot16', 0.15), ('n1', 0.5)):
            span, mask = parsed[name], (p, SEED, COUNTER)
            ref = encode_packed(pk, ctx, 8, IGN, mask=mask, span=span)  # the string kernel
            got = collate_pairs(ctx, pb, None, 8, IGN, mask=mask, span=span)
            assert set(got) == set(ref)
            for k in ref:
                assert torch.equal(got[k], ref[k]), (B, name, k)
            n_masked += int((got['labels'] != IGN).sum())
            # packed: sample i's segment is row i of the unpacked output (draw_stride = its width)
            lens = pb.num_tokens.tolist()
            stride = ref['input_ids'].shape[1]
            for L in (160, 256):
                plan = plan_rows_device(ctx, pb, None, [0, B], L)
                packed = collate_pairs_seqpacked(ctx, pb, None, plan, 0, None, L, stride, IGN,
                                                 mask=mask, span=span)
                assert_packed(packed, got, lens, pb.is_random_next.cpu().numpy().astype(np.int64),
                              L, IGN)
    assert n_masked > 100


def test_pair_kernels_equal_the_string_kernel_2_byte_ids(ctx_u, parsed):
    assert ctx_u.id_bytes == 2
    _check_pairs(ctx_u, parsed)


def test_pair_kernels_equal_the_string_kernel_4_byte_ids(tmp_path, parsed):
    from lddl_amd.context import Context
    with open(VOCAB_UNCASED) as f:
        lines = f.read().splitlines()
    big = tmp_path / 'vocab_big.txt'
    big.write_text('\n'.join(lines + ['[extra{}]'.format(i) for i in range(40000)]) + '\n')
    wide = Context(str(big))
    assert wide.id_bytes == 4
    _check_pairs(wide, parsed)


# ---- the packed string collate, through the C ABI ------------------------------------------------
def _seqpack_span(ctx, batch, L, align, mask, span):
    """lddl_collate_seqpack_masked_span called as the C ABI defines it, for `batch` planned into
    rows of L slots: the arguments of lddl_collate_seqpack_masked without the whole_word flag,
    plus the params. (encode_seqpacked, which stages the same arrays for the sibling, takes no
    span argument.) span=None calls that sibling, lddl_collate_seqpack_masked with whole_word = 1,
    on the same arrays. Returns encode_seqpacked's dict."""
    from lddl_amd._native import check, lib
    from lddl_amd.context import _ptr, _stream
    from lddl_amd.torch.bert import PackedBatch
    from lddl_amd.torch.seqpack import plan_rows
    pk = PackedBatch(batch)
    B = len(pk)
    lens = (pk.na + pk.nb + 3).astype(np.int32)
    plan = plan_rows(lens, L)
    stride = ((int(lens.max()) - 1) // align + 1) * align  # the unpacked batch's width
    dst = plan.row.astype(np.int64) * L + plan.start
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()  # noqa: E731
    d_blob = torch.from_numpy(np.ascontiguousarray(pk.blob)).cuda()
    d_a, d_b, d_dst = dev(pk.a_off, np.int64), dev(pk.b_off, np.int64), dev(dst, np.int64)
    d_na, d_nb = dev(pk.na, np.int32), dev(pk.nb, np.int32)
    d_fill, d_seq = dev(plan.fill, np.int32), dev(plan.seq_in_row, np.int32)
    assert len(pk.a_off) == len(pk.b_off) == B + 1 and int(pk.b_off[-1]) <= len(pk.blob)
    assert int((dst + plan.fill).max()) <= plan.R * L and int(lens.max()) <= L
    out = {k: torch.empty(plan.R, L, dtype=torch.long, device='cuda')
           for k in ('input_ids', 'token_type_ids', 'attention_mask', 'labels', 'position_ids',
                     'sequence_ids')}
    p, seed, counter = mask
    entry, last = (lib.lddl_collate_seqpack_masked, 1) if span is None else \
        (lib.lddl_collate_seqpack_masked_span, span.ptr(p))
    check(entry(
        ctx.handle, _stream(), _ptr(d_blob), _ptr(d_a), _ptr(d_b), _ptr(d_na), _ptr(d_nb), B,
        _ptr(d_dst), _ptr(d_fill), _ptr(d_seq), L, stride, _ptr(out['input_ids']),
        _ptr(out['token_type_ids']), _ptr(out['attention_mask']), _ptr(out['labels']),
        _ptr(out['position_ids']), _ptr(out['sequence_ids']), float(p), IGN, len(ctx), seed,
        counter, last))
    order = plan.order
    out['next_sentence_labels'] = dev(np.asarray(pk.nsl)[order], np.int64)
    out['cls_positions'] = dev(dst[order], np.int64)
    out['seq_lens'] = dev(lens[order], np.int32)
    return out, pk, lens


@pytest.mark.parametrize('name', ['n3', 'onehot16'])
def test_packed_string_entry_point_equals_unpacked_rows(ctx_c, dyn_samples, parsed, name):
    """Sample i's segment of the packed rows is row i of encode_packed(span=) with the same
    seed and counter (draw_stride = the unpacked width)."""
    from lddl_amd.torch.bert import encode_packed
    from test_seqpack_gpu import assert_packed
    span, mask = parsed[name], (0.15, SEED, COUNTER)
    n_masked = 0
    for B in (1, 5, 9):
        batch = dyn_samples[-B:]
        longest = max(len(a.split()) + len(b.split()) + 3 for a, b, _ in batch)
        L = max(longest, 200)
        for align in (8, 64):
            got, pk, lens = _seqpack_span(ctx_c, batch, L, align, mask, span)
            unp = encode_packed(pk, ctx_c, align, IGN, mask=mask, span=span)
            assert_packed(got, unp, lens.tolist(), pk.nsl, L, IGN)
            n_masked += int((got['labels'] != IGN).sum())
    assert n_masked > 0


# ---- the two word modes of each kernel's one loop against each other ----------------------------
def _edge_pairs(words, cont):
    """Five hand-made pairs of at most 128 slots: the last [SEP] on slot 63 and on slot 64 (the
    whole-word carry and the span state both cross a window), a '##' piece at the head of B, a
    pair that fills 128 slots and the smallest pair. A third of the ids are '##' pieces."""
    rng = np.random.default_rng(26)

    def ids(n):
        return np.where(rng.random(n) < 0.33, cont[rng.integers(0, len(cont), n)],
                        words[rng.integers(0, len(words), n)])
    out = []
    for slots, na in ((64, 30), (65, 31), (100, 40), (128, 70), (5, 1)):
        t = ids(slots - 3)
        out.append([t[:na], t[na:], bool(rng.integers(0, 2))])
    out[2][1][0] = cont[7]  # B starts with a piece: behind [SEP] it is a head, not a continuation
    out[0][0][-1], out[1][0][-1] = cont[3], cont[5]  # a word that ends against the middle [SEP]
    return out


def _same(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)
    return int((a['labels'] != IGN).sum())


@pytest.mark.parametrize('p', [0.15, 1.0])
def test_n1_is_whole_word_masking_in_every_collate_kernel(ctx_u, ctx_c, dyn_samples, parsed, p):
    """span=1 and whole_word=True run the same loop of each kernel with the other of its two
    decisions: at equal (seed, counter) every output is bit-equal, through
    encode_packed, collate_pairs (2-byte ids), collate_pairs_seqpacked and, through the C ABI,
    lddl_collate_seqpack_masked / _masked_span. Batches of 5, packed rows of 128 slots."""
    from lddl_amd.torch.bert import PackedBatch, encode_packed
    from lddl_amd.torch.online import collate_pairs, collate_pairs_seqpacked, plan_rows_device
    from test_online_seqpack_gpu import _pair_batch
    n1, mask, L = parsed['n1'], (p, SEED, COUNTER), 128
    assert ctx_u.id_bytes == 2
    words, cont = _ascii_ids(ctx_u)
    samples = _edge_pairs(words, cont)
    lens = [len(a) + len(b) + 3 for a, b, _ in samples]
    assert lens == [64, 65, 100, 128, 5] and len(samples) == 5
    assert ctx_u.tokens[samples[2][1][0]].startswith('##')
    pb = _pair_batch(ctx_u, samples)
    assert pb.num_tokens.tolist() == lens
    rendered = _tuples(ctx_u, pb)
    # the fixture's samples that fit a packed row, the first five
    short = [t for t in dyn_samples if len(t[0].split()) + len(t[1].split()) + 3 <= L][:5]
    assert len(short) == 5
    n_masked = 0
    for ctx, batch in ((ctx_u, rendered), (ctx_c, short)):  # the string kernels
        pk = PackedBatch(batch)
        for align in (8, 64):
            ww = encode_packed(pk, ctx, align, IGN, mask=mask, whole_word=True)
            sp = encode_packed(pk, ctx, align, IGN, mask=mask, span=n1)
            n_masked += _same(ww, sp, ('encode_packed', align))
            ww = _seqpack_span(ctx, batch, L, align, mask, None)[0]
            sp = _seqpack_span(ctx, batch, L, align, mask, n1)[0]
            n_masked += _same(ww, sp, ('lddl_collate_seqpack_masked', align))
    # the pair-table kernels
    ww = collate_pairs(ctx_u, pb, None, 8, IGN, mask=mask, whole_word=True)
    sp = collate_pairs(ctx_u, pb, None, 8, IGN, mask=mask, span=n1)
    n_masked += _same(ww, sp, 'collate_pairs')
    # (the hand-made pairs are the strings' ids: the table kernel sees what the string kernel saw)
    assert torch.equal(ww['input_ids'],
                       encode_packed(PackedBatch(rendered), ctx_u, 8, IGN, mask=mask,
                                     whole_word=True)['input_ids'])
    stride = ww['input_ids'].shape[1]
    plan = plan_rows_device(ctx_u, pb, None, [0, 5], L)
    ww = collate_pairs_seqpacked(ctx_u, pb, None, plan, 0, None, L, stride, IGN, mask=mask,
                                 whole_word=True)
    sp = collate_pairs_seqpacked(ctx_u, pb, None, plan, 0, None, L, stride, IGN, mask=mask,
                                 span=n1)
    n_masked += _same(ww, sp, 'collate_pairs_seqpacked')
    assert n_masked > 100


# ---- refusals -----------------------------------------------------------------------------------
def test_entry_points_refuse_null_context_and_null_or_invalid_params(ctx_u):
    import ctypes
    from lddl_amd._native import SpanParams, lib
    from lddl_amd.context import _ptr, _stream
    from lddl_amd.torch import span as S
    ok = S.parse(3).ptr(0.15)
    bad = SpanParams()
    ctypes.memmove(ctypes.byref(bad), ctypes.byref(S.parse(3).params(0.15)), ctypes.sizeof(bad))
    bad.n = 17
    bad_n = ctypes.cast(ctypes.pointer(bad), ctypes.c_void_p)
    bad2 = SpanParams()
    ctypes.memmove(ctypes.byref(bad2), ctypes.byref(S.parse(3).params(0.15)), ctypes.sizeof(bad2))
    bad2.cum[1] = 0.1  # below cum[0]
    bad_cum = ctypes.cast(ctypes.pointer(bad2), ctypes.c_void_p)
    o = [torch.full((2, 16), 77, dtype=torch.long, device='cuda') for _ in range(6)]
    z = torch.zeros(8, dtype=torch.long, device='cuda')
    zi = torch.zeros(8, dtype=torch.int32, device='cuda')
    h = ctx_u.handle
    P = _ptr

    def calls(c, sp):
        m = (0.15, IGN, len(ctx_u), 1, 2, sp)
        return [
            lib.lddl_mask_dynamic_span(c, _stream(), P(o[0]), P(o[1]), None, None, None, 2, 16,
                                       *m),
            lib.lddl_collate_encode_masked_span(c, _stream(), P(z), P(z), P(z), P(zi), P(zi), 2,
                                                16, P(o[0]), P(o[1]), P(o[2]), P(o[3]), *m),
            lib.lddl_collate_seqpack_masked_span(c, _stream(), P(z), P(z), P(z), P(zi), P(zi), 2,
                                                 P(z), P(zi), P(zi), 16, 16, P(o[0]), P(o[1]),
                                                 P(o[2]), P(o[3]), P(o[4]), P(o[5]), *m),
            lib.lddl_collate_pairs_masked_span(c, _stream(), P(zi), P(z), P(zi), P(zi), None, 2,
                                               16, P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(z), *m),
            lib.lddl_collate_pairs_seqpack_masked_span(
                c, _stream(), P(zi), P(z), P(zi), P(zi), None, 2, P(z), P(zi), P(zi), P(zi), 2, 16,
                16, P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]), P(o[5]), P(z), P(z), P(zi), *m)]
    assert calls(None, ok) == [-1] * 5
    assert b'null ctx' in lib.lddl_last_error()
    assert calls(h, None) == [-1] * 5
    assert b'null span params' in lib.lddl_last_error()
    assert calls(h, bad_n) == [-1] * 5
    assert b'invalid span params' in lib.lddl_last_error()
    assert calls(h, bad_cum) == [-1] * 5
    torch.cuda.synchronize()
    assert all(int((t != 77).sum()) == 0 for t in o)  # nothing was launched


def test_span_with_replay_raises(ctx_u):
    from lddl_amd.torch.bert import _mask_tokens
    ids = torch.full((2, 8), 1500, dtype=torch.long, device='cuda')
    z = torch.zeros(2, 8, dtype=torch.uint8)
    rep = dict(masked=z, replaced=z, random=z, words=torch.zeros(2, 8, dtype=torch.long))
    with pytest.raises(ValueError, match='span'):
        _mask_tokens(ids.clone(), None, ctx_u, replay=rep, span=3)
    assert bool((ids == 1500).all())
