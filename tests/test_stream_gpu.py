"""The GPT stream on the GPU: `stream_plan` and `collate_stream` bit for bit against
stream_oracle.py on a hand-built token table at the edge lengths, with and without
fill-in-the-middle; the loader against the helper."""
import functools

import numpy as np
import pytest

import stream_oracle as O

pytestmark = pytest.mark.gpu
V, EOS, PRE, MID, SUF = 1000, 2, 1001, 1002, 1003
SP = dict(eos_id=EOS, fim_prefix_id=PRE, fim_middle_id=MID, fim_suffix_id=SUF)
SEED, COUNTER = 1, 3  # test_the_seed_draws_the_edge_cuts: what these give
FIMS = [(0, 0), (1, 0), (1, 1), (0.5, 0.5)]
Vocab = type('Vocab', (), {'special_ids': {}, '__len__': lambda self: V})  # what collate_stream reads


def documents(L):
    """Sentence lengths per document: the edge lengths, one longer than 2 L + 2 (some row holds
    no boundary), several sentences with empty ones, and 600 empty documents with and without
    a sentence: at L = 1030 a tile overlaps more than LDDL_STREAM_LDS_DOCS places."""
    return [[0], [1], [2], [3]] + [[], [0]] * 300 + [
        [L - 1], [L], [L + 1], [1], [2], [3], [2 * L + 5], [3, 0, 4], [0, 0, 2, 0], [], [1, 1, 1],
        [2], [1], [5, 0]]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fim_of(rates):
    return None if rates[0] == 0 else rates + (SEED, COUNTER)


@functools.lru_cache(maxsize=None)
def table(L, rates, short):
    """ctx.tokenize's layout (gaps, flag bits) on the host, with a last document sized so that
    the stream holds n_rows * L + 1 tokens exactly, or one less with `short`."""
    docs = documents(L)
    costs = [sum(doc) + 1 + (3 if O.fim_draw(d, sum(doc), fim_of(rates)) else 0)
             for d, doc in enumerate(docs)]
    last = 3 if O.fim_draw(len(docs), 2, fim_of(rates)) else 0  # the same for every t >= 1
    t = 2 + (-(sum(costs) + 2 + 1 + last) + 1) % L  # t >= 2: `short` keeps the draw
    docs = docs + [[t - short]]
    rng = np.random.default_rng(34)
    ids, sent_off, sent_len, dso = [], [], [], [0]
    for doc in docs:
        for n in doc:
            sent_off.append(len(ids))
            sent_len.append(n | ((1 << 30) if n % 3 == 1 else 0))
            ids += rng.integers(10, V, n).tolist() + [0] * int(rng.integers(1, 4))
        dso.append(len(sent_len))
    return (np.array(ids, np.int32), np.array(sent_off + [len(ids)], np.int64),
            np.array(sent_len, np.int32), np.array(dso, np.int64))


def run_both(L, rates=(0, 0), short=0, order=None, rows=None, max_seqs=None, **flags):
    """collate_stream and the oracle on the same call -> (the oracle's stream, its batch, the
    draws); asserts that they agree bit for bit."""
    from lddl_amd.torch import collate_stream, stream_plan
    host = table(L, rates, short)
    on_dev = [dev(a) for a in host]
    toks, term, draws = O.stream(host, order, fim_of(rates), EOS, PRE, MID, SUF)
    plan, n = stream_plan(on_dev, L, None if order is None else dev(order), fim_of(rates))
    assert n == O.n_rows(len(toks), L) and int(plan.counts[1]) == len(toks)
    assert len(toks) == (n + short) * L + 1 - short  # `short` costs the last row
    got = collate_stream(Vocab(), on_dev, plan, None if rows is None else dev(np.array(rows)),
                         max_seqs=max_seqs, special_ids=SP, **flags)
    want = O.collate(toks, term, L, rows, max_seqs=got['cu_seqlens'].numel() - 1, **flags)
    assert got.keys() == want.keys()
    for k in want:
        np.testing.assert_array_equal(got[k].cpu().numpy().reshape(-1),
                                      np.array(want[k]).reshape(-1), err_msg=k)
    return toks, want, draws


@pytest.mark.parametrize('short', [0, 1])
@pytest.mark.parametrize('rates', FIMS)
@pytest.mark.parametrize('L', [5, 64, 1030])
def test_rows_match_the_oracle(L, rates, short):
    n_doc = len(table(L, rates, short)[3]) - 1
    toks, want, _ = run_both(L, rates, short)  # every row, the default cap, the default flags
    assert want['n_seqs'] < len(want['cu_seqlens'])
    assert any(len(set(r)) == 1 for r in want['sequence_ids'])  # a row without a boundary
    order = np.random.default_rng(L).permutation(n_doc)
    rows = [3, 0, 3, O.n_rows(len(toks), L) - 1, 1]  # a repeat, the last row, five rows
    _, cut, _ = run_both(L, rates, short, order, rows, max_seqs=7, eod_mask_loss=True,
                         reset_position_ids=False)
    assert cut['n_seqs'] > 7 and cut['cu_seqlens'][7] == 5 * L  # the overflow contract
    run_both(L, rates, short, order, rows, eod_mask_loss=True)


def test_the_seed_draws_the_edge_cuts():
    for L in (5, 64, 1030):
        for rates in FIMS[1:]:
            host = table(L, rates, 0)
            draws = O.stream(host, None, fim_of(rates))[2]
            t = {d: len(O.doc_tokens(host, d)) for d in draws}
            hit = [(t[d], a, b) for d, v in draws.items() if v for _, a, b in [v]]
            assert any(a == 0 for _, a, _ in hit) and any(b == n for n, _, b in hit)
            assert any(a == b for _, a, b in hit) and any(n == 1 for n, _, _ in hit)
            assert len({bool(v and v[0]) for v in draws.values() if v}) == 1 + (rates[1] == 0.5)


def test_without_fim_the_rows_concatenate_to_the_stream():
    toks, want, _ = run_both(64)
    flat = [v for r in want['input_ids'] for v in r]
    assert flat == toks[:len(flat)] and len(toks) - len(flat) == 1


def test_psm_rows_restore_every_document():
    L = 64
    host = table(L, (1, 0), 0)
    toks, want, draws = run_both(L, (1, 0))
    flat, d = [v for r in want['input_ids'] for v in r] + toks[-1:], 0
    while flat:  # <pre> prefix <suf> suffix <mid> middle eos, or the empty document's eos
        end = flat.index(EOS)
        doc, flat = flat[:end], flat[end + 1:]
        if doc:
            s, m = doc.index(SUF), doc.index(MID)
            assert doc[0] == PRE and draws[d][1:] == (s - 1, s - 1 + len(doc) - m - 1)
            doc = doc[1:s] + doc[m + 1:] + doc[s + 1:m]
        assert doc == O.doc_tokens(host, d)
        d += 1
    assert d == len(host[3]) - 1


def test_equal_draws_give_equal_batches_and_the_counter_changes_them():
    from lddl_amd.torch import collate_stream, stream_plan
    on_dev = [dev(a) for a in table(64, (0.5, 0.5), 0)]
    rows = dev(np.arange(4))
    ids = [collate_stream(Vocab(), on_dev, stream_plan(on_dev, 64, None, (0.5, 0.5, SEED, c))[0],
                          rows, special_ids=SP)['input_ids'] for c in (COUNTER, COUNTER, COUNTER + 1)]
    assert (ids[0] == ids[1]).all() and (ids[0] != ids[2]).any()


def test_loader_batches_are_the_helper_on_the_same_rows(tmp_path):
    import torch
    from lddl_amd import bpe as B
    from lddl_amd.torch import get_gpt_pretrain_data_loader
    lines = ['Document number {} has words {}.'.format(i, 'and on ' * (i % 7)) for i in range(40)]
    for k in range(2):
        (tmp_path / '{}.txt'.format(k)).write_text('\n'.join(lines[20 * k:20 * k + 20]))
    fim = dict(fim_rate=0.5, special_ids=dict(fim_prefix_id=5, fim_middle_id=6, fim_suffix_id=7))
    for kw in ({}, fim):
        a = get_gpt_pretrain_data_loader(str(tmp_path), (B.SYNTH_VOCAB, B.SYNTH_MERGES),
                                         batch_size=3, max_seq_length=48, **kw)
        epochs = list(a), list(a)
        for epoch, batches in enumerate(epochs):
            table_, plan, n = a.plan_round(a.files, epoch, 0)
            assert sum(x['input_ids'].shape[0] for x in batches) == n and len(batches) > 1
            perm = torch.from_numpy(a.order(epoch, 0, n)).cuda()
            for step, x in enumerate(batches):
                want = a.collate(table_, plan, perm[3 * step:3 * step + 3], epoch, step)
                assert x.keys() == want.keys() and all(torch.equal(x[k], want[k]) for k in x)
        assert not torch.equal(epochs[0][0]['input_ids'], epochs[1][0]['input_ids'])
    plain = get_gpt_pretrain_data_loader(str(tmp_path), (B.SYNTH_VOCAB, B.SYNTH_MERGES),
                                         batch_size=3, max_seq_length=48, shuffle_docs=False)
    iter(plain)
    table_, plan, n = plain.plan_round(plain.files)
    first = plain.bpe.encode(lines[0])
    row0 = plain.collate(table_, plan, None, 0, 0)['input_ids'][0].tolist()
    assert row0[:len(first) + 1] == first + [plain.bpe.special_ids['</s>']]
