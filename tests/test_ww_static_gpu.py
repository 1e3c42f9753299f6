"""Whole-word static masking in the pair planner (make_pairs(..., whole_word=True)).

No oracle exists for it (the reference has no whole-word masking), so every pair is checked
against the definition, on the host, from the vocab file:

* special: the id is [CLS] or [SEP] (literal ones in the text);
* continuation: not special, not first in A or B, the token before it not special, and the id a
  "##x" vocab entry; a word is a head and the continuations after it;
* budget: num = min(max(1, rint((na + nb + 3) * ratio)), non-special tokens);
* the masked set is a union of words of at most num tokens, and maximal: it has num tokens or no
  unmasked word fits in what is left.

The statistical bounds are 5 sigma binomial bounds (fixed seeds: a pass is stable)."""
import ctypes
import logging
import os
import re

import numpy as np
import pytest
import torch

from conftest import VOCAB_UNCASED

pytestmark = pytest.mark.gpu

RATIO = 0.15
FLAG = 1 << 30  # sent_len: the sentence holds a literal [CLS] / [SEP]


@pytest.fixture(scope='module')
def ctx():
    from lddl_amd.context import Context
    return Context(VOCAB_UNCASED, True)


def cont_ids(ctx):
    """[vocab] bool: the vocab line starts with '##' and is longer than 2 bytes."""
    return np.array([t.startswith('##') and len(t.encode('utf-8')) > 2 for t in ctx.tokens])


def partition_docs(corp, partition_bytes):
    doc_bytes = corp.sent_off[corp.doc_sent_off]
    cuts = np.searchsorted(doc_bytes, np.arange(0, doc_bytes[-1], partition_bytes), 'left')
    return np.unique(np.concatenate([[0], cuts, [corp.n_doc]])).astype(np.int64)


def synth_batch(ctx, n_bytes=512 << 10, part_bytes=64 << 10, seed=77):
    from lddl_amd import synth
    corp = synth.generate(seed=seed, n_bytes=n_bytes, nonascii_frac=0.01, threads=4)
    part = partition_docs(corp, part_bytes)
    dev = ctx.device
    sent_off = torch.from_numpy(corp.sent_off).to(dev)
    ids, sent_len = ctx.tokenize(torch.from_numpy(corp.text).to(dev), sent_off)
    return dict(part=part, seeds=np.arange(len(part) - 1, dtype=np.int64) * 7919 + 12345,
                sent_off=sent_off, ids=ids, sent_len=sent_len,
                doc_off=torch.from_numpy(corp.doc_sent_off).to(dev))


def run(ctx, b, seq=128, parts=None, native_seed=4242, batch=False, **kw):
    from lddl_amd.pairs import make_pairs
    part, seeds = b['part'], b['seeds']
    if parts is not None:
        part, seeds = part[parts[0]:parts[1] + 1], seeds[parts[0]:parts[1]]
    pb = make_pairs(ctx, b['sent_off'], b['ids'], b['sent_len'], b['doc_off'],
                    torch.from_numpy(part).to(ctx.device), torch.from_numpy(seeds).to(ctx.device),
                    seq=seq, dup=5, masking=True, masked_lm_ratio=RATIO, rng='native',
                    native_seed=native_seed, **kw)
    out = pb.to_host()
    out['n_mask'] = pb.n_masked
    return (out, pb) if batch else out


def restored(out):
    """The pairs' tokens with the labels put back at the masked positions."""
    tok = out['tokens'].astype(np.int64)
    pair_of = np.repeat(np.arange(len(out['len_a'])), np.diff(out['pos_off']))
    p = out['pos'].astype(np.int64)
    la = out['len_a'][pair_of]
    tok[out['tok_off'][pair_of] + np.where(p <= la, p - 1, p - 2)] = out['labels']
    return tok


def check_pairs(out, ctx, seq):
    """Properties 2 and 3 of every pair; returns per-pair records for the statistics."""
    cv = cont_ids(ctx)
    cls_id, sep_id = ctx.vocab['[CLS]'], ctx.vocab['[SEP]']
    orig_all = restored(out)
    tok_off, len_a, pos_off = out['tok_off'], out['len_a'], out['pos_off']
    n_pairs = len(len_a)
    assert out['n_mask'] == pos_off[-1] == int(np.diff(pos_off).sum()) == len(out['pos'])
    assert len(out['labels']) == len(out['pos'])
    recs = []
    for q in range(n_pairs):
        orig = orig_all[tok_off[q]:tok_off[q + 1]]
        n, na = len(orig), int(len_a[q])
        assert 1 <= na < n <= seq - 3
        pos = out['pos'][pos_off[q]:pos_off[q + 1]].astype(np.int64)
        assert np.all(np.diff(pos) > 0)
        assert np.all(((pos >= 1) & (pos <= na)) | ((pos >= na + 2) & (pos <= n + 1)))
        idx = np.where(pos <= na, pos - 1, pos - 2)
        special = (orig == cls_id) | (orig == sep_id)
        assert not special[idx].any()
        first = np.zeros(n, bool)
        first[[0, na]] = True
        prev_sp = np.concatenate([[True], special[:-1]])
        cont = ~special & ~first & ~prev_sp & cv[orig]
        masked = np.zeros(n, bool)
        masked[idx] = True
        # whole words: a continuation is masked iff the token before it is
        assert (masked[1:][cont[1:]] == masked[:-1][cont[1:]]).all(), q
        head = ~special & ~cont
        wid = np.cumsum(head) - 1
        nw = int(head.sum())
        wlen = np.bincount(wid[~special], minlength=nw)
        wmask = masked[head]
        nc = int((~special).sum())
        num = min(max(1, int(np.round((n + 3) * RATIO))), nc)
        m = int(masked.sum())
        assert m <= num, (q, m, num)
        assert m == num or (wlen[~wmask] > num - m).all(), (q, m, num)
        recs.append(dict(q=q, n=n, na=na, num=num, m=m, nw=nw, wlen=wlen, wmask=wmask,
                         head_at=np.flatnonzero(head), orig=orig, special=special, cont=cont,
                         masked=masked))
    return recs


@pytest.fixture(scope='module')
def corpus(ctx):
    return synth_batch(ctx)


@pytest.fixture(scope='module')
def runs(ctx, corpus):
    """seq -> (plain native run, whole-word run) of the shared corpus; computed once."""
    return {seq: (run(ctx, corpus, seq=seq), run(ctx, corpus, seq=seq, whole_word=True))
            for seq in (128, 512)}


@pytest.fixture(scope='module')
def records(ctx, runs):
    return {seq: check_pairs(runs[seq][1], ctx, seq) for seq in runs}


# ---- 1. the same pairs ------------------------------------------------------------------------
@pytest.mark.parametrize('seq', [128, 512])
def test_same_pairs_as_plain_native(ctx, corpus, runs, seq):
    plain, ww = runs[seq]
    for k in ('tok_off', 'len_a', 'is_random_next', 'part_off'):
        np.testing.assert_array_equal(ww[k], plain[k], err_msg=k)
    # labels are the original ids: with them put back, the tokens are the plain run's
    np.testing.assert_array_equal(restored(ww), restored(plain))
    assert len(ww['len_a']) > 500
    off = run(ctx, corpus, seq=seq, whole_word=False)
    for k in ('tokens', 'tok_off', 'len_a', 'is_random_next', 'part_off', 'pos', 'labels',
              'pos_off'):
        np.testing.assert_array_equal(off[k], plain[k], err_msg=k)


# ---- 2 + 3. whole words, budget, maximality: every pair ----------------------------------------
@pytest.mark.parametrize('seq', [128, 512])
def test_whole_words_budget_maximal(records, seq):
    recs = records[seq]  # (check_pairs asserted the properties pair by pair)
    assert sum(int(r['cont'].sum()) for r in recs) > 1000  # the corpus has multi-piece words
    assert sum(int((r['masked'] & r['cont']).sum()) for r in recs) > 100
    assert sum(r['m'] == r['num'] for r in recs) > len(recs) // 2
    # words over a 64-token window boundary are masked too (seq 512: the carry across windows)
    if seq == 512:
        cross = 0
        for r in recs:
            h = r['head_at'][r['wmask']]
            cross += int(((h // 64) != ((h + r['wlen'][r['wmask']] - 1) // 64)).sum())
        assert cross > 10


# ---- 4. crafted id streams ---------------------------------------------------------------------
@pytest.fixture(scope='module')
def ctx_bare(tmp_path_factory):
    """A context over the vocab with one entry replaced by the bare token '##'."""
    from lddl_amd.context import Context
    lines = open(VOCAB_UNCASED, encoding='utf-8').read().split('\n')
    lines[2500] = '##'
    path = tmp_path_factory.mktemp('vocab') / 'vocab_bare.txt'
    path.write_text('\n'.join(lines), encoding='utf-8')
    c = Context(str(path), True)
    assert c.vocab['##'] == 2500 and not cont_ids(c)[2500]
    return c


def crafted(ctx, docs, n_part=1):
    """docs: list of documents, each a list of sentences (lists of ids). Sentence s's ids lie at
    ids[sent_off[s]:], as the tokenizer leaves them; sent_len carries the literal-special flag."""
    cls_id, sep_id = ctx.vocab['[CLS]'], ctx.vocab['[SEP]']
    sents = [np.asarray(s, np.int32) for d in docs for s in d]
    lens = np.array([len(s) for s in sents], np.int64)
    flag = np.array([bool(np.isin(s, [cls_id, sep_id]).any()) for s in sents])
    sent_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    doc_off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    part = np.round(np.linspace(0, len(docs), n_part + 1)).astype(np.int64)
    dev = ctx.device
    return dict(part=part, seeds=np.arange(n_part, dtype=np.int64) * 31 + 5,
                sent_off=torch.from_numpy(sent_off).to(dev),
                ids=torch.from_numpy(np.concatenate(sents)).to(dev),
                sent_len=torch.from_numpy((lens | np.where(flag, FLAG, 0)).astype(np.int32)).to(dev),
                doc_off=torch.from_numpy(doc_off).to(dev))


def id_pools(ctx):
    cv = cont_ids(ctx)
    W = np.array([i for i in range(1000, len(cv)) if not cv[i] and not ctx.tokens[i].startswith('[')
                  and ctx.tokens[i] != '##'])
    return W, np.flatnonzero(cv)


def test_crafted_words_of_70_pieces(ctx):
    """Heads followed by 69 continuations, between single-piece words, at seq 512 (budget 77):
    every such word crosses a window boundary, and at most one fits the budget."""
    W, C = id_pools(ctx)
    rng = np.random.default_rng(3)
    docs = []
    for _ in range(12):
        doc = []
        for _ in range(5):
            s = []
            for _ in range(2):
                s += list(rng.choice(W, int(rng.integers(1, 6))))
                s += [rng.choice(W)] + list(rng.choice(C, 69))
            doc.append(s)
        docs.append(doc)
    out = run(ctx, crafted(ctx, docs, n_part=2), seq=512, whole_word=True)
    recs = check_pairs(out, ctx, 512)
    assert len(recs) >= 20
    long_masked = sum(int((r['wlen'][r['wmask']] >= 64).sum()) for r in recs)
    assert long_masked >= 10
    assert all((r['wlen'][r['wmask']] >= 64).sum() <= 1 for r in recs)
    assert any(r['wlen'].max() == 70 for r in recs)


def test_crafted_all_continuations_zero_masks(ctx):
    """Documents of continuation ids only: A and B are one word each, both longer than the budget
    (30-token sentences, budget <= 19 at seq 128), so no pair has a mask - and such pairs render."""
    from lddl_amd import output
    from lddl_amd.dask.bert.pretrain import _txt_line
    from lddl_amd.utils import deserialize_np_array
    _, C = id_pools(ctx)
    rng = np.random.default_rng(4)
    docs = [[list(rng.choice(C, 30)) for _ in range(4)] for _ in range(10)]
    out, pb = run(ctx, crafted(ctx, docs), seq=128, whole_word=True, batch=True)
    recs = check_pairs(out, ctx, 128)
    assert len(recs) >= 20
    assert all(r['nw'] == 2 and r['m'] == 0 and r['num'] >= 1 for r in recs)
    assert out['n_mask'] == 0 and len(out['pos']) == 0 and not out['pos_off'].any()
    plain = run(ctx, crafted(ctx, docs), seq=128)
    np.testing.assert_array_equal(out['tokens'], restored(plain))  # nothing replaced
    rd = output.render(ctx, pb)
    assert rd.n == len(recs)
    for r in range(rd.n):
        row = rd.row(r)
        assert len(deserialize_np_array(row['masked_lm_positions'])) == 0
        assert row['masked_lm_labels'] == ''
        assert 'masked_lm_positions: [] - masked_lm_labels:  - ' in _txt_line(row, True)
    assert output.table(rd, 0, rd.n, True, False).num_rows == rd.n
    # the loaders' collate over such rows: the tokens as they are, no label anywhere
    from lddl_amd.torch.bert import encode_packed
    from lddl_amd.torch.packing import PackedBatch
    rows = [rd.row(r) for r in range(8)]
    enc = encode_packed(PackedBatch([(x['A'], x['B'], x['is_random_next'],
                                      x['masked_lm_positions'], x['masked_lm_labels'])
                                     for x in rows]), ctx)
    assert (enc['labels'] == -1).all()
    ids, att = enc['input_ids'].cpu().numpy(), enc['attention_mask'].cpu().numpy()
    for k, x in enumerate(rows):
        want = ctx.convert_tokens_to_ids(['[CLS]'] + x['A'].split() + ['[SEP]'] + x['B'].split()
                                         + ['[SEP]'])
        assert ids[k, :len(want)].tolist() == want and att[k].sum() == len(want)


def test_crafted_specials_unk_bare_and_cont_first(ctx_bare):
    """Sentences that start with a '##' id (so B does), literal [CLS] / [SEP] inside would-be
    words, [UNK] and the bare '##' between pieces."""
    ctx = ctx_bare
    W, C = id_pools(ctx)
    cv = cont_ids(ctx)
    cls_id, sep_id, unk, bare = (ctx.vocab[t] for t in ('[CLS]', '[SEP]', '[UNK]', '##'))
    rng = np.random.default_rng(5)
    w = lambda: int(rng.choice(W))  # noqa: E731
    c = lambda: int(rng.choice(C))  # noqa: E731
    docs = []
    for _ in range(16):
        doc = []
        for _ in range(6):
            s = [c(), c()]  # a sentence (hence some A and B) starts with a continuation id
            for _ in range(int(rng.integers(2, 5))):
                s += [w(), c(), [cls_id, sep_id][int(rng.integers(2))], c(), c()]
                s += [w(), c(), unk, c(), w(), c(), bare, c(), c()]
            doc.append(s)
        docs.append(doc)
    for seq in (128, 512):
        out = run(ctx, crafted(ctx, docs, n_part=2), seq=seq, whole_word=True)
        recs = check_pairs(out, ctx, seq)
        assert len(recs) >= 20
        after_special = unk_mid = bare_mid = cont_first_b = 0
        for r in recs:
            o, sp = r['orig'], r['special']
            heads = np.zeros(r['n'], bool)
            heads[r['head_at']] = True
            assert not (r['masked'] & sp).any()
            after = np.flatnonzero(sp[:-1] & cv[o[1:]]) + 1  # a '##' id right after a special
            assert heads[after].all()
            after_special += int((r['masked'][after]).sum())
            assert heads[(o == unk) | (o == bare)].all()
            unk_mid += int(r['masked'][o == unk].sum())
            bare_mid += int(r['masked'][o == bare].sum())
            if cv[o[r['na']]]:
                assert heads[r['na']]
                cont_first_b += 1
        assert after_special > 0 and unk_mid > 0 and bare_mid > 0 and cont_first_b > 0


def test_crafted_pair_of_two_tokens(ctx):
    """Two one-token sentences per document: every pair is [CLS] x [SEP] y [SEP], budget 1, and
    exactly one of its two words is masked."""
    W, _ = id_pools(ctx)
    rng = np.random.default_rng(6)
    docs = [[[int(rng.choice(W))], [int(rng.choice(W))]] for _ in range(40)]
    out = run(ctx, crafted(ctx, docs), seq=128, whole_word=True)
    recs = check_pairs(out, ctx, 128)
    two = [r for r in recs if r['n'] == 2]
    assert len(two) >= 50
    assert all(r['num'] == 1 and r['m'] == 1 for r in two)
    first = sum(int(r['masked'][0]) for r in two)
    assert abs(first - len(two) / 2) <= 5 * np.sqrt(len(two)) / 2  # either word, fairly


# ---- 5. randomness ------------------------------------------------------------------------------
def test_decision_shares(ctx, runs):
    mask_id = ctx.vocab['[MASK]']
    for seq in (128, 512):
        out = runs[seq][1]
        pair_of = np.repeat(np.arange(len(out['len_a'])), np.diff(out['pos_off']))
        p = out['pos'].astype(np.int64)
        la = out['len_a'][pair_of]
        got = out['tokens'][out['tok_off'][pair_of] + np.where(p <= la, p - 1, p - 2)]
        M = len(got)
        assert M > 20000
        f_mask = np.mean(got == mask_id)
        f_keep = np.mean(got == out['labels'])
        f_rand = 1.0 - f_mask - f_keep
        print('seq {} M={} [MASK]={:.5f} keep={:.5f} random={:.5f}'.format(seq, M, f_mask, f_keep,
                                                                          f_rand))
        for f, pr in ((f_mask, 0.8), (f_keep, 0.1), (f_rand, 0.1)):
            assert abs(f - pr) <= 5 * np.sqrt(pr * (1 - pr) / M)


def test_selection_is_a_shuffle(records):
    """Masked words in the first and in the last floor(nw / 2) words of the pairs with >= 20 words:
    the corpus is iid, so the two counts differ by a binomial fluctuation only."""
    for seq in (128, 512):
        m1 = m2 = 0
        for r in records[seq]:
            if r['nw'] >= 20:
                half = r['nw'] // 2
                m1 += int(r['wmask'][:half].sum())
                m2 += int(r['wmask'][r['nw'] - half:].sum())
        print('seq {} masked words: first halves {} last halves {}'.format(seq, m1, m2))
        assert m1 + m2 > 5000
        assert abs(m1 - m2) <= 5 * np.sqrt(m1 + m2)


def test_duplicates_carry_different_masks(runs, records):
    """Pairs with the same A and B (the duplicates of a document often cut the same pair) do not
    share their masks: each pair's draws are keyed by its own index."""
    out = runs[128][1]
    part_of = np.searchsorted(out['part_off'], np.arange(len(out['len_a'])), 'right') - 1
    groups = {}
    for r in records[128]:
        if r['n'] >= 40:
            groups.setdefault((int(part_of[r['q']]), r['na'], r['orig'].tobytes()), []).append(
                r['masked'].tobytes())
    multi = [g for g in groups.values() if len(g) >= 2]
    assert len(multi) >= 5
    assert sum(len(set(g)) > 1 for g in multi) >= len(multi) - 1


# ---- 6. determinism -----------------------------------------------------------------------------
def test_deterministic_batching_invariant_seeded(ctx, corpus, runs):
    full = runs[128][1]
    again = run(ctx, corpus, whole_word=True)
    keys = ('tokens', 'tok_off', 'len_a', 'is_random_next', 'pos', 'labels', 'pos_off')
    for k in keys:
        np.testing.assert_array_equal(full[k], again[k], err_msg=k)
    n_part = len(corpus['part']) - 1
    h = n_part // 2
    tail = run(ctx, corpus, parts=(h, n_part), whole_word=True)
    po = full['part_off']
    q0, q1 = po[h], po[-1]
    t0, m0 = full['tok_off'][q0], full['pos_off'][q0]
    np.testing.assert_array_equal(tail['len_a'], full['len_a'][q0:q1])
    np.testing.assert_array_equal(tail['tokens'], full['tokens'][t0:])
    np.testing.assert_array_equal(tail['pos_off'], full['pos_off'][q0:] - m0)
    np.testing.assert_array_equal(tail['pos'], full['pos'][m0:])
    np.testing.assert_array_equal(tail['labels'], full['labels'][m0:])
    other = run(ctx, corpus, native_seed=4243, whole_word=True)
    assert not (len(other['pos']) == len(full['pos']) and np.array_equal(other['pos'], full['pos']))


# ---- 7. errors ----------------------------------------------------------------------------------
def test_bad_combinations_raise_and_the_context_lives(ctx, corpus, runs):
    from lddl_amd._native import lib, PairParams, RNG_NATIVE, RNG_REPLAY
    from lddl_amd.pairs import make_pairs
    b = corpus
    args = (ctx, b['sent_off'], b['ids'], b['sent_len'], b['doc_off'],
            torch.from_numpy(b['part']).to(ctx.device), torch.from_numpy(b['seeds']).to(ctx.device))
    with pytest.raises(ValueError, match='whole_word'):
        make_pairs(*args, masking=True, rng='replay', whole_word=True)
    with pytest.raises(ValueError, match='whole_word'):
        make_pairs(*args, masking=False, rng='native', whole_word=True)
    # the library's own check (a caller of the C ABI), before anything is allocated
    for prm in (PairParams(128, 5, 1, RNG_REPLAY, 0.1, RATIO, 1, 1),
                PairParams(128, 5, 0, RNG_NATIVE, 0.1, RATIO, 1, 1)):
        h = ctypes.c_void_p()
        assert lib.lddl_pairs_plan(ctx.handle, None, ctypes.byref(prm), None, None, None, 0, None,
                                   0, None, None, 0, ctypes.byref(h), None) == -1
        assert b'whole_word' in lib.lddl_last_error() and not h.value
    again = run(ctx, corpus, whole_word=True)
    np.testing.assert_array_equal(again['pos'], runs[128][1]['pos'])
    np.testing.assert_array_equal(again['tokens'], runs[128][1]['tokens'])


# ---- 8. end to end ------------------------------------------------------------------------------
def _write_source(root, n_docs=120, seed=11):
    from lddl_amd import synth
    corp = synth.generate(seed=seed, n_bytes=n_docs * 3000, nonascii_frac=0.02)
    os.makedirs(os.path.join(root, 'en'))
    lines = ['wiki-{} {}'.format(i, ' '.join(d)) for i, d in enumerate(corp.documents())]
    with open(os.path.join(root, 'en', 'wiki_0.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n\n')


def _row_whole_words(ctx, cv, a, b, pos, labels):
    """Property 2 of one output row (A and B as masked strings, positions, label strings)."""
    ta, tb = a.split(), b.split()
    na, n = len(ta), len(ta) + len(tb)
    orig = np.array(ctx.convert_tokens_to_ids(ta + tb), np.int64)
    pos = np.asarray(pos, np.int64)
    assert len(pos) == len(labels) and np.all(np.diff(pos) > 0)
    assert np.all(((pos >= 1) & (pos <= na)) | ((pos >= na + 2) & (pos <= n + 1)))
    idx = np.where(pos <= na, pos - 1, pos - 2)
    orig[idx] = ctx.convert_tokens_to_ids(labels)
    special = (orig == ctx.vocab['[CLS]']) | (orig == ctx.vocab['[SEP]'])
    first = np.zeros(n, bool)
    first[[0, na]] = True
    cont = ~special & ~first & ~np.concatenate([[True], special[:-1]]) & cv[orig]
    masked = np.zeros(n, bool)
    masked[idx] = True
    assert not (masked & special).any()
    assert (masked[1:][cont[1:]] == masked[:-1][cont[1:]]).all()
    return int((masked & cont).sum())


def test_cli_end_to_end(tmp_path, ctx):
    import pyarrow.parquet as pq
    from lddl_amd.dask.bert import pretrain as P
    from lddl_amd.torch import get_bert_pretrain_data_loader
    from lddl_amd.utils import deserialize_np_array
    src = tmp_path / 'source'
    _write_source(str(src))
    cv = cont_ids(ctx)

    def cli(sink, extra):
        P.main(P.attach_args().parse_args(
            ['--schedule', 'local', '--wikipedia', str(src), '--sink', str(sink), '--masking',
             '--rng', 'native', '--whole-word-masking', '--target-seq-length', '128',
             '--bin-size', '32', '--num-blocks', '2', '--seed', '7', '--vocab-file', VOCAB_UNCASED,
             '--local-n-workers', '1', '--duplicate-factor', '2'] + extra))

    # balanced shards (the streaming balance path), which the loader reads
    sink = tmp_path / 'out'
    cli(sink, ['--num-shards', '2'])
    rows = masked_cont = 0
    for s in range(2):
        for b in range(4):
            for r in pq.read_table(sink / 'shard-{}.parquet_{}'.format(s, b)).to_pylist():
                pos = deserialize_np_array(r['masked_lm_positions'])
                masked_cont += _row_whole_words(ctx, cv, r['A'], r['B'], pos,
                                                r['masked_lm_labels'].split())
                assert len(pos) <= max(1, int(np.round(r['num_tokens'] * RATIO)))
                rows += 1
    assert rows > 50 and masked_cont > 20
    # the loader over that output: the label slots of every batch form whole words
    dl = get_bert_pretrain_data_loader(
        str(sink), vocab_file=VOCAB_UNCASED, data_loader_kwargs={'batch_size': 8, 'num_workers': 1},
        log_level=logging.WARNING)
    sp = ctx.special_ids
    n = n_cont = 0
    for batch in dl:
        lab = batch['labels'].cpu().numpy()
        masked = lab != -1
        orig = np.where(masked, lab, batch['input_ids'].cpu().numpy())
        special = (orig == sp['[CLS]']) | (orig == sp['[SEP]']) | \
            (batch['attention_mask'].cpu().numpy() == 0)
        prev_sp = np.ones_like(special)
        prev_sp[:, 1:] = special[:, :-1]
        cont = ~special & ~prev_sp & cv[orig]
        assert (masked[:, 1:][cont[:, 1:]] == masked[:, :-1][cont[:, 1:]]).all()
        assert not (masked & special).any()
        n += lab.shape[0]
        n_cont += int((masked & cont).sum())
    for gl in getattr(dl, '_dataloaders', [dl]):
        it = gl._loader._iterator
        if it is not None:
            it._shutdown_workers()
    assert n > 40 and n_cont > 20
    # the txt output of the same run parses
    txt = tmp_path / 'txt'
    cli(txt, ['--output-format', 'txt'])
    lines = 0
    for name in sorted(os.listdir(txt)):
        if not name.endswith('.txt'):
            continue
        # (numpy wraps a long positions array over several lines: a record starts at its tag)
        for line in re.split(r'\n(?=is_random_next: )', (txt / name).read_text()):
            if not line:
                continue
            head, rest = line.split(' - [CLS] ', 1)
            assert head in ('is_random_next: True', 'is_random_next: False')
            ab, rest = rest.split(' [SEP] - masked_lm_positions: [', 1)
            a, b = ab.split(' [SEP] ')
            p_str, rest = rest.split('] - masked_lm_labels: ', 1)
            l_str, nt = rest.rsplit(' - ', 1)
            pos = [int(x) for x in p_str.split()]
            assert int(nt) == len(a.split()) + len(b.split()) + 3
            _row_whole_words(ctx, cv, a, b, pos, l_str.split())
            lines += 1
    assert lines == rows
