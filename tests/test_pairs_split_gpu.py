"""The split replay plan (head and tail partition ranges, LDDL_PLAN_SPLIT forcing the cut at
small sizes): every path gives the output of the one-range plan, bit for bit - against the
reference goldens where they have enough partitions, else against the oracle."""
import os

import numpy as np
import pytest
import torch

import test_pairs_gpu as TP
from alloc_util import OWN_ARENA, allocated, needs_torch_arena
from conftest import VOCAB_UNCASED
from test_pairs_gpu import ctx, docs_dev  # noqa: F401  (module-scoped fixtures)

pytestmark = pytest.mark.gpu

KEYS = ('tokens', 'num_tokens', 'len_a', 'pos', 'labels')
N_PART = {'s128_mask': 5, 's512_mask': 2, 's64_mask_ratio': 2}


def split_values(n_part):
    return sorted({1, max(n_part - 1, 1), n_part, n_part + 5})


@pytest.mark.parametrize('name', sorted(N_PART))
def test_split_goldens(name, ctx, docs_dev, monkeypatch):  # noqa: F811
    """Head of 1, of n_part - 1 and of >= n_part partitions (an empty tail range) against the
    reference goldens."""
    for k in split_values(N_PART[name]):
        monkeypatch.setenv('LDDL_PLAN_SPLIT', str(k))
        TP.test_pairs_golden_gpu(name, ctx, docs_dev)


def oracle_batch(vocab, text, sent_off, doc_sent_off, part, seeds, dup, seq, ratio=0.15):
    """The oracle over every partition, after the reference's dropping of empty sentences and
    documents; the concatenated columns and the partitions' pair offsets."""
    from oracle import oracle as O
    tok = O.Tokenizer(vocab)
    e_ids, e_off = tok.tokenize(text, sent_off)
    lens = np.diff(e_off)
    special = [tok.token_id(t) for t in ('[CLS]', '[SEP]', '[MASK]')]
    exp = {k: [np.zeros(0, np.int64)] for k in KEYS}
    part_off = [0]
    for p in range(len(part) - 1):
        docs = [[s for s in range(doc_sent_off[d], doc_sent_off[d + 1]) if lens[s] > 0]
                for d in range(part[p], part[p + 1])]
        docs = [d for d in docs if d]
        n = 0
        if docs:
            ks = [s for d in docs for s in d]
            k_off = np.concatenate([[0], np.cumsum([lens[s] for s in ks])]).astype(np.int64)
            k_ids = np.concatenate([e_ids[e_off[s]:e_off[s + 1]] for s in ks]).astype(np.int32)
            k_doc = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
            out = O.partition_pairs(k_doc, k_off, k_ids, int(seeds[p]), dup, seq, True,
                                    tok.vocab_size, *special, masked_lm_ratio=ratio)
            for k in KEYS:
                exp[k].append(np.asarray(out[k]).astype(np.int64))
            n = len(out['len_a'])
        part_off.append(part_off[-1] + n)
    return {k: np.concatenate(v) for k, v in exp.items()}, np.asarray(part_off, np.int64)


def check_batch(pb, exp, part_off):
    out = pb.to_host()
    for k in KEYS:
        assert np.array_equal(np.asarray(out[k]).astype(np.int64), exp[k]), k
    assert np.array_equal(out['part_off'], part_off)
    # exact-length, contiguous columns whatever buffers they were gathered into
    n = len(exp['len_a'])
    assert pb.len_a.numel() == n and pb.tok_off.numel() == n + 1 and pb.pos_off.numel() == n + 1
    assert pb.tokens.numel() == len(exp['tokens']) and pb.pos.numel() == len(exp['pos'])
    assert int(out['tok_off'][-1]) == len(exp['tokens']) and int(out['pos_off'][-1]) == len(exp['pos'])
    for t in (pb.tokens, pb.tok_off, pb.len_a, pb.is_random_next, pb.pos, pb.labels, pb.pos_off):
        assert t.is_contiguous()


@pytest.fixture(scope='module')
def golden_docs():
    g = TP.load('documents_uncased.npz')
    return g['text'].copy(), g['sent_off'], g['line_sent_off']


def golden_doc_inputs(docs_dev, part, seeds):  # noqa: F811
    return dict(sent_off=docs_dev['sent_off'], ids=docs_dev['ids'], sent_len=docs_dev['sent_len'],
                doc_sent_off=docs_dev['doc_sent_off'],
                part_doc_off=torch.from_numpy(np.asarray(part, np.int64)).cuda(),
                part_seed=torch.from_numpy(np.asarray(seeds, np.int64)).cuda())


@pytest.mark.parametrize('seq,dup,ratio', [(512, 3, 0.15), (64, 4, 0.3)])
def test_split_eight_partitions_vs_oracle(ctx, docs_dev, golden_docs, monkeypatch, seq, dup, ratio):  # noqa: F811
    """The golden documents as 8 partitions (the seq 512 and seq 64 goldens have two): 2-byte
    draws and the long-pair mask replay at seq 512, register draws at seq 64; every head size
    that differs in kind (1, interior, n_part - 1, n_part, beyond) against the oracle."""
    from lddl_amd.pairs import make_pairs
    text, sent_off, line_off = golden_docs
    n_lines = len(line_off) - 1
    part = np.linspace(0, n_lines, 9).astype(np.int64)
    seeds = np.arange(31, 39, dtype=np.int64)
    exp, part_off = oracle_batch(VOCAB_UNCASED, text, sent_off, line_off, part, seeds, dup, seq, ratio)
    assert len(exp['len_a']) > 0
    kw = golden_doc_inputs(docs_dev, part, seeds)
    for k in (0, 1, 3, 7, 8, 13):
        monkeypatch.setenv('LDDL_PLAN_SPLIT', str(k))
        tr = {}
        pb = make_pairs(ctx, seq=seq, dup=dup, masking=True, masked_lm_ratio=ratio, _trace=tr, **kw)
        # (a small head may predict too little for the rest: then the exact-size copy path runs)
        assert tr['split'] == (1 if k else 0) and tr['path'] in (('tail', 'copy') if k else ('full',)), (k, tr)
        check_batch(pb, exp, part_off)


def test_split_four_byte_ids_vs_oracle(tmp_path, monkeypatch):
    """A vocab beyond 65,534 entries: the int32 gather and labels over two ranges."""
    from lddl_amd import synth
    from lddl_amd.context import Context
    from lddl_amd.pairs import make_pairs
    with open(VOCAB_UNCASED) as f:
        lines = f.read().splitlines()
    big = tmp_path / 'vocab_big.txt'
    big.write_text('\n'.join(lines + ['[extra{}]'.format(i) for i in range(40000)]) + '\n')
    ctx4 = Context(str(big))
    assert ctx4.id_bytes == 4
    corp = synth.generate(seed=191, n_bytes=400_000, threads=4)
    part = np.linspace(0, corp.n_doc, 7).astype(np.int64)
    seeds = np.arange(11, 17, dtype=np.int64)
    exp, part_off = oracle_batch(str(big), corp.text, corp.sent_off, corp.doc_sent_off, part, seeds,
                                 2, 128)
    so = torch.from_numpy(corp.sent_off).cuda()
    ids, sl = ctx4.tokenize(torch.from_numpy(corp.text).cuda(), so)
    monkeypatch.setenv('LDDL_PLAN_SPLIT', '2')
    tr = {}
    pb = make_pairs(ctx4, so, ids, sl, torch.from_numpy(corp.doc_sent_off).cuda(),
                    torch.from_numpy(part).cuda(), torch.from_numpy(seeds).cuda(), seq=128, dup=2,
                    masking=True, _trace=tr)
    assert tr['split'] == 1 and tr['head_valid'] == 1 and tr['path'] in ('tail', 'copy')
    check_batch(pb, exp, part_off)


def test_split_empty_partitions(ctx, docs_dev, golden_docs, monkeypatch):  # noqa: F811
    """Empty partitions (repeated document offsets) at the start, at the cut and at the end: a
    head range without pairs, a tail range without pairs, and empty partitions either side of
    the cut."""
    from lddl_amd.pairs import make_pairs
    text, sent_off, line_off = golden_docs
    n = len(line_off) - 1
    part = np.asarray([0, 0, n // 3, n // 3, n // 3, 2 * n // 3, n, n], np.int64)  # 7 partitions
    seeds = np.arange(51, 58, dtype=np.int64)
    exp, part_off = oracle_batch(VOCAB_UNCASED, text, sent_off, line_off, part, seeds, 2, 128)
    assert part_off[1] == 0 and part_off[-1] == part_off[-2] and part_off[3] == part_off[4]
    kw = golden_doc_inputs(docs_dev, part, seeds)
    for k, head_pairs in ((1, 0), (2, part_off[2]), (3, part_off[3]), (4, part_off[4]),
                          (6, part_off[6]), (7, part_off[7])):
        monkeypatch.setenv('LDDL_PLAN_SPLIT', str(k))
        tr = {}
        pb = make_pairs(ctx, seq=128, dup=2, masking=True, _trace=tr, **kw)
        assert tr['split'] == 1 and tr['head_pairs'] == head_pairs and tr['head_valid'] == 1, (k, tr)
        assert tr['path'] in ('tail', 'copy'), (k, tr)
        check_batch(pb, exp, part_off)


def test_split_pool_overflow_replans(ctx, docs_dev, monkeypatch):  # noqa: F811
    """A mask pool that overflows under a split plan: everything is planned again in one range,
    the head range is reported void and the output is the golden. Pool 100: the head range
    overflows it itself (nothing downstream runs on it); pool 40000: about half of what the case
    needs (2,910 pairs of ~16 mask entries) and more than its first partition's third, so the
    head range can be resolved and gathered before the tail range overflows."""
    from lddl_amd.pairs import make_pairs
    g, kw = TP.case_inputs('s128_mask', docs_dev)
    for k, pool in ((1, 100), (4, 100), (1, 40000)):
        monkeypatch.setenv('LDDL_AMD_MASK_POOL', str(pool))
        monkeypatch.setenv('LDDL_PLAN_SPLIT', str(k))
        tr = {}
        out = make_pairs(ctx, _trace=tr, **kw).to_host()
        assert tr['split'] == 1 and tr['head_valid'] == 0 and tr['path'] == 'full', tr
        np.testing.assert_array_equal(out['num_tokens'], g['num_tokens'])
        np.testing.assert_array_equal(out['pos_off'], g['pos_off'])
        np.testing.assert_array_equal(out['pos'], g['pos'])
        np.testing.assert_array_equal(out['labels'], g['labels'])
        TP.test_pairs_golden_gpu('s128_mask', ctx, docs_dev)


def test_split_short_capacity_copies_head(ctx, docs_dev, monkeypatch):  # noqa: F811
    """Output buffers that turn out too small for the whole plan: exact ones are allocated, the
    gathered head range is copied over and the tail gathered behind it."""
    from lddl_amd.pairs import make_pairs
    g, kw = TP.case_inputs('s128_mask', docs_dev)
    monkeypatch.setenv('LDDL_PLAN_SPLIT', '2')
    tr, tr0 = {}, {}
    pb = make_pairs(ctx, _capacity_scale=0.5, _trace=tr, **kw)
    assert tr['split'] == 1 and tr['head_valid'] == 1 and tr['path'] == 'copy', tr
    monkeypatch.setenv('LDDL_PLAN_SPLIT', '0')
    ref = make_pairs(ctx, _trace=tr0, **kw)
    assert tr0['path'] == 'full'
    a, b = pb.to_host(), ref.to_host()
    assert sorted(a) == sorted(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    np.testing.assert_array_equal(a['pos'], g['pos'])
    np.testing.assert_array_equal(a['labels'], g['labels'])
    np.testing.assert_array_equal(a['num_tokens'], g['num_tokens'])


@pytest.mark.parametrize('mode', ['nomask', 'native'])
def test_split_knob_leaves_other_paths_alone(ctx, docs_dev, monkeypatch, mode):  # noqa: F811
    """Without masking and with the native RNG the knob is accepted and the one-range path
    runs: the output equals the one with the split switched off."""
    from lddl_amd.pairs import make_pairs
    _, kw = TP.case_inputs('s128_mask', docs_dev)
    if mode == 'nomask':
        kw['masking'] = False
    else:
        kw['rng'] = 'native'
    monkeypatch.setenv('LDDL_PLAN_SPLIT', '0')
    ref = make_pairs(ctx, **kw).to_host()
    monkeypatch.setenv('LDDL_PLAN_SPLIT', '2')
    tr = {}
    out = make_pairs(ctx, _trace=tr, **kw).to_host()
    assert tr['split'] == 0 and tr['path'] == 'full'
    assert sorted(out) == sorted(ref)
    for k in ref:
        np.testing.assert_array_equal(out[k], ref[k])
    if mode == 'nomask':
        monkeypatch.delenv('LDDL_PLAN_SPLIT')
        TP.test_pairs_golden_gpu('s128_nomask', ctx, docs_dev)


@pytest.mark.parametrize('value', ['-2', 'x', '3x', '', '1.5'])
def test_split_rejects_unsupported_knob(ctx, docs_dev, monkeypatch, value):  # noqa: F811
    """Anything but -1, 0 or a partition count fails the call with the knob's name, keeps none of
    the allocator's memory, and the same context then plans the case."""
    from lddl_amd.pairs import make_pairs
    _, kw = TP.case_inputs('s128_mask', docs_dev)
    monkeypatch.setenv('LDDL_PLAN_SPLIT', value)
    before = allocated()
    with pytest.raises(Exception, match='LDDL_PLAN_SPLIT'):
        make_pairs(ctx, **kw)
    if not OWN_ARENA:
        assert allocated() == before
    monkeypatch.setenv('LDDL_PLAN_SPLIT', '-1')
    TP.test_pairs_golden_gpu('s128_mask', ctx, docs_dev)


@needs_torch_arena
def test_failed_split_plan_returns_its_blocks(ctx, docs_dev, monkeypatch):  # noqa: F811
    """A plan that fails after the compaction took its blocks, with the split forced, gives every
    block back; so does a split plan that succeeds, once its batch is deleted."""
    from lddl_amd.pairs import make_pairs
    monkeypatch.setenv('LDDL_PLAN_SPLIT', '1')
    _, kw = TP.case_inputs('s512_nomask_short', docs_dev)
    kw.update(masking=False, seq=600)
    before = allocated()
    with pytest.raises(Exception, match='replay planner supports target_seq_length <= 512'):
        make_pairs(ctx, **kw)
    assert allocated() == before
    _, kw = TP.case_inputs('s128_mask', docs_dev)
    for env in ({}, {'LDDL_AMD_MASK_POOL': '100'}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        pb = make_pairs(ctx, **kw)
        assert pb.tokens.numel() > 0 and allocated() > before
        del pb
        assert allocated() == before


def test_split_back_to_back(ctx, docs_dev, monkeypatch):  # noqa: F811
    """Two split plans in a row on one context, no synchronisation between them: the side stream
    and the arena's blocks are reused across the calls."""
    from lddl_amd.pairs import make_pairs
    g1, kw1 = TP.case_inputs('s128_mask', docs_dev)
    g2, kw2 = TP.case_inputs('s64_mask_ratio', docs_dev)
    monkeypatch.setenv('LDDL_PLAN_SPLIT', '1')
    pb1 = make_pairs(ctx, **kw1)
    pb2 = make_pairs(ctx, **kw2)
    pb3 = make_pairs(ctx, **kw1)
    for pb, g in ((pb1, g1), (pb2, g2), (pb3, g1)):
        out = pb.to_host()
        np.testing.assert_array_equal(out['num_tokens'], g['num_tokens'])
        np.testing.assert_array_equal(out['pos_off'], g['pos_off'])
        np.testing.assert_array_equal(out['pos'], g['pos'])
        np.testing.assert_array_equal(out['labels'], g['labels'])
    for a, b in zip(pb1.to_host().values(), pb3.to_host().values()):
        np.testing.assert_array_equal(a, b)
