"""T5 span corruption on the GPU: `t5_corrupt` bit for bit against t5_oracle.py on
a hand-built token table at the edge lengths, counts and widths; the loader against the helper."""
import numpy as np
import pytest

import blocks_oracle as BO
import t5_oracle as O
from test_t5_host import TIE, restore

pytestmark = pytest.mark.gpu
V, L = 1000, 602  # T = 600
# rows of exactly these lengths in both modes (a sentence of n pieces before one that fills a
# block alone: 600 tokens), N - 1 and M - 1 on both sides of a window's edge; then separators
# inside a FULL block, empty sentences, and 300 one-piece sentences (44 behind the LDS table)
LENGTHS = [1, 2, 3, 4, 63, 64, 65, 66, 129, 130, 500]
DOCS = [[n, 600] for n in LENGTHS] + [[5, 0, 7], [9], [0, 0], [600], [1, 0, 0] * 300, [600, 0]]
# (noise_density, mean_noise_span_length, n_sentinels): the defaults; N clamped to 1 (k = 1:
# nothing selected); N clamped to n - 1 and k by n - N; k = N (every noise item opens a segment)
# and clipped by 256 sentinels at n = 600; k clipped by 3 sentinels and by 1
CONFIGS = [(0.15, 3.0, 100), (0.00002, 3.0, 100), (0.99, 64.0, 100), (0.5, 1.0, 256),
           (0.3, 1.0, 3), (0.15, 3.0, 1)]
TIE_BELOW = 2529  # as TIE: two equal non-noise keys below the threshold
Vocab = type('Vocab', (), {'special_ids': {}, '__len__': lambda self: V})  # what t5_corrupt reads


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope='module')
def tab():
    """ctx.tokenize's layout (gaps, flag bits) on the host and the device; the plans so far."""
    rng = np.random.default_rng(31)
    ids, sent_off, sent_len, dso = [], [], [], [0]
    for doc in DOCS:
        for n in doc:
            sent_off.append(len(ids))
            sent_len.append(n | ((1 << 30) if n % 3 == 1 else 0))
            ids += rng.integers(10, V, n).tolist() + [0] * int(rng.integers(1, 4))
        dso.append(len(sent_len))
    host = (np.array(ids, np.int32), np.array(sent_off + [len(ids)], np.int64),
            np.array(sent_len, np.int32), np.array(dso, np.int64))
    return host, [dev(a) for a in host], {}


def run_both(tab, mode='doc', rows=None, noise=(11, 3), cfg=CONFIGS[0], cut=0):
    """t5_corrupt and the oracle on the same call -> (device dict as numpy, the rows' tokens,
    k per row); asserts that they agree bit for bit. cut narrows both widths."""
    from lddl_amd.torch import roberta_blocks, t5_corrupt
    host, on_dev, plans = tab
    if mode not in plans:
        plans[mode] = BO.plan(host[2], host[3], L, mode), roberta_blocks(on_dev, L, mode)
    (P, sep, blocks), (plan, nb) = plans[mode]
    assert nb == len(blocks)
    q = O.fixed(*cfg)
    in_len, tgt_len = (w - cut for w in O.lengths(L - 2, *q))
    got = t5_corrupt(Vocab(), on_dev, plan, None if rows is None else dev(np.array(rows)),
                     noise, *cfg, **(dict(in_len=in_len, tgt_len=tgt_len) if cut else {}),
                     special_ids=dict(eos_id=2, pad_id=1))
    got = {k: v.cpu().numpy() for k, v in got.items()}
    want, rws = O.corrupt(host[0], host[1], P, sep, blocks, rows, L, in_len, tgt_len, q,
                          sentinel_first=V + cfg[2] - 1, eos=2, pad=1, dec_start=1, ignore=-100,
                          seed=noise[0], counter=noise[1])
    assert got.keys() == want.keys()
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    return got, [t for t, _ in rws], [O.counts(len(t), *q)[1] for t, _ in rws]


@pytest.mark.parametrize('mode', ['full', 'doc'])
@pytest.mark.parametrize('cfg', CONFIGS)
def test_every_block_at_the_default_widths(tab, cfg, mode):
    got, toks, ks = run_both(tab, mode, cfg=cfg)
    ns = [len(t) for t in toks]
    assert set(LENGTHS) | {600} <= set(ns) and len(ns) % 4  # a partial workgroup
    assert any(2 in t[:-1] for t in toks) == (mode == 'full')  # a separator inside a row
    assert got['input_ids'].shape[1:] + got['labels'].shape[1:] == (
        got['src_lengths'].max(), got['tgt_lengths'].max())
    if cfg == CONFIGS[3]:
        assert max(ks) == 256 and ks[ns.index(130)] == 65
    for i, (t, k) in enumerate(zip(toks, ks)):  # the device rows restore their tokens
        s, e = got['src_lengths'][i], got['tgt_lengths'][i]
        assert restore(got['input_ids'][i, :s - 1].tolist(), got['labels'][i, :e - 1].tolist(),
                       V + cfg[2] - 1, k) == t


@pytest.mark.parametrize('cut', [0, 3])
@pytest.mark.parametrize('rows', [[10], [21, 3, 21, 0, 7], [1, 3, 5, 7, 9, 11, 13, 15, 23]])
def test_rows_batches_and_narrow_widths(tab, rows, cut):
    got, _, _ = run_both(tab, rows=rows, cut=cut)
    if cut and len(rows) > 1:  # the 600-token rows overflow: eos last, lengths untruncated
        over = got['src_lengths'] > got['input_ids'].shape[1]
        assert over.any() and (got['input_ids'][over, -1] == 2).all()
        assert (got['labels'][got['tgt_lengths'] > got['labels'].shape[1], -1] == 2).all()


@pytest.mark.parametrize('seed', [TIE[0], TIE_BELOW])
def test_equal_keys(tab, seed):  # row 0 is the block of TIE's n tokens
    _, toks, _ = run_both(tab, rows=[2 * LENGTHS.index(TIE[2])], noise=(seed, TIE[1]))
    assert len(toks[0]) == TIE[2]


def test_labels_are_equal_iff_the_noise_is(tab):
    lab = [run_both(tab, rows=[0, 8, 20, 21], noise=nz)[0]['labels']
           for nz in ((5, 6), (5, 6), (5, 7), (6, 6))]
    assert (lab[0] == lab[1]).all() and (lab[0] != lab[2]).any() and (lab[0] != lab[3]).any()


def test_loader_batches_are_the_helper_on_the_same_rows(tmp_path):
    import torch
    from lddl_amd import bpe as B
    from lddl_amd.torch import get_t5_pretrain_data_loader, t5_lengths, t5_tokens_length
    for k in range(2):
        (tmp_path / '{}.txt'.format(k)).write_text('\n'.join(
            'Document number {} has words. It has {} sentences! Does it end? Yes {}.'.format(
                i, 'many ' * (i % 5), 'and on ' * i) for i in range(k, 23, 2)))
    for mode, nz in (('full', {}), ('doc', dict(mean_noise_span_length=2.0, n_sentinels=5))):
        a = get_t5_pretrain_data_loader(str(tmp_path), (B.SYNTH_VOCAB, B.SYNTH_MERGES), 4, 64,
                                        mode, **nz)
        epochs = list(a), list(a)
        table, plan, n = a.plan_round(a.files)
        assert plan.seq_len == t5_tokens_length(64, **nz) + 2
        widths = t5_lengths(plan.seq_len - 2, **nz)
        for epoch, batches in enumerate(epochs):
            assert sum(x['input_ids'].shape[0] for x in batches) == n and len(batches) > 1
            perm = torch.from_numpy(a.order(epoch, 0, n)).cuda()
            for step, x in enumerate(batches):
                assert (x['input_ids'].shape[1], x['labels'].shape[1]) == widths <= (64, 64)
                want = a.collate(table, plan, perm[4 * step:4 * step + 4], epoch, step)
                assert all(torch.equal(x[k], want[k]) for k in x)
