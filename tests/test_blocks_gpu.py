"""RoBERTa blocks on the GPU: lddl_blocks_plan through `roberta_blocks` and the two
collates through `collate_blocks`, bit for bit against the sequential oracle (blocks_oracle.py)
on hand-built token tables at the shapes where the kernels take another path; the loader
against the helper."""
import ctypes

import numpy as np
import pytest

import blocks_oracle as O

pytestmark = pytest.mark.gpu
K = 2048  # LDDL_BLOCKS_TILE
V = 1000
SP = dict(bos_id=0, eos_id=2, pad_id=1, mask_id=4, vocab_len=V)
IDS = dict(bos=0, eos=2, pad=1, mask_id=4, vocab_len=V)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def plan_table(n, T):
    """sent_len (flag bits on some) and doc_sent_off of n sentences. Everywhere: sentences of T,
    T + 1 and 3T pieces, a document's last sentence of T pieces (len + sep = T + 1), documents
    of one sentence, of empty sentences only and of none, the last one ending in empties. T = 6:
    single-sentence blocks that end at a tile's end (K), one before it (2K - 1) and a block that
    ends one after it (3K + 1). Otherwise: more than K empty sentences across the whole tile
    [K, 2K), which the chain jumps over."""
    rng = np.random.default_rng(131 * n + T)
    ln = rng.integers(0, T // 2 + 2, n)
    fixed = {3: T, 5: T + 1, 7: 3 * T, 9: T, 20: 0, 21: 0, 22: 0, n - 2: 0, n - 1: 0}
    if T == 6:
        fixed.update({K - 1: T, K: 1, 2 * K - 2: T, 2 * K - 1: 1, 3 * K - 2: T, 3 * K - 1: 1,
                      3 * K: 1, 3 * K + 1: T})
    else:
        fixed.update({i: 0 for i in range(K - 2, 2 * K + 3)})
        fixed[K - 3] = 1
    for i, v in fixed.items():
        if 0 <= i < n:
            ln[i] = v
    cuts = {0, n, 10, 11, 20, 23, 23} | set(rng.integers(0, n + 1, n // 7).tolist())
    if T != 6:  # one document around the empties, so that DOC mode jumps over the tile too
        cuts = {c for c in cuts if not K - 3 < c < 2 * K + 4 or c == n}
    dso = sorted(c for c in cuts if c <= n) + [n]  # the repeated n: a document of no sentences
    flag = np.where(np.arange(n) % 3 == 1, 1 << 30, 0)
    return (ln | flag).astype(np.int32), np.array(dso, np.int64)


@pytest.mark.parametrize('T', [1, 6, 126])
@pytest.mark.parametrize('mode', ['full', 'doc'])
@pytest.mark.parametrize('n', [0, 1, K - 1, K, K + 1, 3 * K + 5])
def test_plan_is_the_oracles(n, mode, T):
    from lddl_amd.torch import roberta_blocks
    sent_len, dso = plan_table(n, T)
    P, sep, blocks = O.plan(sent_len, dso, T + 2, mode)
    if n > 3 * K and T != 6:
        assert any(b < K and e > 2 * K for b, e, _ in blocks)  # tile 1 has no entry
    got, nb = roberta_blocks((None, None, dev(sent_len), dev(dso)), T + 2, mode)
    assert nb == len(blocks)
    np.testing.assert_array_equal(got.piece_off.cpu().numpy(), P)
    np.testing.assert_array_equal(got.sent_sep.cpu().numpy()[:n], sep)
    np.testing.assert_array_equal(got.block_sent.cpu().numpy()[:nb + 1],
                                  [b for b, _, _ in blocks] + [n])
    np.testing.assert_array_equal(got.block_len.cpu().numpy()[:nb], [m for _, _, m in blocks])


# sentence lengths per document. At L = 130 and 66: a separator at slot 63 (30 + 32 pieces
# before it) and at slot 64, each behind a sentence that fills a block alone; blocks of 1, 2,
# 65 and 300 sentences (60 pieces, 44 of them behind the LDS table's 256 sentences)
DOCS = [[200], [30, 32], [5, 0, 7], [200], [31, 32], [3, 4], [200], [1, 0] * 32 + [1], [200],
        [1, 0, 0, 0, 0] * 60, [200, 0], [0, 0], [9, 1, 70], [2] * 40]


class Vocab:
    """What collate_blocks reads of a context: a continuation bitmap over V ids."""
    special_ids = {}

    def __init__(self, cont):
        bits = np.zeros((V + 31) // 32, np.uint32)
        for i in np.flatnonzero(cont):
            bits[i >> 5] |= np.uint32(1 << (i & 31))
        self.bits = dev(bits)
        self.cont_bits = (ctypes.c_void_p(self.bits.data_ptr()), V)

    def __len__(self):
        return V


def make_tab(third):
    """The token table as ctx.tokenize lays it out (gaps between the sentences, a flag bit here
    and there) on the host and the device, and the continuation ids (every third id, or none)."""
    cont = np.arange(V) % 3 == 1 if third else np.zeros(V, bool)
    rng = np.random.default_rng(5)
    ids, sent_off, sent_len, dso = [], [], [], [0]
    for doc in DOCS:
        for n in doc:
            sent_off.append(len(ids))
            sent_len.append(n | ((1 << 30) if n % 3 == 1 else 0))
            ids += rng.integers(10, V, n).tolist() + [0] * int(rng.integers(1, 4))
        dso.append(len(sent_len))
    host = (np.array(ids, np.int32), np.array(sent_off + [len(ids)], np.int64),
            np.array(sent_len, np.int32), np.array(dso, np.int64))
    return host, [dev(a) for a in host], cont, Vocab(cont)


@pytest.fixture(scope='module', params=[False, True], ids=['heads', 'third'])
def tab(request):
    return make_tab(request.param)


def run_both(tab, L, mode='full', rows=None, mask=None, span=None, whole_word=False):
    """collate_blocks and the oracle on the same call -> (device dict as numpy, events, the
    oracle's plan); asserts that they agree bit for bit."""
    from lddl_amd.torch import collate_blocks, roberta_blocks, span as S
    host, on_dev, cont, vocab = tab
    P, sep, blocks = O.plan(host[2], host[3], L, mode)
    plan, nb = roberta_blocks(on_dev, L, mode)
    assert nb == len(blocks)
    got = collate_blocks(vocab, on_dev, plan, None if rows is None else dev(np.array(rows)),
                         mask=mask, span=span, whole_word=whole_word, special_ids=SP)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    kw = {}
    if mask:
        kw = dict(mask=(float(np.float32(mask[0])),) + tuple(mask[1:]))
        if span or whole_word:
            sp = S.parse(span or 1).params(mask[0])
            kw.update(cont=cont, p_start=float(sp.p_start), cum=list(sp.cum))
    want, events = O.collate(host[0], host[1], P, sep, blocks, rows, L, **IDS, **kw)
    assert got.keys() == want.keys()
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    return got, events, (P, sep, blocks)


@pytest.mark.parametrize('mode', ['full', 'doc'])
@pytest.mark.parametrize('L', [8, 66, 130])
def test_unmasked_rows_hold_the_tables_kept_pieces(tab, L, mode):
    got, _, (P, sep, _) = run_both(tab, L, mode)
    host = tab[0]
    kept = [host[0][host[1][s] + o] for s in range(len(sep)) for o in range(P[s + 1] - P[s] - sep[s])]
    np.testing.assert_array_equal(got['input_ids'][got['special_tokens_mask'] == 0], kept)
    if mode == 'full' and L > 8:
        assert got['input_ids'][1, 63] == SP['eos_id'] and got['attention_mask'][1, 64] == 1
        assert any(r[64] == SP['eos_id'] and r[65] != SP['pad_id'] for r in got['input_ids'])


@pytest.mark.parametrize('rows', [None, [3], [9, 2, 9, 0, 7]], ids=['all', '1', '5'])
@pytest.mark.parametrize('p', [0.0, 0.15, 1.0])
def test_per_token_masking(tab, rows, p):
    got, _, _ = run_both(tab, 130, rows=rows, mask=(p, 11, 3))
    plain, _, _ = run_both(tab, 130, rows=rows)
    assert (got['labels'][plain['special_tokens_mask'] == 1] == -100).all()
    if p == 0.0:
        assert (got['labels'] == -100).all()
        np.testing.assert_array_equal(got['input_ids'], plain['input_ids'])
    if p == 1.0:
        assert (got['labels'] != -100).sum() == (plain['special_tokens_mask'] == 0).sum()


@pytest.mark.parametrize('L', [8, 66, 130])
@pytest.mark.parametrize('span', [1, 3])
def test_word_masking(tab, L, span):
    got, _, _ = run_both(tab, L, mask=(0.3, 7, 1), span=span)
    plain, _, _ = run_both(tab, L)
    assert (got['labels'][plain['special_tokens_mask'] == 1] == -100).all()
    if span == 1:  # whole_word=True is span=1
        ww, _, _ = run_both(tab, L, mask=(0.3, 7, 1), whole_word=True)
        np.testing.assert_array_equal(ww['input_ids'], got['input_ids'])


SEED = 12


def test_a_seed_that_shows_the_window_edge_and_a_separator():
    """Seed chosen on the CPU with the oracle alone (continuation table, L = 130, FULL, n = 3):
    a masked word across slots 63 / 64 and a span that runs on over a separator."""
    _, events, _ = run_both(make_tab(True), 130, mask=(0.3, SEED, 0), span=3)
    assert events >= {'word across slots 63 / 64', 'span across a separator'}, events


def test_loader_batches_are_the_helper_on_the_same_rows(tmp_path):
    import torch
    from lddl_amd import bpe as B
    from lddl_amd.torch import get_roberta_pretrain_data_loader
    text = ['Document number {} has words. It has {} sentences! Does it end? Yes {}.'.format(
        i, 'many ' * (i % 5), 'and on ' * i) for i in range(23)]
    for k in range(2):
        (tmp_path / '{}.txt'.format(k)).write_text('\n'.join(text[k::2]))
    make = lambda **kw: get_roberta_pretrain_data_loader(  # noqa: E731
        str(tmp_path), (B.SYNTH_VOCAB, B.SYNTH_MERGES), 4, 64, **kw)
    for kw in (dict(), dict(mode='doc', span=3)):
        a, b = make(**kw), make(**kw)
        e0, e1, again = list(a), list(a), list(b)
        assert len(e0) == len(e1) > 1 and all(x['input_ids'].shape[1] == 64 for x in e0)
        assert all(torch.equal(x[k], y[k]) for x, y in zip(e0, again) for k in x)
        table, plan, n = a.plan_round(a.files)
        assert sum(x['input_ids'].shape[0] for x in e0) == n
        for epoch, batches in enumerate((e0, e1)):
            perm = torch.from_numpy(a.order(epoch, 0, n)).cuda()
            for step, x in enumerate(batches):
                want = a.collate(table, plan, perm[4 * step:4 * step + 4], epoch, step)
                assert all(torch.equal(x[k], want[k]) for k in x)
        # two epochs: the same blocks in another order under other masks
        sizes = lambda e: sorted(v for x in e for v in x['attention_mask'].sum(1).tolist())  # noqa: E731
        assert sizes(e0) == sizes(e1)
        assert not all(torch.equal(x['labels'], y['labels']) for x, y in zip(e0, e1))
