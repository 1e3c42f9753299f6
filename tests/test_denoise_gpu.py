"""BART denoising on the GPU: lddl_bart_denoise through `bart_denoise`, bit for bit
against the sequential oracle (denoise_oracle.py) on hand-built token tables at the shapes
where the kernel takes another path, and the loader against the helper."""
import os

import numpy as np
import pytest

from conftest import REPO
from denoise_oracle import S_MAX, denoise

pytestmark = pytest.mark.gpu
VOCAB = os.path.join(REPO, 'lddl_amd', 'assets', 'vocab_synth_uncased_30522.txt')
# sentence lengths per sample: 0, 1, 62, 63, 64, 65 and 130 pieces; 1, 2, 64 and 65 sentences;
# the tail unit (one-piece and longer sentences); empty sentences
DOCS = [[], [1], [62], [20, 43], [64], [30, 0, 35], [50, 40, 40], [1] * 64, [2] * 65,
        [1] * (S_MAX + 40), [0, 0, 5, 0], [3, 1] * 140, [33] * 4]
LENGTHS = [sum(d) for d in DOCS]
EVENTS = {'span across slots 63 / 64', 'word straddles two windows',
          'span crosses a sentence boundary', 'two adjacent spans, two masks'}
WEIGHTS = {'poisson': None, 'onehot1': [0, 1], 'onehot16': [0] * 16 + [1]}


def table(cont_share):
    """(ids, sent_off, sent_len, doc_sent_off) as ctx.tokenize lays them out: gaps between the
    sentences, a flag bit above the length here and there."""
    with open(VOCAB, encoding='utf-8') as f:
        cont = np.array([t.startswith('##') and len(t) > 2 for t in f.read().split('\n')])
    rng = np.random.default_rng(5)
    pool = {False: np.flatnonzero(~cont)[1000:], True: np.flatnonzero(cont)}
    ids, sent_off, sent_len, dso = [], [], [], [0]
    for doc in DOCS:
        for n in doc:
            sent_off.append(len(ids))
            sent_len.append(n | ((1 << 30) if n % 3 == 1 else 0))
            ids += [int(rng.choice(pool[bool(rng.random() < cont_share)])) for _ in range(n)]
            ids += [0] * int(rng.integers(1, 4))
        dso.append(len(sent_len))
    return (np.array(ids, np.int32), np.array(sent_off + [len(ids)], np.int64),
            np.array(sent_len, np.int32), np.array(dso, np.int64)), cont


@pytest.fixture(scope='module')
def ctx():
    from lddl_amd.context import Context
    return Context(VOCAB)


def on_device(ctx, share):
    import torch
    host, cont = table(share)
    return host, cont, [torch.from_numpy(a).to(ctx.device) for a in host]


@pytest.fixture(scope='module', params=[0.0, 1 / 3], ids=['heads', 'third'])
def tab(request, ctx):
    return on_device(ctx, request.param)


def run_both(ctx, tab, rows, L, ratio=0.3, weights=None, permute=1.0, rnd=0.1, seed=11,
             counter=3, params=None):
    """bart_denoise and the oracle on the same call -> (device dict as numpy, oracle dict,
    events); asserts that they agree bit for bit."""
    import torch
    from lddl_amd.torch import bart_denoise, denoise as D
    host, cont, dev = tab
    w = D.poisson_weights() if weights is None else weights
    if ratio == 'max':  # what every head starting a span deletes or replaces
        q = 1 - np.cumsum(np.asarray(w, np.float64) / np.sum(w))[:-1]
        ratio = float(1 - np.prod(1 - q))
    dp = params or D.make_params(ratio, w)
    d_rows = None if rows is None else torch.tensor(rows, dtype=torch.int64, device=ctx.device)
    got = bart_denoise(ctx, *dev, rows=d_rows, seq_len=L, mask=(ratio, seed, counter),
                       permute_sentence_ratio=permute, random_ratio=rnd, params=dp)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    sp = ctx.special_ids
    want, events = denoise(
        *host, rows, L, cont, bos=sp['[CLS]'], eos=sp['[SEP]'], pad=sp['[PAD]'],
        mask_id=sp['[MASK]'], dec_start=sp['[SEP]'], ignore=-100, vocab_len=len(ctx), seed=seed,
        counter=counter, stride=L, permute_p=float(np.float32(permute)),
        random_ratio=float(np.float32(rnd)), p_start=float(dp.p_start), cum=list(dp.cum))
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        assert got[k].dtype == want[k].dtype
    return got, want, events


@pytest.mark.parametrize('cut', [0, 5], ids=['fits', 'cut'])
@pytest.mark.parametrize('d', range(7))
def test_one_sample_at_its_own_length(ctx, tab, d, cut):
    run_both(ctx, tab, [d], max(LENGTHS[d] + 2 - cut, 2))


@pytest.mark.parametrize('ratio,weights,permute,rnd', [
    (0.0, 'poisson', 0.0, 0.0), (0.0, 'poisson', 1.0, 0.1), (0.3, 'poisson', 1.0, 0.1),
    ('max', 'poisson', 0.5, 1.0), (0.3, 'onehot1', 0.5, 0.0), ('max', 'onehot1', 1.0, 0.1),
    (0.3, 'onehot16', 1.0, 1.0), ('max', 'onehot16', 0.0, 0.1)])
def test_noise_settings_over_every_sample(ctx, tab, ratio, weights, permute, rnd):
    L = 600  # every sample whole: the tail units hold pieces
    got, _, _ = run_both(ctx, tab, None, L, ratio, WEIGHTS[weights], permute, rnd)
    plain, _, _ = run_both(ctx, tab, None, L, 0.0, None, 0.0, 0.0)
    np.testing.assert_array_equal(got['labels'], plain['labels'])  # never depends on the noise
    real = plain['labels'] != -100
    np.testing.assert_array_equal(plain['input_ids'][real], plain['labels'][real])
    if ratio == 0.0:  # the permuted sample: the same pieces, nothing deleted or inserted
        np.testing.assert_array_equal(got['src_lengths'], np.array(LENGTHS) + 2)
        np.testing.assert_array_equal(np.sort(got['input_ids'], 1), np.sort(plain['input_ids'], 1))


@pytest.mark.parametrize('rows', [[9], [8, 3, 11, 3, 0], [11, 10, 9, 9, 6, 1, 0, 7, 5]],
                         ids=['1', '5', '9'])
def test_rows_reordered_and_repeated_with_the_budget_inside_the_tail(ctx, tab, rows):
    run_both(ctx, tab, rows, 280)  # 278 pieces: 23 sentences of sample 9's tail unit
    with pytest.raises(IndexError):
        run_both(ctx, tab, [0, len(DOCS)], 8)


def test_an_insertion_before_every_word_overflows_the_row(ctx, tab):
    from lddl_amd._native import DenoiseParams
    dp = DenoiseParams()
    dp.n, dp.p_start = 1, 1.0
    dp.cum[:] = [1.0] * 16  # every head starts a span, every span has length 0
    for d in (1, 4, 6):
        got, _, _ = run_both(ctx, tab, [d], LENGTHS[d] + 2, params=dp)
        if not tab[1][tab[0][0]].any():  # every piece a head: two ids for each
            assert got['src_lengths'][0] == 2 * LENGTHS[d] + 2 > LENGTHS[d] + 2


def test_a_seed_that_shows_the_window_edges(ctx):
    """Seed chosen on the CPU with the oracle alone (continuation table, samples 8 and 12): a
    span across slots 63 / 64, a word over two windows, a span over a sentence boundary after
    the permutation and two adjacent spans with a mask each."""
    _, _, events = run_both(ctx, on_device(ctx, 1 / 3), [8, 12], 136, seed=SEED, counter=0)
    assert set().union(*events) >= EVENTS, events


SEED = 1


def test_loader_batches_are_the_helper_on_the_same_rows(ctx, tmp_path):
    import torch
    from lddl_amd.torch import get_bart_pretrain_data_loader
    text = ['Chunk number {} has words. It has {} sentences! Does it end? Yes {}.'.format(
        i, 'many ' * (i % 5), 'and on ' * i) for i in range(11)]
    for k in range(2):
        (tmp_path / '{}.txt'.format(k)).write_text('\n'.join(text[k::2]))
    make = lambda **kw: get_bart_pretrain_data_loader(str(tmp_path), VOCAB, 4, 64, **kw)  # noqa: E731
    a, b = make(), make()
    e0, e1, again = list(a), list(a), list(b)
    assert [x['input_ids'].shape[0] for x in e0] == [4, 4, 3] and len(e1) == 3
    assert all(torch.equal(x[k], y[k]) for x, y in zip(e0, again) for k in x)
    assert any(x['input_ids'].shape != y['input_ids'].shape or
               not torch.equal(x['input_ids'], y['input_ids']) for x, y in zip(e0, e1))
    tbl, n_pieces = a.tokenize_round(a.files)
    assert len(n_pieces) == 11
    perm = torch.from_numpy(a.order(0, 0, 11)).to(ctx.device)
    for step, x in enumerate(e0):
        want = a.denoise(tbl, perm[4 * step:4 * step + 4], x['input_ids'].shape[1], 0, step)
        assert all(torch.equal(x[k], want[k]) for k in x)
        assert (x['labels'][:, 0] == ctx.special_ids['[CLS]']).all()
