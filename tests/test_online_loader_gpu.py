"""The online loader (lddl_amd/torch/online.py): an epoch is exactly the preprocessor's pairs,
cut into one-bin batches of the right width; determinism; dynamic and static masking; two ranks
over gloo on one GPU."""
import collections
import os
import socket
from datetime import timedelta
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import VOCAB_UNCASED

pytestmark = pytest.mark.gpu

SEQ, BIN, NBINS = 128, 32, 4
BASE = dict(vocab_file=VOCAB_UNCASED, target_seq_length=SEQ, bin_size=BIN, block_size=70_000,
            base_seed=777, read_threads=2)


def _write_corpus(root):
    """~400 KB of synthetic documents, one per line, as a `source` directory of three files of
    (almost) equal size."""
    from lddl_amd import synth
    text, doc_off = synth.generate_doc_text(seed=99, n_bytes=400_000, nonascii_frac=0.02, threads=2)
    raw = text.tobytes()
    docs = [raw[doc_off[d]:doc_off[d + 1]] for d in range(len(doc_off) - 1)]
    src = os.path.join(root, 'source')
    os.makedirs(src)
    third = (len(docs) + 2) // 3
    for k in range(3):
        with open(os.path.join(src, 'part_{}.txt'.format(k)), 'wb') as f:
            for i, d in enumerate(docs[k * third:(k + 1) * third]):
                f.write('doc-{}-{} '.format(k, i).encode() + d + b'\n')
    return src


@pytest.fixture(scope='module')
def src(tmp_path_factory):
    return _write_corpus(str(tmp_path_factory.mktemp('online')))


def _ns(src, seed, masking=False, rng='native', gpu_batch_bytes=64 << 20):
    """The preprocessor's namespace for the same corpus, written out independently."""
    return SimpleNamespace(wikipedia=None, books=src, common_crawl=None, wikipedia_lang='en',
                           block_size=BASE['block_size'], num_blocks=None, sample_ratio=1.0,
                           seed=seed, target_seq_length=SEQ, duplicate_factor=1, masking=masking,
                           short_seq_prob=0.1, masked_lm_ratio=0.15, rng=rng,
                           whole_word_masking=False, bin_size=BIN,
                           gpu_batch_bytes=gpu_batch_bytes, shuffle_group_bytes=1 << 30,
                           read_threads=2)


_CTX = {}


def _pre_ctx():
    if 'c' not in _CTX:
        from lddl_amd import punkt
        from lddl_amd.context import Context
        from lddl_amd.dask.bert.corpus import punkt_params
        c = _CTX['c'] = Context(VOCAB_UNCASED)
        punkt.set_params(c, punkt_params(SimpleNamespace(punkt_params=None)))
    return _CTX['c']


def _expected(ns, rank=0, world=1):
    """The pairs the preprocessor makes for this rank: a list of (A, B, nsl[, pos, labels])."""
    from lddl_amd.dask.bert.corpus import iter_doc_batches
    from lddl_amd.dask.bert.gpu_batch import make_batch_pairs
    ctx = _pre_ctx()
    out = []
    for partitions, corpus in iter_doc_batches(ns, rank, world):
        h = make_batch_pairs(ctx, ns, partitions, corpus).to_host()
        tok, off, na = h['tokens'].astype(np.int64), h['tok_off'], h['len_a']
        for q in range(len(na)):
            t = tok[off[q]:off[q + 1]]
            s = (t[:na[q]].tobytes(), t[na[q]:].tobytes(), int(h['is_random_next'][q]))
            if ns.masking:
                p0, p1 = h['pos_off'][q], h['pos_off'][q + 1]
                s += (h['pos'][p0:p1].astype(np.int64).tobytes(),
                      h['labels'][p0:p1].astype(np.int64).tobytes())
            out.append(s)
    return out


def _layout(b):
    """(na, nb, num_tokens) per row of a batch, read back from the masks."""
    end = b['attention_mask'].sum(1)
    nb = b['token_type_ids'].sum(1) - 1
    return end - nb - 3, nb, end


def _samples(b, static=False, ignore=-1):
    na, nb, _ = _layout(b)
    ids = b['input_ids'].numpy()
    out = []
    for i in range(ids.shape[0]):
        a, n = int(na[i]), int(nb[i])
        s = (ids[i, 1:1 + a].tobytes(), ids[i, a + 2:a + 2 + n].tobytes(),
             int(b['next_sentence_labels'][i]))
        if static:
            lab = b['labels'][i].numpy()
            pos = np.flatnonzero(lab != ignore)
            s += (pos.astype(np.int64).tobytes(), lab[pos].astype(np.int64).tobytes())
        out.append(s)
    return out


def _epoch(loader):
    return [{k: v.cpu() for k, v in b.items()} for b in loader]


def _bin_of(ntok):
    return np.minimum((np.asarray(ntok) - 1) // BIN, NBINS - 1)


def _make(src, **kw):
    from lddl_amd.torch import get_bert_pretrain_online_data_loader
    args = dict(BASE, books=src, rank=0, world=1)
    args.update(kw)
    return get_bert_pretrain_online_data_loader(**args)


def _check_batches(batches, batch_size, exp):
    """Nothing left out, one bin per batch, L = the rounded longest row, every batch full but at
    most the last of each bin."""
    got = [s for b in batches for s in _samples(b)]
    assert collections.Counter(got) == collections.Counter(exp)
    last = {}
    for k, b in enumerate(batches):
        _, _, end = _layout(b)
        bins = _bin_of(end.numpy())
        assert len(set(bins.tolist())) == 1
        assert b['input_ids'].shape[1] == (int(end.max()) - 1) // 8 * 8 + 8
        assert b['labels'].shape == b['input_ids'].shape and int((b['labels'] != -1).sum()) == 0
        last[int(bins[0])] = k
    short = [k for k, b in enumerate(batches) if b['input_ids'].shape[0] != batch_size]
    assert all(batches[k]['input_ids'].shape[0] < batch_size for k in short)
    assert set(short) <= set(last.values())  # only a bin's last batch may be short


def test_one_epoch_equals_the_preprocessors_pairs(src):
    exp = _expected(_ns(src, 777))
    assert len(exp) > 400
    loader = _make(src, batch_size=32, mlm_probability=0.0, drop_last=False)
    batches = _epoch(loader)
    _check_batches(batches, 32, exp)
    assert loader.dropped_samples == 0 and loader.num_rounds == 1
    with pytest.raises(TypeError):
        len(loader)
    # many rounds, and a batch size that divides no bin's count: the carry crosses rounds
    counts = np.bincount(_bin_of([len(s[0]) // 8 + len(s[1]) // 8 + 3 for s in exp]),
                         minlength=NBINS)
    bs = next(n for n in (37, 41, 43, 47, 53, 59) if all(c % n for c in counts if c))
    loader = _make(src, batch_size=bs, mlm_probability=0.0, drop_last=False,
                   gpu_batch_bytes=100_000)
    batches = _epoch(loader)
    assert loader.num_rounds >= 3
    _check_batches(batches, bs, exp)
    assert sum(b['input_ids'].shape[0] != bs for b in batches) == int((counts > 0).sum())
    # drop_last: the same full batches, the remainders counted
    loader = _make(src, batch_size=bs, mlm_probability=0.0, gpu_batch_bytes=100_000)
    full = _epoch(loader)
    assert all(b['input_ids'].shape[0] == bs for b in full)
    np.testing.assert_array_equal(loader.dropped_per_bin, counts % bs)
    assert loader.dropped_samples == int((counts % bs).sum())
    assert len(full) == int((counts // bs).sum())


def _equal(x, y):
    return len(x) == len(y) and all(
        set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a) for a, b in zip(x, y))


def test_determinism_and_epochs(src):
    kw = dict(batch_size=32, gpu_batch_bytes=150_000)
    a = _make(src, **kw)
    a0, a1 = _epoch(a), _epoch(a)
    b0 = _epoch(_make(src, **kw))
    assert _equal(a0, b0)
    assert _equal(a1, _epoch(_make(src, start_epoch=1, **kw)))
    s0 = collections.Counter(s[:2] for b in _epoch(_make(src, mlm_probability=0.0, **kw))
                             for s in _samples(b))
    s1 = collections.Counter(s[:2] for b in _epoch(_make(src, mlm_probability=0.0, start_epoch=1,
                                                         **kw)) for s in _samples(b))
    assert s0 != s1 and sum((s0 & s1).values()) < 0.9 * sum(s0.values())  # fresh pairs


@pytest.mark.parametrize('ww', [False, True])
def test_dynamic_masking_is_mask_tokens_with_the_documented_key(src, ww):
    from lddl_amd.torch.bert import _mask_tokens, mask_seed
    kw = dict(batch_size=32, gpu_batch_bytes=150_000, start_epoch=2, whole_word_masking=ww)
    plain = _epoch(_make(src, mlm_probability=0.0, **kw))
    masked = _epoch(_make(src, mlm_probability=0.15, **kw))
    assert len(plain) == len(masked) > 8
    ctx = _pre_ctx()
    in_bin = [0] * NBINS
    for p, m in zip(plain, masked):
        na, nb, end = _layout(p)
        b = int(_bin_of(end.numpy())[0])
        x = torch.arange(p['input_ids'].shape[1])[None, :]
        stm = ((x == 0) | (x == (na + 1)[:, None]) | (x >= (end - 1)[:, None])).long()
        ids, labels = _mask_tokens(p['input_ids'].cuda().clone(), stm.cuda(), ctx, 0.15, -1,
                                   seed=mask_seed(777, 0, b), counter=(2 << 32) | in_bin[b],
                                   whole_word=ww)
        in_bin[b] += 1
        assert torch.equal(ids.cpu(), m['input_ids']) and torch.equal(labels.cpu(), m['labels'])
        for k in ('token_type_ids', 'attention_mask', 'next_sentence_labels'):
            assert torch.equal(p[k], m[k])
    assert sum(int((m['labels'] != -1).sum()) for m in masked) > 100


def test_static_masking_is_the_pair_tables(src):
    """static_masking=True, rng='replay': labels sit exactly at the table's positions with the
    table's original ids, and the ids are the table's masked ids."""
    exp = _expected(_ns(src, 777, masking=True, rng='replay'))
    loader = _make(src, batch_size=32, static_masking=True, rng='replay', drop_last=False,
                   gpu_batch_bytes=150_000, ignore_index=-100)
    batches = _epoch(loader)
    got = [s for b in batches for s in _samples(b, static=True, ignore=-100)]
    assert collections.Counter(got) == collections.Counter(exp)
    assert all('special_tokens_mask' not in b for b in batches)


# ---- two ranks over gloo, both on the one GPU ------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, src, bs, out):
    import torch.distributed as dist
    dist.init_process_group('gloo', init_method='tcp://127.0.0.1:{}'.format(port), rank=rank,
                            world_size=world, timeout=timedelta(seconds=60))
    try:
        torch.cuda.set_device(0)
        from lddl_amd.torch import get_bert_pretrain_online_data_loader
        args = dict(BASE, books=src, batch_size=bs, mlm_probability=0.0,
                    gpu_batch_bytes=100_000)
        loader = get_bert_pretrain_online_data_loader(**args)  # rank / world: the group's
        steps, samples = [], []
        for b in loader:
            b = {k: v.cpu() for k, v in b.items()}
            _, _, end = _layout(b)
            bins = set(_bin_of(end.numpy()).tolist())
            assert len(bins) == 1
            steps.append((bins.pop(), b['input_ids'].shape[0]))
            samples += _samples(b)
        out[rank] = (steps, samples, loader.dropped_per_bin.tolist(), loader.dropped_samples,
                     loader.num_rounds)
    finally:
        dist.destroy_process_group()


def test_two_ranks_agree(src):
    import torch.multiprocessing as mp
    bs = 16
    exp = [_expected(_ns(src, 777), r, 2) for r in range(2)]
    rows = np.stack([np.bincount(_bin_of([len(s[0]) // 8 + len(s[1]) // 8 + 3 for s in e]),
                                 minlength=NBINS) for e in exp])
    with mp.Manager() as m:
        out = m.dict()
        mp.spawn(_rank_worker, args=(2, _free_port(), src, bs, out), nprocs=2, join=True)
        res = dict(out)
    assert res[0][0] == res[1][0]  # as many batches, from the same bin at every step
    assert all(n == bs for _, n in res[0][0]) and len(res[0][0]) > 4
    assert res[0][4] == res[1][4] >= 2
    yielded = np.minimum(rows[0] // bs, rows[1] // bs)
    np.testing.assert_array_equal(np.bincount([b for b, _ in res[0][0]], minlength=NBINS), yielded)
    keys = [collections.Counter(e) for e in exp]
    for r in range(2):
        got = collections.Counter(res[r][1])
        assert not got - keys[r]  # this rank's partitions only
        np.testing.assert_array_equal(res[r][2], rows[r] - bs * yielded)
        assert res[r][3] == int((rows[r] - bs * yielded).sum())
        assert res[r][3] <= NBINS * bs + int((rows[r] - rows.min(0)).sum())
    # the partitions of the ranks are disjoint: hardly a pair of one is a pair of the other
    assert sum((keys[0] & keys[1]).values()) < 0.01 * len(exp[0])
