"""CompactMLMTargets as the collate_fn of each of the five loaders: with one seed
the hooked loader yields the unhooked loader's batches, bit for bit, plus the numpy compaction
of each batch's own labels; keep_labels=False removes labels and nothing else."""
import logging

import numpy as np
import pytest
import torch

from conftest import VOCAB_UNCASED
from loader_data import make_loader_dataset
from test_mlm_compact_gpu import ref_flat, ref_rows
from test_online_loader_gpu import BASE, _write_corpus
from test_seqpack_gpu import _stop_workers

pytestmark = pytest.mark.gpu

P = 6  # small enough that some rows overflow
ROWS = ('masked_lm_positions', 'masked_lm_ids', 'masked_lm_weights', 'num_masked')
FLAT = ('masked_lm_flat_positions', 'masked_lm_flat_ids', 'num_masked', 'num_masked_total')


def _take(loader, stop=None):
    """One epoch (a few dozen small batches: no loader is left half-way through its epoch)."""
    out = [{k: v.cpu() for k, v in b.items()} for b in loader]
    if stop is not None:
        stop(loader)
    return out


def _check(make, ignore=-1, stop=None, loss_mask=False):
    """make(collate_fn or None) -> a fresh loader with the same seed."""
    from lddl_amd.torch import CompactMLMTargets
    base = _take(make(None), stop)
    assert len(base) > 8 and all('labels' in b for b in base)
    seen = []
    rows = _take(make(CompactMLMTargets(P, ignore_index=ignore)), stop)
    flat = _take(make(CompactMLMTargets(P, 'flat', ignore, keep_labels=False,
                                        then=lambda b: seen.append(sorted(b)) or b)), stop)
    assert len(rows) == len(flat) == len(base)
    masked = overflow = 0
    for b, r, f in zip(base, rows, flat):
        lab = b['labels'].numpy()
        # rows, labels kept: every original key bit for bit (torch_mp's dense mask, whose name the
        # compact positions take, under loss_mask), the added keys the compaction of these labels
        moved = {'masked_lm_positions': 'loss_mask'} if loss_mask else {}
        assert set(r) == {moved.get(k, k) for k in b} | set(ROWS)
        for k in b:
            assert torch.equal(r[moved.get(k, k)], b[k]), k
        for k, e in zip(ROWS, ref_rows(lab, P, ignore)):
            assert r[k].dtype == torch.from_numpy(e).dtype and r[k].shape == e.shape, k
            np.testing.assert_array_equal(r[k].numpy(), e, err_msg=k)
        # flat, keep_labels=False: only labels left
        assert set(f) == (set(b) - {'labels'}) | set(FLAT)
        for k in set(b) - {'labels'}:
            assert torch.equal(f[k], b[k]), k
        for k, e in zip(FLAT, ref_flat(lab, lab.shape[0] * P, ignore)):
            assert f[k].dtype == torch.from_numpy(e).dtype and f[k].shape == e.shape, k
            np.testing.assert_array_equal(f[k].numpy(), e, err_msg=k)
        if loss_mask:
            assert r['loss_mask'].shape == lab.shape and f['masked_lm_positions'].shape == lab.shape
        n = (lab != ignore).sum(1)
        masked += int(n.sum())
        overflow += int((n > P).sum())
    assert seen == [sorted(f) for f in flat]  # `then` ran on every finished batch
    assert masked > 0
    return masked, overflow


@pytest.fixture(scope='module')
def shards(tmp_path_factory):
    root = tmp_path_factory.mktemp('mlm_compact')
    out = {}
    for name, static in (('static', True), ('dynamic', False)):
        out[name] = str(root / name)
        make_loader_dataset(out[name], VOCAB_UNCASED, binned=False, static=static)  # one worker
    return out


@pytest.fixture(scope='module')
def corpus(tmp_path_factory):
    return _write_corpus(str(tmp_path_factory.mktemp('mlm_compact_online')))


def _parquet_kw(hook, **kw):
    dl = {'batch_size': 4, 'num_workers': 1}
    if hook is not None:
        dl['collate_fn'] = hook
    return dict(shuffle_buffer_size=8, shuffle_buffer_warmup_factor=2, vocab_file=VOCAB_UNCASED,
                data_loader_kwargs=dl, base_seed=77, log_level=logging.WARNING, **kw)


@pytest.mark.parametrize('masking', ['static', 'dynamic'])
def test_parquet_loader(shards, masking):
    from lddl_amd.torch import get_bert_pretrain_data_loader
    _check(lambda hook: get_bert_pretrain_data_loader(
        shards[masking], **_parquet_kw(hook, ignore_index=-100)), -100, _stop_workers)


def test_packed_parquet_loader(shards):
    from lddl_amd.torch import get_bert_pretrain_packed_data_loader
    _, overflow = _check(lambda hook: get_bert_pretrain_packed_data_loader(
        shards['dynamic'], 128, **_parquet_kw(hook)), -1, _stop_workers)
    assert overflow > 0  # several samples share a row: P counts per row


def test_torch_mp_loader(shards):
    from lddl_amd.torch_mp import get_bert_pretrain_data_loader
    _check(lambda hook: get_bert_pretrain_data_loader(
        shards['static'], dp_rank=0, **_parquet_kw(hook)), -1, _stop_workers, loss_mask=True)


def _online_kw(corpus, hook, **kw):
    return dict(BASE, books=corpus, rank=0, world=1, batch_size=32, gpu_batch_bytes=150_000,
                collate_fn=hook, **kw)


def test_online_loader(corpus):
    from lddl_amd.torch import get_bert_pretrain_online_data_loader
    _check(lambda hook: get_bert_pretrain_online_data_loader(**_online_kw(corpus, hook)))


def test_online_packed_loader(corpus):
    from lddl_amd.torch import get_bert_pretrain_online_packed_data_loader
    _, overflow = _check(lambda hook: get_bert_pretrain_online_packed_data_loader(
        128, **_online_kw(corpus, hook, bin_size=None, ignore_index=-100)), -100)
    assert overflow > 0
