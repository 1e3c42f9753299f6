"""lddl_amd.torch_mp (the model-parallel BERT loader) vs the reference's lddl.torch_mp
(tests/golden/loader_mp.npz, made by tests/golden/make_loader_mp_golden.py):

* CPU: sample order per rank at world 4 with two data-parallel groups (files strided and workers
  seeded by dp_rank), spawned workers without the native library, get_dp_size;
* GPU: `_to_encoded_inputs` with the loss mask (`masked_lm_positions`) bit for bit on hand-made
  batches, the C entry point's refusals, the binned static loader, and two ranks of one group
  applying the same dynamic mask."""
import logging
import os
import socket

import numpy as np
import pytest
import pyarrow.parquet as pq
import torch.multiprocessing as mp

from conftest import GOLDEN, VOCAB_UNCASED
from loader_data import make_loader_dataset
from loader_mp_data import (MP_BIN_DL_KWARGS, MP_BIN_KWARGS, MP_KEYS, MP_RAW_DL_KWARGS,
                            MP_RAW_KWARGS, MP_SHARDS, MP_WORLD, make_collate_cases, raw_lines)

CASES = make_collate_cases(VOCAB_UNCASED)
SHARED = ('input_ids', 'token_type_ids', 'attention_mask', 'labels', 'next_sentence_labels')


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(GOLDEN, 'loader_mp.npz')) as z:
        return dict(z)


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _assert_no_native(worker_id):
    import sys
    assert 'lddl_amd._native' not in sys.modules, 'a DataLoader worker loaded the native library'


def _raw_rank(rank, port, raw_dir, dl_kwargs, out):
    import torch.distributed as dist
    from lddl_amd.torch_mp import get_bert_pretrain_data_loader
    dist.init_process_group('gloo', init_method='tcp://127.0.0.1:{}'.format(port), rank=rank,
                            world_size=MP_WORLD)
    dl = get_bert_pretrain_data_loader(
        raw_dir, local_rank=rank, dp_rank=rank // 2, vocab_file=VOCAB_UNCASED,
        data_loader_kwargs=dict(dl_kwargs), log_level=logging.WARNING, **MP_RAW_KWARGS)
    seq = []
    for _ in range(2):
        for batch in dl:
            seq += raw_lines(batch)
    out[rank] = (seq, len(dl))
    dist.barrier()
    dist.destroy_process_group()


def _run_world4(raw_dir, dl_kwargs):
    make_loader_dataset(raw_dir, VOCAB_UNCASED, binned=False, static=False, n_shards=MP_SHARDS)
    with mp.Manager() as m:
        out = m.dict()
        mp.spawn(_raw_rank, args=(_free_port(), raw_dir, dl_kwargs, out), nprocs=MP_WORLD,
                 join=True)
        return dict(out)


def test_world4_raw_order_matches_reference(tmp_path, golden):
    d = str(tmp_path / 'raw')
    # forked workers, as in a torchrun-started rank (the default start method of a spawned
    # process would be spawn: the next test)
    res = _run_world4(d, dict(MP_RAW_DL_KWARGS, multiprocessing_context='fork'))
    for r in range(MP_WORLD):
        assert res[r][1] == int(golden['raw_len_r{}'.format(r)])
        assert res[r][0] == golden['raw_order_r{}'.format(r)].tolist(), r
    # the two ranks of a data-parallel group yield the same sequence
    assert res[0][0] == res[1][0] and res[2][0] == res[3][0]
    assert res[0][0] != res[2][0]
    # the two groups read disjoint files that together cover all eight
    where = {}
    for name in sorted(os.listdir(d)):
        if name.startswith('shard-'):
            t = pq.read_table(os.path.join(d, name)).to_pydict()
            for a, b, c in zip(t['A'], t['B'], t['is_random_next']):
                where.setdefault('{}|{}|{}'.format(a, b, int(c)), set()).add(name)
    assert all(len(v) == 1 for v in where.values())  # a sample names its file
    per_epoch = len(res[0][0]) // 2
    for e in range(2):
        files = [{next(iter(where[s])) for s in res[r][0][e * per_epoch:(e + 1) * per_epoch]
                  if s != '--batch--'} for r in (0, 2)]
        assert len(files[0]) == len(files[1]) == MP_SHARDS // 2
        assert not files[0] & files[1]
        assert len(files[0] | files[1]) == MP_SHARDS


def test_world4_spawned_workers_without_native_library(tmp_path, golden):
    """DataLoader workers started with `spawn` import only the worker-side modules and yield the
    reference's order (rank 0 is compared; every rank runs the check in its workers)."""
    res = _run_world4(str(tmp_path / 'raw'),
                      dict(MP_RAW_DL_KWARGS, multiprocessing_context='spawn',
                           worker_init_fn=_assert_no_native))
    assert res[0][0] == golden['raw_order_r0'].tolist()


def test_get_dp_size_without_process_group():
    from lddl_amd.torch_mp.utils import get_dp_size
    assert get_dp_size(0) == 1


# ---- GPU ------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ctx():
    from lddl_amd.context import Context
    return Context(VOCAB_UNCASED, True)


def _assert_case(enc, golden, name):
    assert set(enc) == set(MP_KEYS)
    for k in MP_KEYS:
        assert enc[k].is_cuda
        np.testing.assert_array_equal(enc[k].cpu().numpy(), golden['col_{}_{}'.format(name, k)],
                                      err_msg='{} {}'.format(name, k))


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_encode_static_with_loss_mask(golden, ctx, case):
    from lddl_amd.torch_mp.bert import _to_encoded_inputs
    name, batch, align, ignore = case
    enc = _to_encoded_inputs(batch, ctx, sequence_length_alignment=align, ignore_index=ignore)
    _assert_case(enc, golden, name)


@pytest.mark.gpu
def test_shared_outputs_equal_plain_collate(ctx):
    """lddl_collate_encode and lddl_collate_encode_mp agree on the five outputs they share."""
    import torch
    from lddl_amd.torch.bert import PackedBatch, encode_packed
    name, batch, align, ignore = next(c for c in CASES if c[0] == 's130')
    pk = PackedBatch(batch)
    plain = encode_packed(pk, ctx, align, ignore)
    mp_ = encode_packed(pk, ctx, align, ignore, loss_mask=True)
    assert set(plain) == set(SHARED) and set(mp_) == set(MP_KEYS)
    for k in SHARED:
        assert torch.equal(plain[k], mp_[k]), k


@pytest.mark.gpu
def test_entry_point_refuses_missing_buffers(golden, ctx):
    """A null loss mask or missing static-masking inputs: -1 and a message, nothing launched,
    and the Context goes on working."""
    import torch
    from lddl_amd._native import lib
    from lddl_amd.context import _ptr, _stream
    from lddl_amd.torch.bert import PackedBatch
    from lddl_amd.torch_mp.bert import _to_encoded_inputs
    name, batch, align, ignore = next(c for c in CASES if c[0] == 'b5')
    pk = PackedBatch(batch)
    B = len(pk)
    L = golden['col_b5_input_ids'].shape[1]
    lab_off, pos, pos_off = pk.extra
    dev = ctx.device
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in dict(
        blob=pk.blob, a=pk.a_off, b=pk.b_off, na=pk.na, nb=pk.nb, lab_off=lab_off,
        pos=pos.view(np.int16), pos_off=pos_off).items()}
    o = [torch.full((B, L), 7, dtype=torch.long, device=dev) for _ in range(5)]

    def call(lab_bytes, lab_off_, pos_, pos_off_, labels, loss_mask):
        return lib.lddl_collate_encode_mp(
            ctx.handle, _stream(), _ptr(t['blob']), _ptr(t['a']), _ptr(t['b']), _ptr(t['na']),
            _ptr(t['nb']), B, L, _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), None, lab_bytes, lab_off_,
            pos_, pos_off_, labels, ignore, loss_mask)

    full = (_ptr(t['blob']), _ptr(t['lab_off']), _ptr(t['pos']), _ptr(t['pos_off']), _ptr(o[3]),
            _ptr(o[4]))
    assert call(*full[:5], None) == -1
    assert lib.lddl_last_error()
    assert call(None, None, None, None, full[4], full[5]) == -1
    assert lib.lddl_last_error()
    for k in range(5):  # one missing input is enough
        bad = list(full)
        bad[k] = None
        assert call(*bad) == -1 and lib.lddl_last_error(), k
    torch.cuda.synchronize()
    assert all(bool((x == 7).all()) for x in o)  # nothing was launched
    assert call(*full) == 0
    for x, k in zip(o, ('input_ids', 'token_type_ids', 'attention_mask', 'labels',
                        'masked_lm_positions')):
        np.testing.assert_array_equal(x.cpu().numpy(), golden['col_b5_' + k], err_msg=k)
    _assert_case(_to_encoded_inputs(batch, ctx, align, ignore), golden, name)


@pytest.mark.gpu
def test_binned_static_loader_matches_reference(tmp_path, golden):
    from lddl_amd.torch_mp import get_bert_pretrain_data_loader
    d = str(tmp_path / 'bin')
    make_loader_dataset(d, VOCAB_UNCASED, binned=True, static=True)
    dl = get_bert_pretrain_data_loader(d, vocab_file=VOCAB_UNCASED,
                                       data_loader_kwargs=dict(MP_BIN_DL_KWARGS),
                                       log_level=logging.WARNING, **MP_BIN_KWARGS)
    assert len(dl) == int(golden['bin_len'])
    k = 0
    for _ in range(2):
        for batch in dl:
            assert set(batch) == set(MP_KEYS)
            for name in MP_KEYS:
                assert batch[name].is_cuda
                np.testing.assert_array_equal(batch[name].cpu().numpy(),
                                              golden['bin{}_{}'.format(k, name)], err_msg=name)
            k += 1
    assert k == int(golden['bin_steps'])


def _dyn_rank(rank, port, d, out):
    import torch.distributed as dist
    from lddl_amd.torch_mp import get_bert_pretrain_data_loader
    dist.init_process_group('gloo', init_method='tcp://127.0.0.1:{}'.format(port), rank=rank,
                            world_size=2)
    dl = get_bert_pretrain_data_loader(
        d, local_rank=rank, dp_rank=0, vocab_file=VOCAB_UNCASED,
        data_loader_kwargs={'batch_size': 4, 'num_workers': 2, 'multiprocessing_context': 'fork'},
        log_level=logging.WARNING)
    steps = [{k: v.cpu().numpy() for k, v in batch.items()} for batch in dl]
    out[rank] = steps
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_one_group_two_ranks_same_dynamic_mask(tmp_path):
    """Two ranks of one data-parallel group (both dp_rank 0) on one GPU: the same samples and,
    keyed by dp_rank, the same dynamic mask, step by step."""
    d = str(tmp_path / 'dyn')
    make_loader_dataset(d, VOCAB_UNCASED, binned=True, static=False)
    with mp.Manager() as m:
        out = m.dict()
        mp.spawn(_dyn_rank, args=(_free_port(), d, out), nprocs=2, join=True)
        res = dict(out)
    assert len(res[0]) == len(res[1]) > 0
    masked = 0
    for a, b in zip(res[0], res[1]):
        assert set(a) == set(b) == {'input_ids', 'token_type_ids', 'attention_mask', 'labels',
                                    'next_sentence_labels'}
        np.testing.assert_array_equal(a['input_ids'], b['input_ids'])
        np.testing.assert_array_equal(a['labels'], b['labels'])
        masked += int((a['labels'] != -1).sum())
    assert masked > 0
