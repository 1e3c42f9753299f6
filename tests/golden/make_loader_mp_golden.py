"""Goldens of the REFERENCE model-parallel loader (lddl.torch_mp) over the inputs of
tests/loader_mp_data.py and tests/loader_data.py. Run in the dev container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_loader_mp_golden.py

* collate: `lddl.torch_mp.bert._to_encoded_inputs` on every hand-made static batch, all six
  outputs (`masked_lm_positions` is the [B, L] loss mask);
* raw, world 4 over gloo with dp_rank = rank // 2 (return_raw_samples=True): per rank the sample
  order of two epochs and len(dl);
* binned static masking, world 1: the collated tensors of every step of two epochs.
"""
import os
import socket
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_goldens import import_reference, VOCAB_UNCASED  # noqa: E402
from loader_data import make_loader_dataset  # noqa: E402
from loader_mp_data import (MP_BIN_DL_KWARGS, MP_BIN_KWARGS, MP_KEYS, MP_RAW_DL_KWARGS,  # noqa: E402
                            MP_RAW_KWARGS, MP_SHARDS, MP_WORLD, make_collate_cases, raw_lines)


def _reference_mp():
    import_reference()
    import transformers
    from lddl.torch_mp import bert
    return bert, transformers.BertTokenizerFast


def _raw_rank(rank, port, raw_dir, out):
    import torch.distributed as dist
    bert, tok_cls = _reference_mp()
    dist.init_process_group('gloo', init_method='tcp://127.0.0.1:{}'.format(port), rank=rank,
                            world_size=MP_WORLD)
    dl = bert.get_bert_pretrain_data_loader(
        raw_dir, local_rank=rank, dp_rank=rank // 2, tokenizer_class=tok_cls,
        vocab_file=VOCAB_UNCASED,
        # a spawned rank defaults to spawned workers, which the reference's dataset (it holds a
        # lambda) does not survive: fork them, as a torchrun-started rank would
        data_loader_kwargs=dict(MP_RAW_DL_KWARGS, multiprocessing_context='fork'),
        **MP_RAW_KWARGS)
    seq = []
    for epoch in range(2):
        for batch in dl:
            seq += raw_lines(batch)
    out[rank] = (seq, len(dl))
    dist.barrier()
    dist.destroy_process_group()


def main():
    import torch.multiprocessing as mp
    bert, tok_cls = _reference_mp()
    tok = tok_cls(VOCAB_UNCASED)
    out = {}
    for name, batch, align, ignore in make_collate_cases(VOCAB_UNCASED):
        enc = bert._to_encoded_inputs(batch, tok, sequence_length_alignment=align,
                                      ignore_index=ignore)
        assert set(enc) == set(MP_KEYS)
        for k in MP_KEYS:
            out['col_{}_{}'.format(name, k)] = enc[k].numpy()
    with tempfile.TemporaryDirectory() as d:
        raw_dir = os.path.join(d, 'raw')
        make_loader_dataset(raw_dir, VOCAB_UNCASED, binned=False, static=False, n_shards=MP_SHARDS)
        s = socket.socket()
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
        s.close()
        with mp.Manager() as m:
            res = m.dict()
            mp.spawn(_raw_rank, args=(port, raw_dir, res), nprocs=MP_WORLD, join=True)
            res = dict(res)
        for r in range(MP_WORLD):
            out['raw_order_r{}'.format(r)] = np.asarray(res[r][0])
            out['raw_len_r{}'.format(r)] = np.asarray(res[r][1])
        bin_dir = os.path.join(d, 'bin')
        make_loader_dataset(bin_dir, VOCAB_UNCASED, binned=True, static=True)
        dl = bert.get_bert_pretrain_data_loader(
            bin_dir, tokenizer_class=tok_cls, vocab_file=VOCAB_UNCASED,
            data_loader_kwargs=dict(MP_BIN_DL_KWARGS), **MP_BIN_KWARGS)
        k = 0
        for epoch in range(2):
            for batch in dl:
                for name in MP_KEYS:
                    out['bin{}_{}'.format(k, name)] = batch[name].numpy()
                k += 1
        out['bin_steps'] = np.asarray(k)
        out['bin_len'] = np.asarray(len(dl))
    np.savez_compressed(os.path.join(HERE, 'loader_mp.npz'), **out)
    print('loader_mp goldens: {} collate cases, raw {} entries per rank, binned {} steps'.format(
        len(make_collate_cases(VOCAB_UNCASED)), len(out['raw_order_r0']), k))


if __name__ == '__main__':
    main()
