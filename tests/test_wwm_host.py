"""Whole-word masking, host side: the loaders' `whole_word_masking` keyword (no GPU)."""
import inspect

import pytest

from conftest import VOCAB_UNCASED


def _loaders():
    from lddl_amd import torch as lt, torch_mp as lmp
    return [lt.get_bert_pretrain_data_loader, lmp.get_bert_pretrain_data_loader]


@pytest.mark.parametrize('k', [0, 1], ids=['torch', 'torch_mp'])
def test_keyword_is_trailing_and_defaults_to_false(k):
    params = list(inspect.signature(_loaders()[k]).parameters.values())
    assert params[-1].name == 'whole_word_masking'
    assert params[-1].default is False


@pytest.mark.parametrize('k', [0, 1], ids=['torch', 'torch_mp'])
@pytest.mark.parametrize('bad', [1, 'yes', None])
def test_non_bool_is_refused_before_any_file_is_read(tmp_path, k, bad):
    """The path holds no dataset and the vocab file does not exist: a bool would get as far as
    FileNotFoundError, a non-bool is refused with the other argument checks."""
    missing = str(tmp_path / 'no_vocab.txt')
    with pytest.raises(AssertionError):
        _loaders()[k](str(tmp_path), vocab_file=missing, whole_word_masking=bad)
    with pytest.raises(FileNotFoundError):
        _loaders()[k](str(tmp_path), vocab_file=missing, whole_word_masking=True)


def test_internal_keywords_default_to_false():
    from lddl_amd.torch import bert
    for fn in (bert._mask_tokens, bert.encode_packed, bert.GPUCollateLoader.__init__):
        assert inspect.signature(fn).parameters['whole_word'].default is False


def test_keyword_is_ignored_with_raw_samples(tmp_path):
    """return_raw_samples=True: the option changes nothing (no collate runs)."""
    import logging
    from loader_data import make_loader_dataset
    from lddl_amd.torch import get_bert_pretrain_data_loader
    d = str(tmp_path / 'raw')
    make_loader_dataset(d, VOCAB_UNCASED, binned=False, static=True)
    seqs = []
    for ww in (False, True):
        dl = get_bert_pretrain_data_loader(
            d, shuffle_buffer_size=8, shuffle_buffer_warmup_factor=2, vocab_file=VOCAB_UNCASED,
            data_loader_kwargs={'batch_size': 3, 'num_workers': 1}, return_raw_samples=True,
            log_level=logging.WARNING, whole_word_masking=ww)
        seqs.append([[list(map(str, col)) for col in batch] for batch in dl])
        dl._iterator._shutdown_workers()
    assert seqs[0] == seqs[1] and seqs[0]
