"""Host side of the packed online loader (lddl_amd/torch/online.py), no GPU: the
entry point exists, its argument errors fire before any device call, and the unpacked loader's
validation is what it was."""
import inspect
import re

import pytest

from conftest import REPO, VOCAB_UNCASED


def _corpus(tmp_path):
    d = tmp_path / 'source'
    d.mkdir()
    (d / 'f.txt').write_text(''.join(
        'doc-{} One sentence here. Another one follows it.\n'.format(i) for i in range(20)))
    return str(d)


@pytest.fixture
def no_gpu(monkeypatch):
    import lddl_amd.context as C

    def boom(*a, **k):
        raise AssertionError('the GPU was touched')
    monkeypatch.setattr(C.Context, '__init__', boom)


def test_entry_point_and_its_keywords():
    import lddl_amd.torch as T
    from lddl_amd.torch import online
    packed = T.get_bert_pretrain_online_packed_data_loader
    assert packed is online.get_bert_pretrain_online_packed_data_loader
    assert T.plan_rows_device is online.plan_rows_device
    assert T.collate_pairs_seqpacked is online.collate_pairs_seqpacked
    old = inspect.signature(T.get_bert_pretrain_online_data_loader).parameters
    new = inspect.signature(packed).parameters
    assert list(new)[0] == 'max_seq_length'
    assert list(new)[1:] == list(old)  # every keyword of the online loader, in its order
    for k in old:
        assert new[k].default == old[k].default, k
    assert 'max_seq_length' not in old and '_packed' not in old


def test_bound_mirrors_the_header():
    from lddl_amd.torch.online import SEQPLAN_MAX_BATCH
    with open(REPO + '/include/lddl_amd.h') as f:
        m = re.search(r'#define LDDL_SEQPLAN_MAX_BATCH (\d+)', f.read())
    assert int(m.group(1)) == SEQPLAN_MAX_BATCH >= 1024


def test_packed_argument_errors_fire_without_a_gpu(tmp_path, no_gpu):
    from lddl_amd.torch import get_bert_pretrain_online_packed_data_loader as make
    from lddl_amd.torch.online import SEQPLAN_MAX_BATCH
    ok = dict(books=_corpus(tmp_path), vocab_file=VOCAB_UNCASED, batch_size=8)
    for bad in (None, 127, 128.0, '128', True):
        with pytest.raises(ValueError, match='max_seq_length'):
            make(bad, **ok, target_seq_length=128)
    with pytest.raises(ValueError, match='max_seq_length'):
        make(**ok)  # not given
    with pytest.raises(ValueError, match=str(SEQPLAN_MAX_BATCH)):
        make(128, **dict(ok, batch_size=SEQPLAN_MAX_BATCH + 1))
    # the online loader's own errors still fire
    with pytest.raises(ValueError, match='divide'):
        make(128, **ok, bin_size=24)
    with pytest.raises(ValueError, match='no corpus'):
        make(128, vocab_file=VOCAB_UNCASED, batch_size=8)
    with pytest.raises(ValueError):
        make(128, **dict(ok, batch_size=0))
    # valid arguments build the loader without a device: the bound itself, a row longer than
    # the pairs, bins allowed; no length
    loader = make(128, **dict(ok, batch_size=SEQPLAN_MAX_BATCH))
    assert loader._packed and loader.nbins == 1
    loader = make(max_seq_length=512, **ok, target_seq_length=128, bin_size=32)
    assert loader._packed and loader.nbins == 4
    with pytest.raises(TypeError, match='no length'):
        len(loader)


def test_unpacked_loader_validates_as_before(tmp_path, no_gpu):
    from lddl_amd.torch import get_bert_pretrain_online_data_loader as make
    from lddl_amd.torch.online import SEQPLAN_MAX_BATCH, validate_args
    ok = dict(books=_corpus(tmp_path), vocab_file=VOCAB_UNCASED, batch_size=8)
    loader = make(**dict(ok, batch_size=SEQPLAN_MAX_BATCH + 1))  # no bound on its batches
    assert not loader._packed
    with pytest.raises(TypeError):
        make(**ok, max_seq_length=128)  # not a keyword of the unpacked loader
    with pytest.raises(ValueError, match='divide'):
        make(**ok, target_seq_length=128, bin_size=24)
    with pytest.raises(ValueError, match='Only one of'):
        make(**ok, block_size=1 << 20, num_blocks=4)
    assert validate_args(**ok) is None
    assert validate_args(**ok, max_seq_length=3) is None  # ignored unless packing is on
    with pytest.raises(ValueError, match='max_seq_length'):
        validate_args(**ok, max_seq_length=3, _packed=True)
