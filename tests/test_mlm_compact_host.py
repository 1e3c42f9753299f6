"""Host side of the compact MLM targets (lddl_amd/torch/targets.py), no GPU: the
names are exported, the header declares the entry points, the hook validates and composes
without a device, and no loader signature moved."""
import inspect
import re

import pytest

from conftest import REPO


@pytest.fixture
def no_gpu(monkeypatch):
    import lddl_amd.context as C

    def boom(*a, **k):
        raise AssertionError('the GPU was touched')
    monkeypatch.setattr(C.Context, '__init__', boom)


def test_exports():
    import lddl_amd.torch as T
    from lddl_amd.torch import targets
    assert T.compact_labels is targets.compact_labels
    assert T.CompactMLMTargets is targets.CompactMLMTargets
    sig = inspect.signature(T.compact_labels).parameters
    assert list(sig) == ['labels', 'max_predictions_per_seq', 'ignore_index', 'layout']
    assert sig['ignore_index'].default == -1 and sig['layout'].default == 'rows'
    sig = inspect.signature(T.CompactMLMTargets).parameters
    assert list(sig) == ['max_predictions_per_seq', 'layout', 'ignore_index', 'keep_labels', 'then']
    assert [sig[k].default for k in list(sig)[1:]] == ['rows', -1, True, None]


def test_header_declares_both_entry_points():
    from lddl_amd import _native
    with open(REPO + '/include/lddl_amd.h') as f:
        src = f.read()
    for name in ('lddl_mlm_compact_rows', 'lddl_mlm_compact_flat'):
        assert re.search(r'^int {}\(void\* stream, const int64_t\* d_labels,'.format(name), src,
                         flags=re.M), name
        assert name in _native.SIGNATURES and hasattr(_native.lib, name)


@pytest.mark.parametrize('bad', [0, -1, True, 1.5, None, '20'])
def test_constructor_refuses_max_predictions(no_gpu, bad):
    from lddl_amd.torch import CompactMLMTargets, compact_labels
    with pytest.raises(ValueError, match='max_predictions_per_seq'):
        CompactMLMTargets(bad)
    with pytest.raises(ValueError, match='max_predictions_per_seq'):
        compact_labels(None, bad)  # refused before the tensor is looked at


def test_constructor_refuses_layout_and_ignore_index(no_gpu):
    from lddl_amd.torch import CompactMLMTargets
    with pytest.raises(ValueError, match='layout'):
        CompactMLMTargets(20, layout='dense')
    with pytest.raises(ValueError, match='layout'):
        CompactMLMTargets(20, layout=None)
    for bad in (1.0, None, True, 1 << 63):
        with pytest.raises(ValueError, match='ignore_index'):
            CompactMLMTargets(20, ignore_index=bad)
    with pytest.raises(ValueError, match='then'):
        CompactMLMTargets(20, then=3)
    h = CompactMLMTargets(1, 'flat', -100, keep_labels=False)
    assert (h.max_predictions_per_seq, h.layout, h.ignore_index, h.keep_labels, h.then) == \
        (1, 'flat', -100, False, None)


@pytest.fixture
def stub(monkeypatch):
    """compact_labels replaced by a recorder: the hook's own work, without a device."""
    from lddl_amd.torch import targets
    calls = []

    def fake(labels, P, ignore_index=-1, layout='rows'):
        calls.append((labels, P, ignore_index, layout))
        if layout == 'rows':
            return {'masked_lm_positions': 'pos', 'masked_lm_ids': 'ids',
                    'masked_lm_weights': 'w', 'num_masked': 'n'}
        return {'masked_lm_flat_positions': 'fpos', 'masked_lm_flat_ids': 'fids',
                'num_masked': 'n', 'num_masked_total': 't'}
    monkeypatch.setattr(targets, 'compact_labels', fake)
    return calls


def test_hook_adds_the_keys_and_passes_its_arguments(no_gpu, stub):
    from lddl_amd.torch import CompactMLMTargets
    batch = {'input_ids': 'x', 'labels': 'lab'}
    out = CompactMLMTargets(20, ignore_index=-100)(batch)
    assert stub == [('lab', 20, -100, 'rows')]
    assert out == {'input_ids': 'x', 'labels': 'lab', 'masked_lm_positions': 'pos',
                   'masked_lm_ids': 'ids', 'masked_lm_weights': 'w', 'num_masked': 'n'}
    out = CompactMLMTargets(7, 'flat')({'labels': 'lab2'})
    assert stub[-1] == ('lab2', 7, -1, 'flat')
    assert out == {'labels': 'lab2', 'masked_lm_flat_positions': 'fpos',
                   'masked_lm_flat_ids': 'fids', 'num_masked': 'n', 'num_masked_total': 't'}


def test_keep_labels_false_and_then(no_gpu, stub):
    from lddl_amd.torch import CompactMLMTargets
    out = CompactMLMTargets(20, keep_labels=False)({'input_ids': 'x', 'labels': 'lab'})
    assert set(out) == {'input_ids', 'masked_lm_positions', 'masked_lm_ids', 'masked_lm_weights',
                        'num_masked'}
    seen = []

    def then(b):
        seen.append(sorted(b))
        return ('wrapped', b)
    tag, out = CompactMLMTargets(20, 'flat', keep_labels=False, then=then)({'labels': 'lab'})
    assert tag == 'wrapped' and 'labels' not in out and 'masked_lm_flat_ids' in out
    assert seen == [sorted(out)]  # `then` saw the finished batch


def test_loss_mask_of_torch_mp_keeps_its_values(no_gpu, stub):
    """torch_mp's static batches name their dense [B, L] loss mask masked_lm_positions: the rows
    layout takes that name and leaves the mask as loss_mask; flat does not collide."""
    from lddl_amd.torch import CompactMLMTargets
    out = CompactMLMTargets(20)({'labels': 'lab', 'masked_lm_positions': 'dense'})
    assert out['loss_mask'] == 'dense' and out['masked_lm_positions'] == 'pos'
    out = CompactMLMTargets(20, 'flat')({'labels': 'lab', 'masked_lm_positions': 'dense'})
    assert out['masked_lm_positions'] == 'dense' and 'loss_mask' not in out
    with pytest.raises(ValueError, match='num_masked'):
        CompactMLMTargets(20)({'labels': 'lab', 'num_masked': 0})
    with pytest.raises(ValueError, match='masked_lm_positions'):
        CompactMLMTargets(20)({'labels': 'lab', 'masked_lm_positions': 1, 'loss_mask': 2})


def test_missing_labels_names_the_cause(no_gpu, stub):
    from lddl_amd.torch import CompactMLMTargets
    hook = CompactMLMTargets(20)
    with pytest.raises(KeyError, match='special_tokens_mask'):
        hook({'input_ids': 'x', 'special_tokens_mask': 'm'})  # the online loader's plain collate
    with pytest.raises(KeyError, match='raw samples'):
        hook([('a b', 'c d', True)])  # return_raw_samples=True hands the hook a list
    assert stub == []


LOADER_SIGNATURES = {
    'lddl_amd.torch.get_bert_pretrain_data_loader':
        ['path', 'local_rank', 'shuffle_buffer_size', 'shuffle_buffer_warmup_factor',
         'tokenizer_class', 'vocab_file', 'tokenizer_kwargs', 'data_loader_class',
         'data_loader_kwargs', 'mlm_probability', 'base_seed', 'log_dir', 'log_level',
         'return_raw_samples', 'start_epoch', 'sequence_length_alignment', 'ignore_index',
         'whole_word_masking'],
    'lddl_amd.torch.get_bert_pretrain_packed_data_loader':
        ['path', 'max_seq_length', 'local_rank', 'shuffle_buffer_size',
         'shuffle_buffer_warmup_factor', 'tokenizer_class', 'vocab_file', 'tokenizer_kwargs',
         'data_loader_class', 'data_loader_kwargs', 'mlm_probability', 'base_seed', 'log_dir',
         'log_level', 'return_raw_samples', 'start_epoch', 'sequence_length_alignment',
         'ignore_index', 'whole_word_masking'],
    'lddl_amd.torch_mp.get_bert_pretrain_data_loader':
        ['path', 'local_rank', 'dp_rank', 'shuffle_buffer_size', 'shuffle_buffer_warmup_factor',
         'tokenizer_class', 'vocab_file', 'tokenizer_kwargs', 'data_loader_class',
         'data_loader_kwargs', 'mlm_probability', 'base_seed', 'log_dir', 'log_level',
         'return_raw_samples', 'start_epoch', 'sequence_length_alignment', 'ignore_index',
         'whole_word_masking'],
    'lddl_amd.torch.get_bert_pretrain_online_data_loader':
        ['wikipedia', 'books', 'common_crawl', 'wikipedia_lang', 'vocab_file', 'batch_size',
         'target_seq_length', 'bin_size', 'short_seq_prob', 'duplicate_factor', 'static_masking',
         'masked_lm_ratio', 'mlm_probability', 'whole_word_masking', 'rng', 'block_size',
         'num_blocks', 'sample_ratio', 'base_seed', 'start_epoch', 'rank', 'world',
         'gpu_batch_bytes', 'shuffle_group_bytes', 'read_threads', 'sequence_length_alignment',
         'ignore_index', 'drop_last', 'tokenizer_kwargs', 'punkt_params', 'collate_fn'],
}
LOADER_SIGNATURES['lddl_amd.torch.get_bert_pretrain_online_packed_data_loader'] = \
    ['max_seq_length'] + LOADER_SIGNATURES['lddl_amd.torch.get_bert_pretrain_online_data_loader']


@pytest.mark.parametrize('name', list(LOADER_SIGNATURES))
def test_loader_signatures_are_unchanged(name):
    import importlib
    mod, fn = name.rsplit('.', 1)
    params = inspect.signature(getattr(importlib.import_module(mod), fn)).parameters
    assert list(params) == LOADER_SIGNATURES[name]
    assert params['ignore_index'].default == -1
    assert not any(k in params for k in ('max_predictions_per_seq', 'compact', 'layout'))
