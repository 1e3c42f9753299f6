"""Whole-word static masking, host surface: the CLI flag and its argument checks,
the `whole_word` keyword of the pair entry points, and the ctypes mirror of lddl_pair_params."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import REPO


def test_flag_parses_and_defaults_off():
    from lddl_amd.dask.bert import pretrain as P
    ap = P.attach_args()
    flags = {a for act in ap._actions for a in act.option_strings}
    assert {'--whole-word-masking', '--no-whole-word-masking'} <= flags
    assert ap.parse_args(['--sink', 'x']).whole_word_masking is False
    assert ap.parse_args(['--sink', 'x', '--whole-word-masking']).whole_word_masking is True
    assert ap.parse_args(['--sink', 'x', '--whole-word-masking',
                          '--no-whole-word-masking']).whole_word_masking is False


@pytest.mark.parametrize('extra', [[], ['--masking'], ['--masking', '--rng', 'replay'],
                                   ['--rng', 'native']])
def test_main_refuses_bad_combinations(extra):
    """Before any GPU work (this test runs without a GPU): --whole-word-masking needs both
    --masking and --rng native."""
    from lddl_amd.dask.bert import pretrain as P
    ap = P.attach_args()
    with pytest.raises(ValueError, match='whole-word-masking'):
        P.main(ap.parse_args(['--sink', '/tmp/x', '--whole-word-masking'] + extra))


def test_pair_entry_points_take_whole_word():
    from lddl_amd import pairs
    for fn in (pairs.make_pairs, pairs.tokenize_and_pair_chunked):
        prm = inspect.signature(fn).parameters['whole_word']
        assert prm.default is False
    # the positional order of the existing parameters stands
    names = list(inspect.signature(pairs.make_pairs).parameters)
    assert names[:16] == ['ctx', 'sent_off', 'ids', 'sent_len', 'doc_sent_off', 'part_doc_off',
                          'part_seed', 'seq', 'dup', 'masking', 'short_seq_prob',
                          'masked_lm_ratio', 'rng', 'native_seed', '_capacity_scale', '_trace']
    assert [f.name for f in pairs.PairBatch.__dataclass_fields__.values()][:12] == [
        'tokens', 'tok_off', 'len_a', 'is_random_next', 'pos', 'labels', 'pos_off',
        'n_kept_sentences', 'n_kept_documents', 'part_off', 'plan_ms', 'n_masked']


def test_pair_entry_points_refuse_before_the_native_call():
    """The two bad combinations raise ValueError from the argument check: no context, tensor or
    GPU is touched (every other argument is None)."""
    from lddl_amd import pairs
    none6 = (None,) * 6
    with pytest.raises(ValueError, match='whole_word'):
        pairs.make_pairs(None, *none6, masking=False, rng='native', whole_word=True)
    with pytest.raises(ValueError, match='whole_word'):
        pairs.make_pairs(None, *none6, masking=True, rng='replay', whole_word=True)
    none5 = (None,) * 5
    with pytest.raises(ValueError, match='whole_word'):
        pairs.tokenize_and_pair_chunked(None, *none5, masking=True, whole_word=True)


_CTYPES = {'int32_t': ctypes.c_int32, 'uint32_t': ctypes.c_uint32, 'int64_t': ctypes.c_int64,
           'uint64_t': ctypes.c_uint64, 'double': ctypes.c_double, 'float': ctypes.c_float}


def header_pair_params():
    """[(type, name)] of lddl_pair_params as include/lddl_amd.h lists them."""
    src = open(os.path.join(REPO, 'include', 'lddl_amd.h')).read()
    body = re.search(r'typedef struct \{(.*?)\} lddl_pair_params;', src, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    return re.findall(r'(\w+)\s+(\w+)\s*;', body)


def test_pair_params_mirror_the_header():
    from lddl_amd._native import PairParams
    fields = header_pair_params()
    names = [n for _, n in fields]
    assert names[-2:] == ['native_seed', 'whole_word']
    assert [n for n, _ in PairParams._fields_] == names
    assert [t for _, t in PairParams._fields_] == [_CTYPES[t] for t, _ in fields]

    class FromHeader(ctypes.Structure):
        _fields_ = [(n, _CTYPES[t]) for t, n in fields]
    assert ctypes.sizeof(PairParams) == ctypes.sizeof(FromHeader) == 48
    assert PairParams.whole_word.offset == 40
    assert PairParams(128, 5, 1, 1, 0.1, 0.15, 7, 1).whole_word == 1
