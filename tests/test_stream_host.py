"""The GPT stream without a GPU: every argument error of `stream_plan`,
`collate_stream` and the loader's `validate_args`, and stream_oracle.py against three rows
written out by hand."""
from types import SimpleNamespace

import numpy as np
import pytest

import stream_oracle as O
from lddl_amd.torch import gpt

Vocab = type('Vocab', (), {'special_ids': {}})
PLAIN, FIM = SimpleNamespace(fim=(0, 0, 0, 0)), SimpleNamespace(fim=(65536, 0, 0, 0))
ALL = dict(eos_id=1, fim_prefix_id=2, fim_middle_id=3, fim_suffix_id=4)


@pytest.mark.parametrize('kw', [
    dict(seq_len=0), dict(seq_len=(1 << 20) + 1), dict(seq_len=8.0), dict(seq_len=True),
    dict(seq_len=8, fim=(0.5, 0.5)), dict(seq_len=8, fim=(1.5, 0, 1, 1)),
    dict(seq_len=8, fim=(0.5, -0.1, 1, 1)), dict(seq_len=8, fim=('x', 0, 1, 1)),
    dict(seq_len=8, fim=(0.5, 0.5, None, 1))])
def test_stream_plan_refuses(kw):
    with pytest.raises(ValueError):
        gpt.stream_plan(None, **kw)


@pytest.mark.parametrize('plan,kw,word', [
    (PLAIN, dict(special_ids=dict(bos_id=1)), 'bos_id'),
    (PLAIN, dict(special_ids=dict(eos_id=-1)), 'eos_id'),
    (PLAIN, dict(max_seqs=0), 'max_seqs'), (PLAIN, dict(max_seqs=2.0), 'max_seqs'),
    (PLAIN, dict(ignore_index=None), 'ignore_index'),
    (PLAIN, {}, 'endoftext'),
    (FIM, dict(special_ids=dict(eos_id=1)), '<fim_prefix>'),
    (FIM, dict(special_ids=dict(ALL, fim_suffix_id=None)), 'fim_suffix_id'),
    (FIM, dict(special_ids={k: v for k, v in ALL.items() if k != 'fim_middle_id'}), '<fim_middle>')])
def test_collate_stream_refuses(plan, kw, word):
    with pytest.raises(ValueError, match=word):
        gpt.collate_stream(Vocab(), None, plan, **kw)


def test_fixed_point_rates_round_half_up():
    assert gpt.check_fim(None) == (0, 0, 0, 0)
    assert gpt.check_fim((1, 0.5, -1, 1 << 64)) == (65536, 32768, (1 << 64) - 1, 0)
    assert gpt.check_fim((1.5 / 65536, 1.49 / 65536, 0, 0))[:2] == (2, 1)


@pytest.mark.parametrize('kw', [
    dict(max_seq_length=0), dict(max_seq_length=1 << 21), dict(fim_rate=2), dict(fim_spm_rate=-1),
    dict(special_ids=dict(pad_id=0)), dict(ignore_index='x'), dict(batch_size=0), dict(bpe=None),
    dict(rank=0), dict(rank=2, world=2), dict(round_bytes=0)])
def test_loader_refuses(tmp_path, kw):
    from lddl_amd import bpe as B
    (tmp_path / 'a.txt').write_text('one document\n')
    good = dict(path=str(tmp_path), bpe=(B.SYNTH_VOCAB, B.SYNTH_MERGES), batch_size=2)
    assert gpt.validate_args(**good) == [str(tmp_path / 'a.txt')]
    with pytest.raises(ValueError):
        gpt.validate_args(**dict(good, **kw))
    with pytest.raises(FileNotFoundError):
        gpt.validate_args(**dict(good, path=str(tmp_path / 'none')))


def test_oracle_against_three_rows_by_hand():
    # d0 = 10 .. 14, d1 = 20 21 | 22 23 (two sentences, a gap), d2 = an empty sentence, d3 = no
    # sentence, d4 = 30 31. Under seed 45 d0 is PSM with a, b = 1, 2, d1 SPM with 1, 2 and d4 PSM
    # with 0, 1; eos 1, <pre> 90, <mid> 91, <suf> 92:
    #   90 10 92 12 13 14 91 11 1 | 90 92 22 23 91 20 21 1 | 1 | 1 | 90 92 31 91 30 1
    table = (np.array([10, 11, 12, 13, 14, 0, 20, 21, 0, 0, 22, 23, 30, 31], np.int32),
             np.array([0, 6, 10, 12, 12, 14]), np.array([5 | (1 << 30), 2, 2, 0, 2], np.int32),
             np.array([0, 1, 3, 4, 4, 5]))
    toks, term, draws = O.stream(table, None, (1, 0.5, 45, 0), 1, 90, 91, 92)
    assert draws == {0: (False, 1, 2), 1: (True, 1, 2), 2: None, 3: None, 4: (False, 0, 1)}
    assert len(toks) == 25 and O.n_rows(25, 7) == 3 and O.n_rows(22, 7) == 3
    assert O.n_rows(21, 7) == 2 and O.n_rows(1, 7) == 0 and O.n_rows(0, 7) == 0
    got = O.collate(toks, term, 7, eod_mask_loss=True)
    assert got == {
        'input_ids': [[90, 10, 92, 12, 13, 14, 91], [11, 1, 90, 92, 22, 23, 91],
                      [20, 21, 1, 1, 1, 90, 92]],
        'labels': [[10, 92, 12, 13, 14, 91, 11], [1, -100, 92, 22, 23, 91, 20],
                   [21, 1, -100, -100, -100, 92, 31]],
        'position_ids': [[0, 1, 2, 3, 4, 5, 6], [0, 1, 0, 1, 2, 3, 4], [0, 1, 2, 0, 0, 0, 1]],
        'sequence_ids': [[0, 0, 0, 0, 0, 0, 0], [0, 0, 1, 1, 1, 1, 1], [0, 0, 0, 1, 2, 3, 3]],
        'cu_seqlens': [0, 7, 9, 14, 17, 18, 19, 21], 'n_seqs': 7}
    cut = O.collate(toks, term, 7, rows=[2, 0], reset_position_ids=False, max_seqs=3)
    assert cut['labels'][0] == [21, 1, 1, 1, 90, 92, 31] and cut['position_ids'][0] == list(range(7))
    assert cut['cu_seqlens'] == [0, 3, 4, 14] and cut['n_seqs'] == 5
