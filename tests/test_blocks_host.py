"""RoBERTa blocks without a GPU: every refusal of the three entry points (the
values are checked before anything is launched), the Python helpers' argument errors, and the
oracle itself on three tiny cases whose blocks are written out here."""
import ctypes

import pytest

import blocks_oracle as O

X = 0x1000  # stands for a device pointer: a refusal never follows it


def refused(status, word):
    from lddl_amd._native import lib
    assert status == -1 and word in lib.lddl_last_error().decode(), lib.lddl_last_error()


def span_params(**kw):
    from lddl_amd._native import SpanParams, lib
    sp = SpanParams()
    assert lib.lddl_span_params_make(0.15, 3, None, ctypes.byref(sp)) == 0
    for k, v in kw.items():
        setattr(sp, k, v)
    return ctypes.cast(ctypes.pointer(sp), ctypes.c_void_p)


@pytest.mark.parametrize('word,at,value', [
    ('seq_len', 5, 2), ('mode', 6, 2), ('negative', 2, -1), ('null output', 7, None),
    ('null output', 11, None), ('null token table', 1, None), ('null token table', 8, None)])
def test_plan_refusals(word, at, value):
    from lddl_amd._native import lib
    args = [None, X, 4, X, 1, 8, 0, X, X, X, X, X]
    args[at] = value
    refused(lib.lddl_blocks_plan(*args), word)


@pytest.mark.parametrize('word,at,value', [
    ('seq_len', 8, 2), ('null token table or plan', 1, None), ('null token table or plan', 3, None),
    ('null token table or plan', 5, None), ('null output', 11, None)])
def test_collate_refusals(word, at, value):
    from lddl_amd._native import lib
    args = [None, X, X, X, X, X, None, 4, 8, X, X, X, 0, 2, 1]
    args[at] = value
    refused(lib.lddl_collate_blocks(*args), word)
    masked = [X, 100] + args[:12] + [0, 2, 1, 4, 0.15, -100, 100, 1, 0, span_params()]
    refused(lib.lddl_collate_blocks_masked(*masked), word)
    assert lib.lddl_collate_blocks(None, X, X, X, X, X, None, 0, 8, None, None, None, 0, 2, 1) == 0


@pytest.mark.parametrize('word,at,value', [
    ('n_ids', 1, 0), ('n_ids', 1, 1 << 31), ('continuation bitmap', 0, None),
    ('span params', 23, lambda: span_params(n=17)),
    ('span params', 23, lambda: span_params(p_start=2.0)),
    ('span params', 23, lambda: span_params(cum=(ctypes.c_float * 15)(*[0.5] * 15))),
    ('mlm_probability', 18, 1.5), ('vocab_len', 20, 0)])
def test_masked_collate_refusals_of_its_own(word, at, value):
    from lddl_amd._native import lib
    args = [X, 100, None, X, X, X, X, X, None, 4, 8, X, X, X, 0, 2, 1, 4, 0.15, -100, 100, 1, 0,
            span_params()]
    args[at] = value() if callable(value) else value
    refused(lib.lddl_collate_blocks_masked(*args), word)


def test_python_argument_errors(tmp_path):
    from lddl_amd import bpe as B
    from lddl_amd.torch import roberta
    for L in (2, 3.0, True, None, (1 << 24) + 1):
        with pytest.raises(ValueError, match='seq_len'):
            roberta.roberta_blocks((None,) * 4, L)
    with pytest.raises(ValueError, match='mode'):
        roberta.roberta_blocks((None,) * 4, 8, 'none')
    for kw, word in ((dict(mask=(0.1, 0)), 'mask must'), (dict(mask=(2, 0, 0)), 'p must'),
                     (dict(mask=None, whole_word=True), 'need mask'),
                     (dict(mask=(0.1, 0, 0), whole_word=True, span=2), 'not both'),
                     (dict(mask=None, special_ids={'cls': 1}), 'unknown keys')):
        with pytest.raises(ValueError, match=word):
            roberta.collate_blocks(None, None, None, **kw)
    (tmp_path / 'a.txt').write_text('One document. Two sentences.\n')
    make = lambda **kw: roberta.get_roberta_pretrain_data_loader(**{  # noqa: E731
        **dict(path=str(tmp_path), bpe=(B.SYNTH_VOCAB, B.SYNTH_MERGES), batch_size=4), **kw})
    assert make().files == [str(tmp_path / 'a.txt')]
    for kw, err in ((dict(path=str(tmp_path / 'none')), FileNotFoundError),
                    (dict(bpe=B.SYNTH_VOCAB), ValueError), (dict(batch_size=0), ValueError),
                    (dict(max_seq_length=2), ValueError), (dict(mode='eos'), ValueError),
                    (dict(mlm_probability=1.5), ValueError), (dict(rank=0), ValueError),
                    (dict(whole_word_masking=True, span=3), ValueError),
                    (dict(round_bytes=0), ValueError)):
        with pytest.raises(err):
            make(**kw)


@pytest.mark.parametrize('mode,lens,dso,L,P,sep,blocks', [
    # FULL: the separator rides on each document's last sentence that holds a piece
    ('full', [2, 1, 0, 3, 1], [0, 3, 5], 6, [0, 2, 4, 4, 7, 9], [0, 1, 0, 0, 1],
     [(0, 3, 4), (3, 4, 3), (4, 5, 2)]),
    # DOC: no separators, a block stops at its document's end; the empty document gives none
    ('doc', [2, 1, 0, 0, 3, 1], [0, 2, 4, 6], 6, [0, 2, 3, 3, 3, 6, 7], [0] * 6,
     [(0, 2, 3), (4, 6, 4)]),
    # T = 2: a long last sentence is cut to T - 1 pieces and its separator; flag bits are no length
    ('full', [5 | 1 << 30, 1, 7], [0, 1, 3], 4, [0, 2, 3, 5], [1, 0, 1],
     [(0, 1, 2), (1, 2, 1), (2, 3, 2)])])
def test_the_oracle_on_cases_written_out(mode, lens, dso, L, P, sep, blocks):
    assert O.plan(lens, dso, L, mode) == (P, sep, blocks)
    ids = list(range(10, 10 + sum(v & 0xFFFF for v in lens)))
    off = [sum(v & 0xFFFF for v in lens[:s]) for s in range(len(lens))]
    got, _ = O.collate(ids, off, P, sep, blocks, [0], L, bos=0, eos=2, pad=1)
    first = {'full6': [0, 10, 11, 12, 2, 2], 'doc6': [0, 10, 11, 12, 2, 1], 'full4': [0, 10, 2, 2]}
    assert got['input_ids'].tolist() == [first[mode + str(L)]]
    assert got['special_tokens_mask'].tolist()[0][1] == 0
