"""Sequence packing, host side: the row plan against a plain first-fit-decreasing
loop, its invariants, pickling, and the loader's argument checks (no GPU)."""
import inspect
import pickle
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, VOCAB_UNCASED

CAP = 128


def ffd(lengths, cap):
    """The specification, O(B * R): visit by length descending (ties: lower index), lowest row
    that still has room, else a new row; back to back inside a row."""
    idx = sorted(range(len(lengths)), key=lambda i: (-lengths[i], i))
    rows = []  # per row: the samples in the order placed
    place = {}
    for i in idx:
        for r, members in enumerate(rows):
            if cap - sum(lengths[j] for j in members) >= lengths[i]:
                break
        else:
            rows.append([])
            r = len(rows) - 1
        place[i] = (r, sum(lengths[j] for j in rows[r]), len(rows[r]) + 1)
        rows[r].append(i)
    fill = list(lengths)
    for members in rows:
        fill[members[-1]] += cap - sum(lengths[j] for j in members)
    order = [i for members in rows for i in members]
    return place, fill, order, len(rows)


def _cases():
    rng = np.random.default_rng(17)
    out = {}
    for B in (1, 5, 7, 64):
        out['random{}'.format(B)] = rng.integers(4, CAP + 1, B).tolist()
    out['full_rows'] = [CAP] * 6
    out['one_plus_rest'] = [1, CAP - 1] * 5
    out['ties'] = [40, 64, 40, 64, 24, 64, 40, 24, 64, 24, 40]
    out['short'] = rng.integers(4, 20, 64).tolist()
    return out


CASES = _cases()


@pytest.mark.parametrize('name', sorted(CASES))
def test_plan_equals_first_fit_decreasing(name):
    from lddl_amd.torch.seqpack import plan_rows
    lengths = CASES[name]
    plan = plan_rows(lengths, CAP)
    place, fill, order, R = ffd(lengths, CAP)
    assert plan.R == R and plan.capacity == CAP
    for i in range(len(lengths)):
        assert (int(plan.row[i]), int(plan.start[i]), int(plan.seq_in_row[i])) == place[i], i
    assert plan.fill.tolist() == fill
    assert plan.order.tolist() == order


@pytest.mark.parametrize('name', sorted(CASES))
def test_plan_invariants(name):
    from lddl_amd.torch.seqpack import plan_rows
    lengths = np.asarray(CASES[name])
    plan = plan_rows(lengths, CAP)
    R = plan.R
    assert R >= -(-int(lengths.sum()) // CAP)
    real = np.zeros((R, CAP), np.int64)
    written = np.zeros((R, CAP), np.int64)
    for i, n in enumerate(lengths):
        r, s = plan.row[i], plan.start[i]
        assert s + plan.fill[i] <= CAP and plan.fill[i] >= n
        real[r, s:s + n] += 1
        written[r, s:s + plan.fill[i]] += 1
    assert real.max() == 1 and real.sum() == lengths.sum()  # segments are disjoint
    assert (written == 1).all()                             # the fill regions tile [R, CAP] once
    key = [(int(plan.row[i]), int(plan.start[i])) for i in plan.order]
    assert key == sorted(key) and sorted(plan.order.tolist()) == list(range(len(lengths)))
    for r in range(R):  # seq_in_row counts 1, 2, ... along the row
        members = [i for i in plan.order if plan.row[i] == r]
        assert [int(plan.seq_in_row[i]) for i in members] == list(range(1, len(members) + 1))


def test_the_cases_hold_what_they_are_meant_to():
    from lddl_amd.torch.seqpack import plan_rows
    assert plan_rows(CASES['full_rows'], CAP).R == 6
    p = plan_rows(CASES['one_plus_rest'], CAP)
    assert p.R == 5 and (p.fill == np.asarray(CASES['one_plus_rest'])).all()  # no tail anywhere
    assert plan_rows(CASES['short'], CAP).R < 64 // 4


def test_too_long_sample_raises():
    from lddl_amd.torch.seqpack import plan_rows
    with pytest.raises(ValueError, match=r'129.*128'):
        plan_rows([5, CAP + 1, 7], CAP)


BATCH = [('a b c', 'd e', True), ('f', 'g h i j', False), ('k l', 'm', False)]


def test_batch_and_collate_pickle():
    from lddl_amd.torch.seqpack import SeqPackedBatch, plan_rows, seqpack_collate
    fn = pickle.loads(pickle.dumps(seqpack_collate(16)))
    spk = pickle.loads(pickle.dumps(fn(BATCH)))
    assert isinstance(spk, SeqPackedBatch) and len(spk) == 3 and not spk.static
    want = plan_rows([8, 8, 6], 16)
    for k in ('row', 'start', 'seq_in_row', 'fill', 'order'):
        np.testing.assert_array_equal(getattr(spk.plan, k), getattr(want, k), err_msg=k)
    assert (spk.plan.R, spk.plan.capacity) == (2, 16)
    assert spk.na.tolist() == [3, 1, 2] and spk.nsl.tolist() == [1, 0, 0]
    with pytest.raises(ValueError):
        seqpack_collate(7)(BATCH)


def test_module_does_not_load_the_native_library():
    code = ('import sys; import lddl_amd.torch.seqpack as s; s.seqpack_collate(16); '
            'assert "lddl_amd._native" not in sys.modules; print("ok")')
    r = subprocess.run([sys.executable, '-c', code], cwd=REPO, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stderr


def test_loader_argument_checks(tmp_path):
    from lddl_amd.torch import get_bert_pretrain_packed_data_loader as mk
    with pytest.raises(ValueError, match='return_raw_samples'):
        mk(str(tmp_path), 128, vocab_file=VOCAB_UNCASED, return_raw_samples=True)
    for bad in (128.0, '128', None, True):
        with pytest.raises(AssertionError):
            mk(str(tmp_path), bad, vocab_file=VOCAB_UNCASED)
    with pytest.raises(FileNotFoundError):  # valid arguments get as far as the vocab file
        mk(str(tmp_path), 128, vocab_file=str(tmp_path / 'no_vocab.txt'))


def test_signature():
    from lddl_amd.torch import bert
    params = list(inspect.signature(bert.get_bert_pretrain_packed_data_loader).parameters.values())
    assert [p.name for p in params[:2]] == ['path', 'max_seq_length']
    assert params[-1].name == 'whole_word_masking' and params[-1].default is False
    old = list(inspect.signature(bert.get_bert_pretrain_data_loader).parameters)
    assert [p.name for p in params] == ['path', 'max_seq_length'] + old[1:]
    enc = inspect.signature(bert.encode_seqpacked).parameters
    assert list(enc) == ['spk', 'ctx', 'max_seq_length', 'sequence_length_alignment',
                         'ignore_index', 'mask', 'events', 'stager', 'whole_word']
    assert enc['whole_word'].default is False and enc['sequence_length_alignment'].default == 8
