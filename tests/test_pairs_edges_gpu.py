"""The pair stage against its oracles on hand-built token tables (pair_tables.py): sentences
of exactly the lengths and ids at which compaction, the planners, layout, the partition shuffle
and the gather branch, handed to make_pairs as the tokenizer would hand them, with every output
array compared for equality, partition by partition. The vocabs have 65,534 lines (the largest
with 2-byte ids, top id 65,533 next to the 16-bit gather's reserved 0xFFFE / 0xFFFF) and 65,535
(the smallest with 4-byte ids). Which gather instantiation each case reaches: DESIGN.md,
"Pair-stage edge cases"; that each case meets its shape classes is asserted on the oracle in
test_pair_tables_host.py and here again on the device's output."""
import numpy as np
import pytest
import torch

import pair_tables as T

pytestmark = pytest.mark.gpu

ARRAYS = ('tokens', 'len_a', 'is_random_next', 'pos', 'labels')


@pytest.fixture(scope='module')
def ctxs(tmp_path_factory):
    from lddl_amd.context import Context
    d = tmp_path_factory.mktemp('vocab')
    out = {n: Context(T.write_vocab(d / 'vocab_{}.txt'.format(n), n)) for n in (T.VOCAB_2B, T.VOCAB_4B)}
    assert out[T.VOCAB_2B].id_bytes == 2 and out[T.VOCAB_4B].id_bytes == 4
    for n, c in out.items():
        assert len(c) == n
        assert tuple(c.vocab[t] for t in ('[CLS]', '[SEP]', '[MASK]')) == T.special_ids()
    return out


_EXPECTED = {}


def expected(case):
    """The oracle's output per partition, computed once per case and shared."""
    if case.id not in _EXPECTED:
        _EXPECTED[case.id] = case.oracle()
    return _EXPECTED[case.id]


def run(ctx, case, trace=None):
    from lddl_amd.pairs import make_pairs
    t = case.tables()

    def dev(a):
        return torch.from_numpy(np.array(a)).cuda()
    kw = dict(masked_lm_ratio=case.ratio) if case.masking else {}
    return make_pairs(ctx, dev(t['sent_off']), dev(t['ids']), dev(t['sent_len']), dev(t['doc_sent_off']),
                      dev(t['part_doc_off']), dev(case.part_seed), seq=case.seq, dup=T.DUP,
                      masking=case.masking, rng=case.rng, native_seed=T.NATIVE_SEED, _trace=trace,
                      **kw).to_host()


def check(case, out):
    exp = expected(case)
    po = out['part_off']
    assert len(po) == len(exp) + 1 and po[0] == 0 and po[-1] == len(out['len_a'])
    assert ('pos' in out) == case.masking
    for p, e in enumerate(exp):
        q0, q1 = int(po[p]), int(po[p + 1])
        if e is None:
            assert q1 == q0, p
            continue
        assert q1 - q0 == len(e['len_a']), p
        t0, t1 = int(out['tok_off'][q0]), int(out['tok_off'][q1])
        msg = 'partition {}'.format(p)
        np.testing.assert_array_equal(np.diff(out['tok_off'][q0:q1 + 1]), np.diff(e['tok_off']), err_msg=msg)
        np.testing.assert_array_equal(out['tokens'][t0:t1], e['tokens'], err_msg=msg)
        np.testing.assert_array_equal(out['len_a'][q0:q1], e['len_a'], err_msg=msg)
        np.testing.assert_array_equal(out['is_random_next'][q0:q1], e['is_random_next'], err_msg=msg)
        if case.masking:
            m0, m1 = int(out['pos_off'][q0]), int(out['pos_off'][q1])
            np.testing.assert_array_equal(np.diff(out['pos_off'][q0:q1 + 1]), np.diff(e['pos_off']),
                                          err_msg=msg)
            np.testing.assert_array_equal(out['pos'][m0:m1], e['pos'], err_msg=msg)
            np.testing.assert_array_equal(out['labels'][m0:m1], e['labels'], err_msg=msg)
    assert out['tok_off'][0] == 0 and out['tok_off'][-1] == len(out['tokens'])
    if case.masking:
        assert out['pos_off'][0] == 0 and out['pos_off'][-1] == len(out['pos']) == len(out['labels'])
    assert T.missing(out, case.seq, case.tables(), case.ratio) == []


@pytest.mark.parametrize('case', T.CASES, ids=lambda c: c.id)
def test_pairs_edge_tables_vs_oracle(ctxs, case):
    check(case, run(ctxs[case.vocab_size], case))


def _knob_case():
    return next(c for c in T.CASES if c.id == 'replay-2B-s132-r0.15')


@pytest.mark.parametrize('knob', ['LDDL_PLAN_SPLIT', 'LDDL_PLAN_SLICE', 'LDDL_SHUFFLE_GLOBAL',
                                  'LDDL_AMD_MASK_POOL'])
def test_pairs_edge_tables_knobs(ctxs, monkeypatch, knob):
    """The same tables through the split plan (the head is the first partition, the tail the
    empty one and the last), the time-sliced plan, the partition shuffle in global memory and
    the re-plan after a mask pool overflow."""
    case = _knob_case()
    monkeypatch.setenv(knob, '100' if knob == 'LDDL_AMD_MASK_POOL' else '1')
    tr = {}
    out = run(ctxs[case.vocab_size], case, tr)
    if knob == 'LDDL_PLAN_SPLIT':
        assert tr['split'] == 1 and tr['head_valid'] == 1 and tr['path'] in ('tail', 'copy'), tr
        assert tr['head_pairs'] == len(expected(case)[0]['len_a'])
    elif knob == 'LDDL_PLAN_SLICE':
        assert tr['split'] == 0 and tr['slices'] > 0 and tr['path'] == 'full', tr
    else:
        assert tr['split'] == 0 and tr['slices'] == 0 and tr['path'] == 'full', tr
    check(case, out)
