"""The hand-built pair tables (pair_tables.py) on the CPU: for every case of the GPU matrix
(test_pairs_edges_gpu.py) the oracle's output reaches every shape class that applies to the
case, so the GPU comparison cannot pass without having met them; and the tables keep the
layout the pair stage's inputs have."""
import numpy as np
import pytest

import pair_tables as T


def test_case_matrix():
    ids = [c.id for c in T.CASES]
    assert len(ids) == 38 and len(set(ids)) == 38 and set(ids) == set(T.SEEDS)


@pytest.mark.parametrize('case', T.CASES, ids=lambda c: c.id)
def test_oracle_reaches_every_class(case):
    parts = case.oracle()
    assert [p is None for p in parts] == [False, True, False]  # the middle partition is empty
    tab = case.tables()
    cl = T.classes(T.merge(parts), case.seq, tab, case.ratio)
    assert len(cl) >= 14
    assert ('mask at 1' in cl) == case.masking
    assert ('a pass with all 128 tokens masked' in cl) == (case.ratio == 1.0)
    assert [k for k, v in cl.items() if not v] == []
    n = np.concatenate([p['num_tokens'] for p in parts if p is not None])
    assert n.max() == case.seq  # (the long documents fill seq 4096)


@pytest.mark.parametrize('seq,vocab_size,long', [(20, T.VOCAB_2B, False), (512, T.VOCAB_4B, False),
                                                 (4096, T.VOCAB_4B, True)])
def test_table_layout(seq, vocab_size, long):
    t = T.build(seq, vocab_size, 1, long)
    lens = (t['sent_len'] & (T.LEN_HAS_CLS_SEP - 1)).astype(np.int64)
    so, ids = t['sent_off'], t['ids']
    assert lens.max() == T.MAX_SENT and (np.diff(so) > lens).all() and len(ids) == so[-1]
    assert lens[0] == 0 and lens[-1] == 0  # dropped sentences at the very front and end
    used = np.zeros(len(ids), bool)
    for s in range(len(lens)):
        used[so[s]:so[s] + lens[s]] = True
    assert (ids[~used] == T.SLACK).all()
    np.testing.assert_array_equal(ids[used], t['k_ids'])
    assert t['k_ids'].min() >= min(T.special_ids()[:2]) and t['k_ids'].max() == vocab_size - 1
    # the flag marks exactly the sentences with a literal [CLS] / [SEP]
    special = (t['k_ids'] == t['cls_id']) | (t['k_ids'] == t['sep_id'])
    has = np.add.reduceat(np.concatenate([special, [False]]), np.cumsum(lens) - lens)[:len(lens)]
    has = np.where(lens > 0, has, 0) > 0
    np.testing.assert_array_equal((t['sent_len'] & T.LEN_HAS_CLS_SEP) != 0, has)
    assert has.sum() > 10
    # three partitions, none in the middle; documents of dropped sentences only between real ones
    pdo, dso = t['part_doc_off'], t['doc_sent_off']
    assert len(pdo) == 4 and pdo[1] == pdo[2] and pdo[0] == 0 and pdo[3] == len(dso) - 1
    per_doc = np.asarray([lens[dso[d]:dso[d + 1]].sum() for d in range(len(dso) - 1)])
    assert per_doc[0] == 0 and per_doc[-1] == 0 and (per_doc[1:-1] == 0).any()
    assert t['kp_off'][-1] == len(t['k_doc']) - 1 == (per_doc > 0).sum()
    assert t['k_off'][-1] == len(t['k_ids']) and t['k_doc'][-1] == len(t['k_off']) - 1
    # the first and the last kept document have two sentences
    assert t['k_doc'][1] == 2 and t['k_doc'][-1] - t['k_doc'][-2] == 2
