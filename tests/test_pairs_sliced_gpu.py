"""The time-sliced replay plan (LDDL_PLAN_SLICE forcing it at small sizes, LDDL_PLAN_WAVES the
number of persistent waves): partitions parked at document boundaries and taken up by other
waves give the output of the one-shot plan, bit for bit - against the reference goldens and the
oracle."""
import numpy as np
import pytest

import test_pairs_gpu as TP
from alloc_util import OWN_ARENA, allocated, needs_torch_arena
from conftest import VOCAB_UNCASED
from test_pairs_gpu import ctx, docs_dev  # noqa: F401  (module-scoped fixtures)
from test_pairs_split_gpu import check_batch, golden_doc_inputs, golden_docs, oracle_batch  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture
def traces(monkeypatch):
    """Every make_pairs call of the test reports its _trace here (the golden and oracle checks of
    test_pairs_gpu call make_pairs themselves)."""
    import lddl_amd.pairs as LP
    seen = []
    real = LP.make_pairs

    def traced(*a, **kw):
        tr = kw.setdefault('_trace', {})
        out = real(*a, **kw)
        seen.append(tr)
        return out

    monkeypatch.setattr(LP, 'make_pairs', traced)
    return seen


@pytest.mark.parametrize('quantum', [1, 7, 10 ** 6])
@pytest.mark.parametrize('name', ['s128_mask', 's512_mask', 's64_mask_ratio', 's128_nomask'])
def test_sliced_goldens(name, quantum, ctx, docs_dev, monkeypatch, traces):  # noqa: F811
    """A quantum of 1 and of 7 documents (hand-offs at every and at every seventh document
    boundary) and one longer than any partition (no hand-off) against the reference goldens."""
    monkeypatch.setenv('LDDL_PLAN_SLICE', str(quantum))
    TP.test_pairs_golden_gpu(name, ctx, docs_dev)
    (tr,) = traces
    assert tr['split'] == 0 and tr['path'] == 'full', tr
    assert (tr['slices'] > 0) if quantum < 10 ** 6 else (tr['slices'] == 0), tr


@pytest.fixture(scope='module')
def eight_parts(golden_docs):  # noqa: F811
    """The golden documents as 8 partitions with the oracle's output for the two cases of the
    split test, computed once."""
    text, sent_off, line_off = golden_docs
    part = np.linspace(0, len(line_off) - 1, 9).astype(np.int64)
    seeds = np.arange(31, 39, dtype=np.int64)
    exp = {(seq, dup, ratio): oracle_batch(VOCAB_UNCASED, text, sent_off, line_off, part, seeds, dup, seq, ratio)
           for seq, dup, ratio in ((512, 3, 0.15), (64, 4, 0.3))}
    return part, seeds, exp


@pytest.mark.parametrize('waves', [1, 2, 3, 8])
@pytest.mark.parametrize('seq,dup,ratio', [(512, 3, 0.15), (64, 4, 0.3)])
def test_sliced_eight_partitions_vs_oracle(ctx, docs_dev, eight_parts, monkeypatch, seq, dup, ratio,  # noqa: F811
                                           waves):
    """Quantum 1 on 1, 2 and 3 waves (more partitions than waves: the queue holds waiting
    partitions, they migrate between waves, and a wave reads again a save area it read before)
    and on 8 (every partition resident); every column against the oracle, and two runs against
    each other."""
    from lddl_amd.pairs import make_pairs
    part, seeds, exp_all = eight_parts
    exp, part_off = exp_all[(seq, dup, ratio)]
    assert len(exp['len_a']) > 0
    kw = golden_doc_inputs(docs_dev, part, seeds)
    monkeypatch.setenv('LDDL_PLAN_SLICE', '1')
    monkeypatch.setenv('LDDL_PLAN_WAVES', str(waves))
    runs = []
    for _ in range(2):
        tr = {}
        pb = make_pairs(ctx, seq=seq, dup=dup, masking=True, masked_lm_ratio=ratio, _trace=tr, **kw)
        assert tr['split'] == 0 and tr['path'] == 'full' and tr['slices'] > 0, tr
        check_batch(pb, exp, part_off)
        runs.append(pb.to_host())
    assert sorted(runs[0]) == sorted(runs[1])
    for k in runs[0]:
        np.testing.assert_array_equal(runs[0][k], runs[1][k])


def test_sliced_empty_partitions(ctx, docs_dev, golden_docs, monkeypatch):  # noqa: F811
    """Empty partitions at the start, in the middle and at the end (the split test's layout):
    they finish without a slice of their own work, between partitions that are parked."""
    from lddl_amd.pairs import make_pairs
    text, sent_off, line_off = golden_docs
    n = len(line_off) - 1
    part = np.asarray([0, 0, n // 3, n // 3, n // 3, 2 * n // 3, n, n], np.int64)  # 7 partitions
    seeds = np.arange(51, 58, dtype=np.int64)
    exp, part_off = oracle_batch(VOCAB_UNCASED, text, sent_off, line_off, part, seeds, 2, 128)
    assert part_off[1] == 0 and part_off[-1] == part_off[-2] and part_off[3] == part_off[4]
    monkeypatch.setenv('LDDL_PLAN_SLICE', '1')
    monkeypatch.setenv('LDDL_PLAN_WAVES', '2')
    tr = {}
    pb = make_pairs(ctx, seq=128, dup=2, masking=True, _trace=tr, **golden_doc_inputs(docs_dev, part, seeds))
    assert tr['split'] == 0 and tr['slices'] > 0, tr
    check_batch(pb, exp, part_off)


def test_sliced_large_partition(ctx, monkeypatch, traces):  # noqa: F811
    """A partition of more than 512 documents (the document table read from global memory),
    parked at every document boundary."""
    monkeypatch.setenv('LDDL_PLAN_SLICE', '1')
    TP.test_pairs_large_partition_vs_oracle(ctx)
    assert traces and all(tr['slices'] > 600 for tr in traces), traces


def test_sliced_empty_and_dropped_inputs(ctx, monkeypatch, traces):  # noqa: F811
    """No partitions, partitions of dropped sentences only, and dropped documents between real
    ones, with quantum 1."""
    monkeypatch.setenv('LDDL_PLAN_SLICE', '1')
    TP.test_pairs_empty_and_dropped_inputs(ctx)
    assert [tr['slices'] > 0 for tr in traces] == [False, False, True], traces


def test_sliced_pool_overflow_replans(ctx, docs_dev, monkeypatch, traces):  # noqa: F811
    """A mask pool that overflows under a sliced plan: planned again, sliced, with the exact
    sizes (the pool chunks travel with the partitions, so the sizes do not depend on which wave
    planned which slice); the output is the golden."""
    monkeypatch.setenv('LDDL_AMD_MASK_POOL', '100')
    for quantum, waves in ((1, 2), (7, 64)):
        monkeypatch.setenv('LDDL_PLAN_SLICE', str(quantum))
        monkeypatch.setenv('LDDL_PLAN_WAVES', str(waves))
        TP.test_pairs_golden_gpu('s128_mask', ctx, docs_dev)
    assert len(traces) == 2 and all(tr['slices'] > 0 and tr['path'] == 'full' for tr in traces), traces


@pytest.mark.parametrize('value', ['-2', 'x', '', '1.5'])
def test_sliced_rejects_unsupported_knob(ctx, docs_dev, monkeypatch, value):  # noqa: F811
    """Anything but -1, 0 or a quantum fails the call with the knob's name and keeps none of the
    allocator's memory; the same context then plans the case."""
    from lddl_amd.pairs import make_pairs
    _, kw = TP.case_inputs('s128_mask', docs_dev)
    monkeypatch.setenv('LDDL_PLAN_SLICE', value)
    before = allocated()
    with pytest.raises(Exception, match='LDDL_PLAN_SLICE'):
        make_pairs(ctx, **kw)
    if not OWN_ARENA:
        assert allocated() == before
    monkeypatch.setenv('LDDL_PLAN_SLICE', '-1')
    TP.test_pairs_golden_gpu('s128_mask', ctx, docs_dev)


def test_sliced_and_split_both_forced(ctx, docs_dev, monkeypatch):  # noqa: F811
    """Both knobs positive: refused, naming both. LDDL_PLAN_SPLIT alone still splits."""
    from lddl_amd.pairs import make_pairs
    _, kw = TP.case_inputs('s128_mask', docs_dev)
    monkeypatch.setenv('LDDL_PLAN_SPLIT', '2')
    monkeypatch.setenv('LDDL_PLAN_SLICE', '3')
    with pytest.raises(Exception, match='LDDL_PLAN_SPLIT.*LDDL_PLAN_SLICE'):
        make_pairs(ctx, **kw)
    monkeypatch.delenv('LDDL_PLAN_SLICE')
    tr = {}
    make_pairs(ctx, _trace=tr, **kw)
    assert tr['split'] == 1 and tr['slices'] == 0, tr
    # a split switched off and a forced slice: sliced
    monkeypatch.setenv('LDDL_PLAN_SPLIT', '0')
    monkeypatch.setenv('LDDL_PLAN_SLICE', '3')
    tr = {}
    make_pairs(ctx, _trace=tr, **kw)
    assert tr['split'] == 0 and tr['slices'] > 0, tr


@pytest.mark.parametrize('value', ['0', '-2', 'x', ''])
def test_sliced_rejects_unsupported_waves(ctx, docs_dev, monkeypatch, value):  # noqa: F811
    from lddl_amd.pairs import make_pairs
    _, kw = TP.case_inputs('s128_mask', docs_dev)
    monkeypatch.setenv('LDDL_PLAN_WAVES', value)
    with pytest.raises(Exception, match='LDDL_PLAN_WAVES'):
        make_pairs(ctx, **kw)


@needs_torch_arena
def test_failed_sliced_plan_returns_its_blocks(ctx, docs_dev, monkeypatch):  # noqa: F811
    """A plan that fails after the compaction took its blocks, with slicing forced, gives every
    block back; so does a sliced plan that succeeds (with and without the re-plan), once its batch
    is deleted."""
    from lddl_amd.pairs import make_pairs
    monkeypatch.setenv('LDDL_PLAN_SLICE', '1')
    _, kw = TP.case_inputs('s512_nomask_short', docs_dev)
    kw.update(masking=False, seq=600)
    before = allocated()
    with pytest.raises(Exception, match='replay planner supports target_seq_length <= 512'):
        make_pairs(ctx, **kw)
    assert allocated() == before
    _, kw = TP.case_inputs('s128_mask', docs_dev)
    for env in ({}, {'LDDL_AMD_MASK_POOL': '100'}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        tr = {}
        pb = make_pairs(ctx, _trace=tr, **kw)
        assert tr['slices'] > 0 and pb.tokens.numel() > 0 and allocated() > before
        del pb
        assert allocated() == before
