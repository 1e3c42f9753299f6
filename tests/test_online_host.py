"""Host pieces of the online loader (lddl_amd/torch/online.py), no GPU: the cut of a round into
batches with its carry, the step order, the round count and the argument validation."""
import numpy as np
import pytest

from conftest import VOCAB_UNCASED


def test_cut_round_conserves_rows():
    from lddl_amd.torch.online import cut_round
    new = np.array([0, 7, 64, 65, 3], np.int64)
    carry = np.array([0, 1, 0, 31, 29], np.int64)
    batches, left = cut_round(new, carry, 32)
    np.testing.assert_array_equal(batches, [0, 0, 2, 3, 1])
    np.testing.assert_array_equal(left, [0, 8, 0, 0, 0])
    np.testing.assert_array_equal(batches * 32 + left, new + carry)  # nothing lost, nothing made
    # all zeros: nothing to yield, nothing carried
    b0, l0 = cut_round(np.zeros(3, np.int64), np.zeros(3, np.int64), 4)
    assert not b0.any() and not l0.any()
    # batch_size 1 never carries
    b1, l1 = cut_round(new, carry, 1)
    np.testing.assert_array_equal(b1, new + carry)
    assert not l1.any()
    # the end of an epoch: one short batch per non-empty bin, no carry
    bf, lf = cut_round(np.zeros(5, np.int64), left, 32, flush=True)
    np.testing.assert_array_equal(bf, [0, 1, 0, 0, 0])
    assert not lf.any()
    with pytest.raises(ValueError):
        cut_round(new, carry[:3], 32)
    with pytest.raises(ValueError):
        cut_round(new, carry, 0)


def test_cut_round_agreement_and_a_rank_out_of_partitions():
    """Two ranks over rounds: every rank yields min over the ranks per bin, the rest stays in
    its carry; a rank whose partitions ran out contributes zeros and keeps cutting its carry."""
    from lddl_amd.torch.online import cut_round
    bs = 8
    rounds = [(np.array([20, 3, 9]), np.array([9, 30, 8])),
              (np.array([5, 0, 17]), np.array([0, 0, 0])),   # rank 1 is out of partitions
              (np.array([1, 14, 0]), np.array([0, 0, 0]))]
    carry = [np.zeros(3, np.int64), np.zeros(3, np.int64)]
    total = [np.zeros(3, np.int64), np.zeros(3, np.int64)]
    yielded = np.zeros(3, np.int64)
    for new in rounds:
        local = [cut_round(new[r], carry[r], bs)[0] for r in range(2)]
        agreed = np.minimum(*local)
        for r in range(2):
            b, left = cut_round(new[r], carry[r], bs, agreed=agreed)
            np.testing.assert_array_equal(b, agreed)
            np.testing.assert_array_equal(b * bs + left, new[r] + carry[r])
            carry[r] = left
            total[r] += new[r]
        yielded += agreed
    # over the epoch: batches = min over ranks of rows // batch_size, per bin
    np.testing.assert_array_equal(yielded, np.minimum(total[0] // bs, total[1] // bs))
    for r in range(2):
        np.testing.assert_array_equal(carry[r], total[r] - bs * yielded)


def test_step_order_is_a_function_of_the_seed_and_honours_the_counts():
    from lddl_amd.torch.online import mix_seed, step_order
    sizes = [[4, 4, 4], [], [4], [4, 4, 4, 4, 2]]
    a = step_order(mix_seed(12345, 0, 3), sizes)
    assert a == step_order(mix_seed(12345, 0, 3), [list(s) for s in sizes])
    assert [a.count(b) for b in range(4)] == [3, 0, 1, 5]
    others = [step_order(mix_seed(12345, e, r), sizes) for e in range(3) for r in range(4)
              if (e, r) != (0, 3)]
    assert any(o != a for o in others)
    assert step_order(7, [[], []]) == []
    # Binned's rule: the draw is random.Random(seed).choices(bins, weights=rows remaining)
    import random
    rnd = random.Random(99)
    remaining, exp = [8, 0, 6], []
    per = [[4, 4], [], [4, 2]]
    nxt = [0, 0, 0]
    while sum(remaining):
        b = rnd.choices([0, 1, 2], weights=remaining, k=1)[0]
        remaining[b] -= per[b][nxt[b]]
        nxt[b] += 1
        exp.append(b)
    assert step_order(99, per) == exp


def test_mix_seed_separates_its_parts():
    from lddl_amd.torch.online import mix_seed
    seen = {mix_seed(1, e, r, k, b) for e in range(3) for r in range(3) for k in range(3)
            for b in range(3)}
    assert len(seen) == 81
    assert mix_seed(1, 2) != mix_seed(2, 1) and 0 <= mix_seed(-5, 3) < 1 << 64


def _corpus(tmp_path):
    d = tmp_path / 'source'
    d.mkdir()
    for k in range(3):
        (d / 'f{}.txt'.format(k)).write_text(''.join(
            'doc-{}-{} One sentence here. Another one follows it.\n'.format(k, i)
            for i in range(50)))
    return str(d)


def test_count_rounds_matches_the_reader_plan(tmp_path):
    from types import SimpleNamespace
    from lddl_amd.dask.bert.corpus import plan_partitions, rank_batches
    from lddl_amd.torch.online import count_rounds
    src = _corpus(tmp_path)
    ns = SimpleNamespace(wikipedia=None, books=src, common_crawl=None, wikipedia_lang='en',
                         block_size=1000, num_blocks=None, sample_ratio=1.0, seed=1,
                         gpu_batch_bytes=2500, shuffle_group_bytes=5000)
    blocks = plan_partitions(ns)
    assert len(blocks) > 6
    for world in (1, 2, 3):
        tot = 0
        for r in range(world):
            n = count_rounds(ns, blocks, r, world)
            assert n >= len(rank_batches(ns, blocks, r, world)) >= 1
            tot += n
        assert tot >= len(blocks) * 1000 // 2500
    ns.gpu_batch_bytes = 1 << 30
    assert count_rounds(ns, blocks, 0, 1) == len(rank_batches(ns, blocks, 0, 1))


def test_invalid_arguments_raise_before_any_device_call(tmp_path, monkeypatch):
    import lddl_amd.context as C
    from lddl_amd.torch import get_bert_pretrain_online_data_loader as make

    def boom(*a, **k):
        raise AssertionError('the GPU was touched')
    monkeypatch.setattr(C.Context, '__init__', boom)
    src = _corpus(tmp_path)
    ok = dict(books=src, vocab_file=VOCAB_UNCASED, batch_size=8)
    with pytest.raises(ValueError, match='divide'):
        make(**ok, target_seq_length=128, bin_size=24)
    with pytest.raises(ValueError, match='<= target-seq-length'):
        make(**ok, target_seq_length=128, bin_size=256)
    with pytest.raises(ValueError, match='no corpus'):
        make(vocab_file=VOCAB_UNCASED, batch_size=8)
    with pytest.raises(FileNotFoundError):
        make(books=src, vocab_file=str(tmp_path / 'missing.txt'), batch_size=8)
    with pytest.raises(FileNotFoundError):
        make(books=str(tmp_path / 'nowhere'), vocab_file=VOCAB_UNCASED, batch_size=8)
    with pytest.raises(ValueError, match='Only one of'):
        make(**ok, block_size=1 << 20, num_blocks=4)
    with pytest.raises(ValueError, match="rng='native'"):
        make(**ok, static_masking=True, whole_word_masking=True, rng='replay')
    with pytest.raises(ValueError):
        make(books=src, vocab_file=VOCAB_UNCASED, batch_size=0)
    with pytest.raises(ValueError):
        make(**ok, rank=2, world=2)
    # valid arguments build the loader without a device, and it has no length
    loader = make(**ok, bin_size=32, static_masking=True, whole_word_masking=True, rng='native')
    assert loader.nbins == 4
    with pytest.raises(TypeError, match='no length'):
        len(loader)
