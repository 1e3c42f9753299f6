"""The device row planner (lddl_seqpack_plan) against seqpack.plan_rows, array for
array: row * capacity + start, fill, seq_in_row, the inverse of order, and R, for every batch of
a launch."""
import numpy as np
import pytest
import torch

from conftest import VOCAB_UNCASED

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from lddl_amd.context import Context
    return Context(VOCAB_UNCASED)


def _bound():
    from lddl_amd.torch.online import SEQPLAN_MAX_BATCH
    return SEQPLAN_MAX_BATCH


def _expected(lens, cap):
    """plan_rows' arrays of one batch in the planner's layout; a sample longer than cap takes
    no row and the others are planned without it."""
    from lddl_amd.torch.seqpack import plan_rows
    lens = np.asarray(lens, np.int64)
    keep = np.flatnonzero(lens <= cap)
    plan = plan_rows(lens[keep], cap)
    B = len(lens)
    dst, fill = np.full(B, -1, np.int64), np.zeros(B, np.int32)
    seq, at = np.zeros(B, np.int32), np.full(B, -1, np.int32)
    dst[keep] = plan.row.astype(np.int64) * cap + plan.start
    fill[keep] = plan.fill
    seq[keep] = plan.seq_in_row
    inv = np.empty(len(keep), np.int32)
    inv[plan.order] = np.arange(len(keep), dtype=np.int32)
    at[keep] = inv
    return dst, fill, seq, at, plan.R


def _table(lens, source):
    """The length source of a table whose row r has lens[r] tokens: an int32 num_tokens tensor,
    or a PairBatch whose tok_off gives len - 3 tokens per pair."""
    from lddl_amd.pairs import PairBatch
    lens = np.asarray(lens, np.int64)
    if source == 'num_tokens':
        return torch.from_numpy(lens.astype(np.int32)).cuda()
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens - 3)])).cuda()
    n = len(lens)
    return PairBatch(torch.zeros(1, dtype=torch.int16, device='cuda'), off,
                     torch.zeros(n, dtype=torch.int32, device='cuda'),
                     torch.zeros(n, dtype=torch.uint8, device='cuda'))


def _check(ctx, batches, cap, source='num_tokens', rows='none', seed=0):
    """Plan `batches` (a list of length arrays) in one launch and compare every batch. rows:
    'none' (the identity), 'perm' (the table shuffled) or 'subset' (rows scattered over a table
    three times as large)."""
    from lddl_amd.torch.online import plan_rows_device
    lens = np.concatenate([np.asarray(b, np.int64) for b in batches] + [np.zeros(0, np.int64)])
    off = np.concatenate([[0], np.cumsum([len(b) for b in batches])]).astype(np.int64)
    n = len(lens)
    rng = np.random.default_rng(seed)
    d_rows, table = None, lens
    if rows != 'none':
        size = n if rows == 'perm' else 3 * n
        pick = rng.permutation(size)[:n]
        table = rng.integers(3, cap + 1, size)  # the rows not picked: any length
        table[pick] = lens
        d_rows = torch.from_numpy(pick.astype(np.int64)).cuda()
    plan = plan_rows_device(ctx, _table(table, source), d_rows, off, cap)
    got = [t.cpu().numpy() for t in plan.tensors()]
    assert [g.dtype for g in got] == [np.int64, np.int32, np.int32, np.int32, np.int32]
    assert all(len(g) == n for g in got[:4]) and len(got[4]) == len(batches)
    for k, b in enumerate(batches):
        exp = _expected(b, cap)
        s = slice(off[k], off[k + 1])
        for name, g, e in zip(('dst', 'fill', 'seq_in_row', 'packed_idx'), got, exp):
            np.testing.assert_array_equal(g[s], e, err_msg='{} of batch {}'.format(name, k))
        assert got[4][k] == exp[4], 'R of batch {}'.format(k)
    return plan, got


def _rand(rng, B, lo, hi):
    return rng.integers(lo, hi + 1, B)


@pytest.mark.parametrize('B', [1, 63, 64, 65, 129])
@pytest.mark.parametrize('source', ['num_tokens', 'tok_off'])
def test_lane_edges(ctx, B, source):
    rng = np.random.default_rng(B)
    _check(ctx, [_rand(rng, B, 3, 128)], 128, source)


@pytest.mark.parametrize('rows', ['none', 'perm', 'subset'])
def test_halves_full_rows_and_rows_that_take_nothing_more(ctx, rows):
    """Capacity 128, lengths from {64, 65, 128}: two 64s fill a row, a 65 leaves 63 slots that
    nothing takes, a 128 fills its row alone."""
    rng = np.random.default_rng(5)
    lens = rng.choice([64, 65, 128], 200)
    _, got = _check(ctx, [lens], 128, 'tok_off', rows, seed=6)
    n64 = int((lens == 64).sum())
    assert got[4][0] == int((lens != 64).sum()) + (n64 + 1) // 2


def test_equal_lengths_are_placed_by_index(ctx):
    _, got = _check(ctx, [np.full(100, 40)], 128)  # three to a row, in index order
    np.testing.assert_array_equal(got[3], np.arange(100))
    np.testing.assert_array_equal(got[0][:4], [0, 40, 80, 128])


@pytest.mark.parametrize('B', [65, 'bound'])
def test_every_sample_its_own_row(ctx, B):
    """All lengths > capacity / 2: R = B, across a 64-row group and at the bound."""
    B = _bound() if B == 'bound' else B
    rng = np.random.default_rng(11)
    _, got = _check(ctx, [_rand(rng, B, 65, 128)], 128)
    assert got[4][0] == B


def test_all_ones_capacity_8(ctx):
    _, got = _check(ctx, [np.ones(100, np.int64)], 8)
    assert got[4][0] == 13 and got[2].max() == 8


def test_one_long_and_127_short(ctx):
    _check(ctx, [np.array([4] * 60 + [128] + [4] * 67)], 128)
    _check(ctx, [np.array([4] * 60 + [100] + [4] * 67)], 128, 'tok_off')


@pytest.mark.parametrize('cap,lo,hi', [(512, 3, 512), (128, 3, 128), (512, 3, 40)])
def test_random_lengths_at_the_bound(ctx, cap, lo, hi):
    rng = np.random.default_rng(cap + hi)
    _check(ctx, [_rand(rng, _bound(), lo, hi)], cap, 'tok_off', 'perm', seed=1)


@pytest.mark.parametrize('source', ['num_tokens', 'tok_off'])
@pytest.mark.parametrize('rows', ['none', 'subset'])
def test_batches_of_different_sizes_in_one_launch(ctx, source, rows):
    rng = np.random.default_rng(21)
    sizes = [256, 1, 0, 64, 65, 300, 0, 7]
    plan, got = _check(ctx, [_rand(rng, B, 3, 128) for B in sizes], 128, source, rows, seed=2)
    assert got[4][2] == 0 and got[4][6] == 0  # the empty batches
    assert plan.batch_off == np.concatenate([[0], np.cumsum(sizes)]).tolist()


def test_no_batches(ctx):
    from lddl_amd.torch.online import plan_rows_device
    plan = plan_rows_device(ctx, _table([5, 6], 'num_tokens'), None, [], 128)
    assert plan.num_rows.numel() == 0
    _check(ctx, [[]], 128)  # one empty batch: R = 0


def test_sample_longer_than_capacity_takes_no_row(ctx):
    rng = np.random.default_rng(31)
    lens = _rand(rng, 70, 3, 64)
    lens[[0, 33, 69]] = [65, 200, 66]
    _, got = _check(ctx, [lens, _rand(rng, 10, 3, 64)], 64)
    assert (got[0][[0, 33, 69]] == -1).all() and (got[1][[0, 33, 69]] == 0).all()


def test_refusals(ctx):
    from lddl_amd._native import lib
    from lddl_amd.context import _ptr, _stream
    from lddl_amd.torch.online import plan_rows_device
    bound = _bound()
    n = bound + 1
    with pytest.raises(ValueError, match=str(bound)):  # the wrapper: before anything is launched
        plan_rows_device(ctx, _table(np.full(n, 8), 'num_tokens'), None, [0, n], 128)
    with pytest.raises(ValueError, match='capacity'):
        plan_rows_device(ctx, _table([5], 'num_tokens'), None, [0, 1], 0)
    with pytest.raises(ValueError, match='batch_off'):
        plan_rows_device(ctx, _table([5, 6], 'num_tokens'), None, [0, 1], 128)
    nt = torch.full((n,), 8, dtype=torch.int32, device='cuda')
    off = torch.tensor([0, n], device='cuda')
    i64 = torch.full((n,), 77, dtype=torch.int64, device='cuda')
    i32 = [torch.full((n,), 77, dtype=torch.int32, device='cuda') for _ in range(4)]
    outs = (_ptr(i64), _ptr(i32[0]), _ptr(i32[1]), _ptr(i32[2]), _ptr(i32[3]))

    def call(c=ctx.handle, ntok=_ptr(nt), tok_off=None, rows=n, cap=128, o=outs, nb=1):
        return lib.lddl_seqpack_plan(c, _stream(), ntok, tok_off, None, rows, _ptr(off), nb, cap,
                                     *o)
    assert call() == -1  # B = bound + 1
    assert str(bound).encode() in lib.lddl_last_error()
    assert call(c=None, rows=8) == -1
    assert b'null ctx' in lib.lddl_last_error()
    for k in range(5):
        assert call(rows=8, o=outs[:k] + (None,) + outs[k + 1:]) == -1
        assert b'null output' in lib.lddl_last_error()
    assert call(rows=8, ntok=None) == -1  # both length sources NULL
    assert b'null lengths' in lib.lddl_last_error()
    assert call(rows=8, cap=0) == -1
    assert b'capacity' in lib.lddl_last_error()
    assert call(rows=8, nb=0) == 0 and call(rows=8, nb=-2) == 0
    torch.cuda.synchronize()
    assert int((i64 != 77).sum()) == 0 and all(int((t != 77).sum()) == 0 for t in i32)
