"""The device-wide exclusive scan (csrc/scan.h, and scan.hip with
lddl_scan_i64) by itself against np.cumsum: wave and
tile edges, the single-workgroup scan of the tile sums across its carry loop (more than 256
tiles of 2048 elements), 64-bit values whose low halves carry into the high halves, and the
functor instantiation behind HipOps.ragged_offsets against TorchCpuOps."""
import numpy as np
import pytest
import torch

from conftest import VOCAB_UNCASED

pytestmark = pytest.mark.gpu

TILE = 2048            # kScanTile
CARRY = 256 * TILE     # elements per iteration of scan_sums_block's carry loop
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE, CARRY - 1, CARRY,
         CARRY + 1, 2 * CARRY + TILE + 5]


@pytest.fixture(scope='module')
def ctx():
    from lddl_amd.context import Context
    return Context(VOCAB_UNCASED, True)


def _value_sets(n):
    rng = np.random.default_rng(1000 + n % 9973)
    return {'ones': np.ones(n, np.int64),
            'u33': rng.integers(0, 1 << 33, n, dtype=np.int64),
            's40': rng.integers(-(1 << 40), 1 << 40, n, dtype=np.int64)}


@pytest.mark.parametrize('n', SIZES)
def test_scan_vs_cumsum(ctx, n):
    from lddl_amd.output import scan
    for name, x in _value_sets(n).items():
        out = scan(ctx, torch.from_numpy(x).cuda()).cpu().numpy()
        assert out.dtype == np.int64 and out.shape == (n + 1,)
        inc = np.cumsum(x, dtype=np.int64)
        exp = np.concatenate([np.zeros(1, np.int64), inc[:-1]])[:n]
        bad = np.flatnonzero(out[:-1] != exp)
        assert bad.size == 0, '{} n={}: first difference at {}'.format(name, n, bad[0])
        assert out[-1] == (inc[-1] if n else 0), (name, n)


@pytest.mark.parametrize('n', SIZES)
def test_ragged_offsets_vs_cpu(ctx, n):
    """Row sizes read through the two-source offset tables (rows >= n_a from table B, whose
    offsets differ from A's), scanned by the functor instantiation of the same scan."""
    from balance_util import TorchCpuOps
    from lddl_amd.balance import HipOps
    rng = np.random.default_rng(77 + n % 9973)
    n_a, n_b = 1000, 700
    off_a = np.concatenate([[0], np.cumsum(rng.integers(0, 300, n_a))]).astype(np.int64)
    off_b = np.concatenate([[5], 5 + np.cumsum(rng.integers(200, 5000, n_b))]).astype(np.int64)
    rows = rng.integers(0, n_a + n_b, n).astype(np.int64)
    if n:
        rows[-1] = n_a + n_b - 1
        rows[0] = n_a
    t = lambda a: torch.from_numpy(a)  # noqa: E731
    exp = TorchCpuOps().ragged_offsets(t(off_a), n_a, t(off_b), t(rows)).numpy()
    got = HipOps(ctx).ragged_offsets(t(off_a).cuda(), n_a, t(off_b).cuda(), t(rows).cuda())
    got = got.cpu().numpy()
    assert got.dtype == np.int64
    assert np.array_equal(got, exp)
    # rows all below n_a need no second table
    rows_a = rows % n_a
    exp = TorchCpuOps().ragged_offsets(t(off_a), n_a, None, t(rows_a)).numpy()
    got = HipOps(ctx).ragged_offsets(t(off_a).cuda(), n_a, None, t(rows_a).cuda()).cpu().numpy()
    assert np.array_equal(got, exp)
