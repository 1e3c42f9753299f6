"""The load balance's row-movement kernels (csrc/output_rows.hip: take, ragged gather, segment
expansion, metadata pack / unpack), HipOps method by method against TorchCpuOps (the numpy
restatement in balance_util.py) on the same inputs; and the C entry points' NULL row index (the
identity), which HipOps never passes."""
import numpy as np
import pytest
import torch

from balance_util import TorchCpuOps, random_table
from conftest import VOCAB_UNCASED

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.int16, np.int32, np.int64]
ROW_COUNTS = [1, 255, 256, 257]
ROW_LENS = np.asarray([0, 1, 63, 64, 65, 200])


@pytest.fixture(scope='module')
def ctx():
    from lddl_amd.context import Context
    return Context(VOCAB_UNCASED, True)


@pytest.fixture(scope='module')
def ops(ctx):
    from lddl_amd.balance import HipOps
    return HipOps(ctx), TorchCpuOps()


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _d(a):
    return None if a is None else _t(a).cuda()


def _values(rng, n, dtype):
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)


def _row_cases(rng, n_a, n_b):
    """(name, rows, uses the second source): empty; below n_a only; at or above n_a only; mixed
    with duplicates; at each of ROW_COUNTS."""
    yield 'empty', np.zeros(0, np.int64), True
    for m in ROW_COUNTS:
        yield 'a{}'.format(m), rng.integers(0, n_a, m).astype(np.int64), False
        yield 'b{}'.format(m), (n_a + rng.integers(0, n_b, m)).astype(np.int64), True
        mixed = rng.integers(0, n_a + n_b, m).astype(np.int64)
        mixed[m // 2:] = mixed[:m - m // 2]  # every row of the first half again
        mixed[0], mixed[-1] = n_a - 1, n_a
        yield 'mixed{}'.format(m), mixed, True


@pytest.mark.parametrize('dtype', DTYPES)
def test_take_vs_cpu(ops, dtype):
    hip, cpu = ops
    rng = np.random.default_rng(np.dtype(dtype).itemsize)
    n_a, n_b = 300, 170
    a, b = _values(rng, n_a, dtype), _values(rng, n_b, dtype)
    for name, rows, two in _row_cases(rng, n_a, n_b):
        bb = b if two else None
        exp = cpu.take(_t(a), n_a, _t(bb), _t(rows)).numpy()
        got = hip.take(_d(a), n_a, _d(bb), _d(rows))
        assert got.dtype == _t(a).dtype and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), exp), name


def _ragged(rng, n, dtype, lead):
    """A ragged source of n rows with lengths from ROW_LENS (each at least once) whose offsets
    start at `lead`, so the two sources' offset tables are not interchangeable."""
    lens = rng.choice(ROW_LENS, n)
    lens[:len(ROW_LENS)] = ROW_LENS
    lens[-2:] = (0, 65)
    off = (lead + np.concatenate([[0], np.cumsum(lens)])).astype(np.int64)
    return _values(rng, int(off[-1]) + 3, dtype), off


@pytest.mark.parametrize('dtype', DTYPES)
def test_gather_vs_cpu(ops, dtype):
    hip, cpu = ops
    rng = np.random.default_rng(10 + np.dtype(dtype).itemsize)
    n_a, n_b = 40, 23
    a, off_a = _ragged(rng, n_a, dtype, 0)
    b, off_b = _ragged(rng, n_b, dtype, 7)
    for name, rows, two in _row_cases(rng, n_a, n_b):
        bb, ob = (b, off_b) if two else (None, None)
        e_off = cpu.ragged_offsets(_t(off_a), n_a, _t(ob), _t(rows))
        d_off = hip.ragged_offsets(_d(off_a), n_a, _d(ob), _d(rows))
        assert np.array_equal(d_off.cpu().numpy(), e_off.numpy()), name
        total = int(e_off[-1])
        exp = cpu.gather(_t(a), _t(off_a), n_a, _t(bb), _t(ob), _t(rows), e_off, total).numpy()
        got = hip.gather(_d(a), _d(off_a), n_a, _d(bb), _d(ob), _d(rows), d_off, total)
        assert got.dtype == _t(a).dtype and got.numel() == total
        assert np.array_equal(got.cpu().numpy(), exp), name


def _segments(rng, lens, n_src, rep):
    """Segment table (start, stride, direct) for the given lengths: strides 1, 0, -1 and 3,
    direct and indirect (segment k takes combination (k + rep) % 8), every element inside src
    (empty segments too, so a wrong segment shows as a wrong value)."""
    seg = []
    for k, L in enumerate(lens):
        stride = (1, 0, -1, 3)[(k + rep) % 4]
        direct = ((k + rep) // 4) % 2
        span = stride * max(int(L) - 1, 0)
        lo, hi = max(0, -span), n_src - 1 - max(0, span)
        seg.append((int(rng.integers(lo, hi + 1)), stride, direct))
    return np.asarray(seg, np.int64).reshape(-1, 3)


def _expand_cases(rng):
    yield 'one segment, one output', [1]
    yield 'one segment, 256', [256]
    yield 'one segment, 257', [257]
    yield 'one segment, 5000', [5000]
    yield 'empty first', [0, 257]
    yield 'empty last', [256, 0]
    yield 'two segments', [1, 255]
    # 257 segments: empty ones first, in the middle, doubled and last
    for total in (1, 256, 257, 5000):
        lens = np.zeros(257, np.int64)
        if total == 1:
            lens[128] = 1
        else:
            cuts = np.sort(rng.integers(0, total + 1, 256 - 9))
            body = np.diff(np.concatenate([[0], cuts, [total]]))
            lens[1:100] = body[:99]
            lens[102:251] = body[99:]  # 100, 101 (doubled), 251 .. 256 and 0 stay empty
        assert lens.sum() == total and lens[0] == 0 and lens[-1] == 0
        yield '257 segments, {}'.format(total), lens


def test_expand_vs_cpu(ops):
    hip, cpu = ops
    rng = np.random.default_rng(3)
    n_src = 20000
    src = rng.integers(-(1 << 40), 1 << 40, n_src, dtype=np.int64)
    d_src = _d(src)
    for name, lens in _expand_cases(rng):
        lens = np.asarray(lens, np.int64)
        seg_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        for rep in range(8):  # rotate which stride / mode each segment gets
            seg = _segments(rng, lens, n_src, rep)
            exp = cpu.expand(_t(src), seg, seg_off, 'cpu').numpy()
            got = hip.expand(d_src, seg, seg_off, d_src.device)
            assert got.dtype == torch.int64 and got.numel() == seg_off[-1]
            assert np.array_equal(got.cpu().numpy(), exp), (name, rep)
    # no outputs at all
    assert hip.expand(d_src, np.zeros((2, 3), np.int64), np.zeros(3, np.int64),
                      d_src.device).numel() == 0


def _on_device(pb):
    from lddl_amd.pairs import PairBatch
    c = lambda x: None if x is None else x.cuda()  # noqa: E731
    return PairBatch(c(pb.tokens), c(pb.tok_off), c(pb.len_a), c(pb.is_random_next), c(pb.pos),
                     c(pb.labels), c(pb.pos_off))


@pytest.mark.parametrize('masking', [True, False])
def test_meta_pack_unpack_vs_cpu(ops, masking):
    from lddl_amd._native import lib
    from lddl_amd.context import _ptr, _stream
    hip, cpu = ops
    rng = np.random.default_rng(20 + masking)
    for n in (0, 1, 255, 256, 257):
        pb = random_table(rng, n, 128, rank=1, masking=masking)
        assert (pb.pos_off is None) == (not masking)
        d_pb = _on_device(pb)
        some = rng.integers(0, max(n, 1), 300).astype(np.int64)[:300 if n else 0]
        for rows in (np.arange(n, dtype=np.int64), some):
            exp = cpu.meta_pack(pb, _t(rows)).numpy()
            got = hip.meta_pack(d_pb, _d(rows))
            assert got.dtype == torch.int32
            assert np.array_equal(got.cpu().numpy(), exp), (n, len(rows))
            back = [x.cpu().numpy() for x in hip.meta_unpack(got)]
            for g, e in zip(back, cpu.meta_unpack(_t(exp))):
                assert g.dtype == e.numpy().dtype and np.array_equal(g, e.numpy()), n
            ntok, len_a, is_rn, nmask = back
            assert np.array_equal(ntok, np.diff(pb.tok_off.numpy())[rows])
            assert np.array_equal(len_a, pb.len_a.numpy()[rows])
            assert np.array_equal(is_rn, pb.is_random_next.numpy()[rows])
            assert np.array_equal(nmask, np.diff(pb.pos_off.numpy())[rows] if masking
                                  else np.zeros(len(rows), np.int64))
        if n:  # no row index at all: the identity
            out = torch.empty(4 * n, dtype=torch.int32, device='cuda')
            assert lib.lddl_pairs_meta_pack(_stream(), _ptr(d_pb.tok_off), _ptr(d_pb.len_a),
                                            _ptr(d_pb.is_random_next), _ptr(d_pb.pos_off), None, n,
                                            _ptr(out)) == 0
            assert np.array_equal(out.cpu().numpy(),
                                  cpu.meta_pack(pb, torch.arange(n)).numpy())


def _last_error():
    from lddl_amd._native import lib
    return (lib.lddl_last_error() or b'').decode()


@pytest.mark.parametrize('dtype', DTYPES)
def test_null_row_index_is_the_identity(ctx, dtype):
    """lddl_take / lddl_gather_ragged / lddl_ragged_offsets with d_rows = NULL: output row i is
    row i of source A; more rows than A holds is an error, not a read past its end."""
    from lddl_amd._native import lib
    from lddl_amd.context import _ptr, _stream
    rng = np.random.default_rng(30 + np.dtype(dtype).itemsize)
    eb = np.dtype(dtype).itemsize
    n_a = 300
    a, off = _ragged(rng, n_a, dtype, 5)
    d_a, d_off = _d(a), _d(off)
    for n in (1, 255, 256, 257, n_a):
        out = torch.empty(n, dtype=d_a.dtype, device='cuda')
        assert lib.lddl_take(_stream(), _ptr(d_a), n_a, None, eb, None, n, _ptr(out)) == 0
        assert np.array_equal(out.cpu().numpy(), a[:n])
        dst_off = torch.empty(n + 1, dtype=torch.int64, device='cuda')
        assert lib.lddl_ragged_offsets(ctx.handle, _stream(), _ptr(d_off), n_a, None, None, n,
                                       _ptr(dst_off)) == 0
        assert np.array_equal(dst_off.cpu().numpy(), off[:n + 1] - off[0])
        total = int(off[n] - off[0])
        dst = torch.empty(max(total, 1), dtype=d_a.dtype, device='cuda')
        assert lib.lddl_gather_ragged(_stream(), _ptr(d_a), _ptr(d_off), n_a, None, None, eb, None,
                                      n, _ptr(dst_off), _ptr(dst)) == 0
        assert np.array_equal(dst[:total].cpu().numpy(), a[off[0]:off[n]])
    out = torch.empty(n_a + 1, dtype=d_a.dtype, device='cuda')
    dst_off = torch.zeros(n_a + 2, dtype=torch.int64, device='cuda')
    assert lib.lddl_take(_stream(), _ptr(d_a), n_a, None, eb, None, n_a + 1, _ptr(out)) != 0
    assert 'without a row index' in _last_error()
    assert lib.lddl_gather_ragged(_stream(), _ptr(d_a), _ptr(d_off), n_a, None, None, eb, None,
                                  n_a + 1, _ptr(dst_off), _ptr(out)) != 0
    assert 'without a row index' in _last_error()
    assert lib.lddl_ragged_offsets(ctx.handle, _stream(), _ptr(d_off), n_a, None, None, n_a + 1,
                                   _ptr(dst_off)) != 0
    assert 'without a row index' in _last_error()


def test_unsupported_element_size(ctx):
    from lddl_amd._native import lib
    from lddl_amd.context import _ptr, _stream
    a = torch.zeros(64, dtype=torch.uint8, device='cuda')
    off = torch.arange(0, 16, 3, dtype=torch.int64, device='cuda')
    rows = torch.zeros(2, dtype=torch.int64, device='cuda')
    out = torch.zeros(64, dtype=torch.uint8, device='cuda')
    assert lib.lddl_take(_stream(), _ptr(a), 5, None, 3, _ptr(rows), 2, _ptr(out)) != 0
    assert 'elem_bytes 3 unsupported' in _last_error()
    assert lib.lddl_gather_ragged(_stream(), _ptr(a), _ptr(off), 5, None, None, 3, _ptr(rows), 2,
                                  _ptr(off), _ptr(out)) != 0
    assert 'elem_bytes 3 unsupported' in _last_error()
    assert lib.lddl_take(_stream(), _ptr(a), -1, None, 1, None, 1, _ptr(out)) != 0
    assert 'bad size' in _last_error()
