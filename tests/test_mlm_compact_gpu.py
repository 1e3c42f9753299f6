"""lddl_mlm_compact_rows / lddl_mlm_compact_flat and compact_labels against a
numpy restatement, bit for bit. The entry points are called with every output pre-filled with a
sentinel, so an element the kernels did not write shows up; the Python path gets the same through
a torch.empty that fills what it returns."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = {torch.int64: -7777, torch.float32: -3.0, torch.int32: -9}


# ---- the restatement --------------------------------------------------------------------------
def ref_rows(lab, P, ign):
    R = lab.shape[0]
    pos = np.zeros((R, P), np.int64)
    ids = np.full((R, P), ign, np.int64)
    w = np.zeros((R, P), np.float32)
    num = np.zeros(R, np.int32)
    for r in range(R):
        x = np.flatnonzero(lab[r] != ign)
        num[r] = len(x)
        k = min(len(x), P)
        pos[r, :k] = x[:k]
        ids[r, :k] = lab[r, x[:k]]
        w[r, :k] = 1
    return pos, ids, w, num


def ref_flat(lab, cap, ign):
    x = np.flatnonzero(lab.reshape(-1) != ign)
    pos = np.zeros(cap, np.int64)
    ids = np.full(cap, ign, np.int64)
    k = min(len(x), cap)
    pos[:k] = x[:k]
    ids[:k] = lab.reshape(-1)[x[:k]]
    num = (lab != ign).sum(1).astype(np.int32).reshape(lab.shape[0])
    return pos, ids, num, np.asarray([len(x)], np.int64)


# ---- direct calls, outputs pre-filled ---------------------------------------------------------
def _full(n, dtype):
    return torch.full((max(n, 1),), SENT[dtype], dtype=dtype, device='cuda')


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def call_rows(lab, P, ign):
    """-> (status, [positions, ids, weights, num_masked] as flat numpy arrays)."""
    from lddl_amd._native import lib
    R, L = lab.shape
    d = torch.from_numpy(lab).cuda()
    o = [_full(R * P, torch.int64), _full(R * P, torch.int64), _full(R * P, torch.float32),
         _full(R, torch.int32)]
    st = lib.lddl_mlm_compact_rows(_stream(), ctypes.c_void_p(d.data_ptr()) if d.numel() else
                                   ctypes.c_void_p(o[0].data_ptr()), R, L, ign, P,
                                   *(ctypes.c_void_p(t.data_ptr()) for t in o))
    return st, [t.cpu().numpy() for t in o]


def call_flat(lab, cap, ign):
    from lddl_amd._native import lib
    R, L = lab.shape
    d = torch.from_numpy(lab).cuda()
    o = [_full(cap, torch.int64), _full(cap, torch.int64), _full(R, torch.int32),
         _full(1, torch.int64)]
    st = lib.lddl_mlm_compact_flat(_stream(), ctypes.c_void_p(d.data_ptr()) if d.numel() else
                                   ctypes.c_void_p(o[0].data_ptr()), R, L, ign, cap,
                                   *(ctypes.c_void_p(t.data_ptr()) for t in o))
    return st, [t.cpu().numpy() for t in o]


def check_rows(lab, P, ign, tag=''):
    st, got = call_rows(lab, P, ign)
    assert st == 0, tag
    R = lab.shape[0]
    exp = ref_rows(lab, P, ign)
    for g, e, n, name in zip(got, exp, (R * P, R * P, R * P, R), ('positions', 'ids', 'weights',
                                                                  'num_masked')):
        np.testing.assert_array_equal(g[:n], e.reshape(-1), err_msg='{} {}'.format(name, tag))


def check_flat(lab, cap, ign, tag=''):
    st, got = call_flat(lab, cap, ign)
    assert st == 0, tag
    exp = ref_flat(lab, cap, ign)
    for g, e, n, name in zip(got, exp, (cap, cap, lab.shape[0], 1), ('positions', 'ids',
                                                                     'num_masked', 'total')):
        np.testing.assert_array_equal(g[:n], e, err_msg='{} {}'.format(name, tag))


# ---- the cases --------------------------------------------------------------------------------
def patterns(L, P, ign, rng):
    """Rows of L labels, one per edge: name -> int64[L]."""
    def row(slots, value=None):
        r = np.full(L, ign, np.int64)
        slots = np.asarray(sorted(slots), np.int64)
        r[slots] = rng.integers(1, 30522, len(slots)) if value is None else value
        return r
    out = {
        'none': row([]),
        'all': row(range(L)),
        'first': row([0]),
        'last': row([L - 1]),
        'zero_label': row([L // 2], 0),  # a label of value 0 is a masked slot
        'random': np.where(rng.random(L) < 0.15, rng.integers(0, 30522, L), ign).astype(np.int64),
    }
    if L >= P:  # exactly P: no padding, no overflow; spread over the row, both ends included
        out['exactly_P'] = row(np.unique(np.linspace(0, L - 1, P).round().astype(int))
                               if P > 1 else [L - 1])
        if len(np.flatnonzero(out['exactly_P'] != ign)) != P:
            out['exactly_P'] = row(range(L - P, L))
    if L >= P + 1:  # overflow by one: the last masked slot is the one dropped
        out['P_plus_1'] = row(range(L - P - 1, L))
    if L >= 65:
        out['63_64'] = row([63, 64])  # the two sides of a window boundary
    if L >= 2:
        out['neg_labels'] = row([0, L - 1], -5)  # only ignore_index ignores
    return out


def matrices(L, R, P, ign, rng):
    """Enough [R, L] matrices that every pattern sits in some row, rotated so that each also
    meets different neighbours; then one all-random matrix."""
    pats = patterns(L, P, ign, rng)
    names = list(pats)
    for k in range(0, len(names), R):
        rows = [names[(k + i) % len(names)] for i in range(R)]
        yield '+'.join(rows), np.stack([pats[n] for n in rows])
    yield 'random', np.where(rng.random((R, L)) < 0.15, rng.integers(0, 30522, (R, L)),
                             ign).astype(np.int64)


LS = (1, 8, 63, 64, 65, 128, 129, 512)
RS = (1, 3, 4, 5, 9)  # below, at and above a block of four waves


@pytest.mark.parametrize('L', LS)
def test_rows(L):
    rng = np.random.default_rng(1000 + L)
    seen = set()
    for ign in (-1, -100):
        for P in sorted({1, 20, L, L + 3}):
            for R in RS:
                for name, lab in matrices(L, R, P, ign, rng):
                    check_rows(lab, P, ign, 'L {} R {} P {} ign {} {}'.format(L, R, P, ign, name))
                    seen.update(name.split('+'))
    assert {'none', 'all', 'first', 'last', 'zero_label', 'random', 'exactly_P'} <= seen
    assert ('63_64' in seen) == (L >= 65) and ('P_plus_1' in seen) == (L >= 2)


def _capacities(lab, ign, P):
    """Capacity in the middle of a row, at the total, above it, 1, and the Python side's R * P."""
    n = (lab != ign).sum(1)
    total = int(n.sum())
    caps = {1, total + 3, max(total, 1), lab.shape[0] * P}
    mid = [int(n[:r].sum()) + int(n[r]) // 2 for r in range(len(n)) if n[r] >= 2]
    if mid:
        caps.add(mid[len(mid) // 2])  # cuts a row that has slots on both sides of it
    return sorted(caps)


@pytest.mark.parametrize('L', LS)
def test_flat(L):
    rng = np.random.default_rng(2000 + L)
    cut = empty = 0
    for ign in (-1, -100):
        for P in sorted({1, 20, L, L + 3}):  # (P sets the patterns and the capacity R * P)
            for R in RS:
                for name, lab in matrices(L, R, P, ign, rng):
                    n = (lab != ign).sum(1)
                    for cap in _capacities(lab, ign, P):
                        check_flat(lab, cap, ign, 'L {} R {} cap {} ign {} {}'.format(
                            L, R, cap, ign, name))
                        before = np.concatenate([[0], np.cumsum(n)])
                        cut += bool(((before[:-1] < cap) & (cap < before[1:])).any())
                    empty += int(n.sum()) == 0
    assert empty > 0 and (cut > 0 or L == 1)  # total 0; capacity hit in the middle of a row


@pytest.mark.parametrize('R', [257, 1025])
def test_many_rows(R):
    """Row offsets across blocks and across the 256-row tiles of the count sum; a capacity that
    ends in a late row."""
    rng = np.random.default_rng(R)
    lab = np.where(rng.random((R, 8)) < 0.3, rng.integers(0, 30522, (R, 8)), -1).astype(np.int64)
    lab[R // 2] = -1
    lab[R - 1] = 5
    total = int((lab != -1).sum())
    check_rows(lab, 3, -1, 'R {}'.format(R))
    for cap in (total - 3, total, total + 700, R * 3):
        check_flat(lab, cap, -1, 'R {} cap {}'.format(R, cap))


def test_no_rows_and_no_slots():
    """R == 0: the rows form launches nothing, the flat form still pads and writes total 0.
    L == 0: rows without a masked slot."""
    for R, L in ((0, 8), (0, 0), (3, 0), (5, 0)):
        lab = np.zeros((R, L), np.int64)
        check_rows(lab, 4, -1, 'R {} L {}'.format(R, L))
        for cap in (1, 300, 70000):
            check_flat(lab, cap, -100, 'R {} L {} cap {}'.format(R, L, cap))


# ---- the Python path --------------------------------------------------------------------------
@pytest.fixture
def sentinel_empty(monkeypatch):
    """torch.empty that fills what it returns: compact_labels may rely on no initial value."""
    real = torch.empty

    def empty(*a, **k):
        t = real(*a, **k)
        return t.fill_(SENT[t.dtype]) if t.dtype in SENT else t
    monkeypatch.setattr(torch, 'empty', empty)


def assert_python(lab_t, P, ign):
    from lddl_amd.torch import compact_labels
    lab = lab_t.cpu().numpy()
    R = lab.shape[0]
    got = compact_labels(lab_t, P, ign)
    assert list(got) == ['masked_lm_positions', 'masked_lm_ids', 'masked_lm_weights', 'num_masked']
    exp = ref_rows(lab, P, ign)
    for (k, g), e in zip(got.items(), exp):
        assert g.is_cuda and g.is_contiguous() and g.shape == e.shape, k
        assert g.dtype == torch.from_numpy(e).dtype, k
        np.testing.assert_array_equal(g.cpu().numpy(), e, err_msg=k)
    got = compact_labels(lab_t, P, ign, layout='flat')
    assert list(got) == ['masked_lm_flat_positions', 'masked_lm_flat_ids', 'num_masked',
                         'num_masked_total']
    exp = ref_flat(lab, R * P, ign)
    for (k, g), e in zip(got.items(), exp):
        assert g.is_cuda and g.shape == e.shape and g.dtype == torch.from_numpy(e).dtype, k
        np.testing.assert_array_equal(g.cpu().numpy(), e, err_msg=k)


def _labels(R, L, ign, seed, p=0.15):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((R, L)) < p, rng.integers(0, 30522, (R, L)), ign).astype(np.int64)


def test_python_path_and_default_ignore_index(sentinel_empty):
    from lddl_amd.torch import compact_labels
    lab = torch.from_numpy(_labels(9, 129, -1, 5)).cuda()
    assert_python(lab, 20, -1)
    assert_python(torch.from_numpy(_labels(5, 65, -100, 6, p=0.5)).cuda(), 20, -100)  # overflows
    a, b = compact_labels(lab, 20), compact_labels(lab, 20, -1, 'rows')
    assert all(torch.equal(a[k], b[k]) for k in a)
    for bad in (lab.int(), lab.cpu(), lab[0], lab.cpu().numpy()):
        with pytest.raises(ValueError, match='cuda int64'):
            compact_labels(bad, 20)
    empty = compact_labels(lab[:0], 4, layout='flat')
    assert empty['masked_lm_flat_positions'].shape == (0,)
    assert empty['num_masked_total'].tolist() == [0]
    assert compact_labels(lab[:0], 4)['masked_lm_positions'].shape == (0, 4)


def test_non_contiguous_labels(sentinel_empty):
    big = torch.from_numpy(_labels(10, 140, -1, 7)).cuda()
    for view in (big[:, 3:132], big[::2], big[1:8:3, 5:70:2], big.t()[:64]):
        assert not view.is_contiguous()
        assert_python(view, 20, -1)


def test_non_default_stream(sentinel_empty):
    lab = torch.from_numpy(_labels(9, 512, -1, 8)).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        assert_python(lab, 128, -1)
    s.synchronize()


def test_no_host_wait_inside_a_captured_graph():
    """Neither form allocates outside torch's pool, copies to the host or synchronises: both
    capture into a graph, and the replay compacts the labels that are in the buffer then."""
    from lddl_amd.torch import compact_labels
    static = torch.from_numpy(_labels(9, 129, -1, 9)).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm up outside the capture
        compact_labels(static, 20)
        compact_labels(static, 20, layout='flat')
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rows = compact_labels(static, 20)
        flat = compact_labels(static, 20, layout='flat')
    new = _labels(9, 129, -1, 10, p=0.2)
    static.copy_(torch.from_numpy(new))
    g.replay()
    torch.cuda.synchronize()
    for g_, e in zip(rows.values(), ref_rows(new, 20, -1)):
        np.testing.assert_array_equal(g_.cpu().numpy(), e)
    for g_, e in zip(flat.values(), ref_flat(new, 9 * 20, -1)):
        np.testing.assert_array_equal(g_.cpu().numpy(), e)


# ---- refusals ---------------------------------------------------------------------------------
def test_abi_refusals():
    """-1 with a message and nothing launched. The entry points take a stream and no context, so
    these calls share no state with anything else."""
    from lddl_amd._native import lib
    lab = torch.from_numpy(_labels(4, 16, -1, 11, p=0.5)).cuda()
    o = [_full(64, torch.int64), _full(64, torch.int64), _full(64, torch.float32),
         _full(4, torch.int32), _full(1, torch.int64)]
    p = [ctypes.c_void_p(t.data_ptr()) for t in o]
    lp = ctypes.c_void_p(lab.data_ptr())
    st = _stream()

    def rows(lab_p=lp, R=4, L=16, P=16, out=None):
        return lib.lddl_mlm_compact_rows(st, lab_p, R, L, -1, P, *(out or p[:4]))

    def flat(lab_p=lp, R=4, L=16, cap=64, out=None):
        return lib.lddl_mlm_compact_flat(st, lab_p, R, L, -1, cap,
                                         *(out or (p[0], p[1], p[3], p[4])))
    for k in range(4):  # each output in turn, then the labels
        assert rows(out=p[:k] + [None] + p[k + 1:4]) == -1
        assert b'null pointer' in lib.lddl_last_error()
        f = [p[0], p[1], p[3], p[4]]
        assert flat(out=f[:k] + [None] + f[k + 1:]) == -1
        assert b'null pointer' in lib.lddl_last_error()
    assert rows(lab_p=None) == -1 and b'null pointer' in lib.lddl_last_error()
    assert flat(lab_p=None) == -1 and b'null pointer' in lib.lddl_last_error()
    for bad in (0, -1):
        assert rows(P=bad) == -1 and b'P' in lib.lddl_last_error()
        assert flat(cap=bad) == -1 and b'capacity' in lib.lddl_last_error()
    assert rows(R=-1) == -1 and b'negative' in lib.lddl_last_error()
    assert flat(R=-1) == -1 and b'negative' in lib.lddl_last_error()
    assert rows(L=-1) == -1 and b'negative' in lib.lddl_last_error()
    assert flat(L=-1) == -1 and b'negative' in lib.lddl_last_error()
    assert rows(L=1 << 31, R=0) == -1 and b'2^31' in lib.lddl_last_error()
    assert flat(L=1 << 31, R=0) == -1 and b'2^31' in lib.lddl_last_error()
    torch.cuda.synchronize()
    for t in o:  # nothing was launched
        assert int((t != SENT[t.dtype]).sum()) == 0
    assert rows() == 0 and flat() == 0  # and the same buffers are accepted
    torch.cuda.synchronize()
