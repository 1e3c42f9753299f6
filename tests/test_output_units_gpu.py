"""The output stage's kernels one by one at their edge shapes: per-partition and single-segment
binning (csrc/output_bin.hip) against numpy's stable argsort / bincount, and the string / npy
rendering (csrc/output_render.hip) of hand-built pair tables, every row against Python's
' '.join and np.save, with 2-byte and 4-byte token ids."""
import io

import numpy as np
import pytest
import torch

from conftest import VOCAB_UNCASED
from render_util import py_rows

pytestmark = pytest.mark.gpu

MAX_BINS = 8192  # kMaxBinsLds


@pytest.fixture(scope='module')
def ctx():
    from lddl_amd.context import Context
    return Context(VOCAB_UNCASED, True)


@pytest.fixture(scope='module')
def wide_ctx(tmp_path_factory):
    """A vocab of more than 65,536 lines: 4-byte ids in the pair tables and the render."""
    from lddl_amd.context import Context
    with open(VOCAB_UNCASED, encoding='utf-8') as f:
        lines = f.read().splitlines()
    big = tmp_path_factory.mktemp('vocab') / 'vocab_big.txt'
    big.write_text('\n'.join(lines + ['[extra{}]'.format(i) for i in range(40000)]) + '\n',
                   encoding='utf-8')
    c = Context(str(big), True)
    assert c.id_bytes == 4
    return c


# ---- binning ----------------------------------------------------------------------------------
def _np_bins(nt, bin_size, nbins):
    """(bin of every row, stable order by bin, rows per bin) as _to_dataframe_binned."""
    b = np.minimum((nt.astype(np.int64) - 1) // bin_size, nbins - 1)
    return b, np.argsort(b, kind='stable'), np.bincount(b, minlength=nbins).astype(np.int64)


def _tok_off(nt):
    """Token offsets of a pair table whose rows have num_tokens nt (len(A) + len(B) + 3)."""
    return np.concatenate([[0], np.cumsum(nt.astype(np.int64) - 3)]).astype(np.int64)


def _check_partitions(ctx, nt, off, bin_size, nbins):
    from lddl_amd.output import bin_partitions
    d_off = torch.from_numpy(off).cuda()
    by_nt = bin_partitions(ctx, torch.from_numpy(nt).cuda(), d_off, bin_size, nbins)
    by_off = bin_partitions(ctx, None, d_off, bin_size, nbins,
                            tok_off=torch.from_numpy(_tok_off(nt)).cuda())
    for perm, bin_id, counts in (by_nt, by_off):
        perm, bin_id, counts = perm.cpu().numpy(), bin_id.cpu().numpy(), counts.cpu().numpy()
        assert perm.shape == bin_id.shape == nt.shape and counts.shape == (len(off) - 1, nbins)
        for p in range(len(off) - 1):
            a, z = off[p], off[p + 1]
            eb, eo, ec = _np_bins(nt[a:z], bin_size, nbins)
            assert np.array_equal(perm[a:z] - a, eo), p
            assert np.array_equal(bin_id[a:z], eb[eo]), p
            assert np.array_equal(counts[p], ec), p


BIN_SHAPES = [(1, 8), (3, 40), (5, 100), (100, 5), (MAX_BINS, 1)]
PART_SIZES = [0, 1, 63, 64, 65, 0, 256, 257, 1000, 0]


@pytest.mark.parametrize('nbins,bin_size', BIN_SHAPES)
def test_bin_partitions_edge_shapes(ctx, nbins, bin_size):
    rng = np.random.default_rng(nbins)
    off = np.concatenate([[0], np.cumsum(PART_SIZES)]).astype(np.int64)
    nt = rng.integers(5, nbins * bin_size + 51, off[-1]).astype(np.int32)
    assert nt.max() > nbins * bin_size  # the clamp to the last bin
    _check_partitions(ctx, nt, off, bin_size, nbins)


@pytest.mark.parametrize('nbins,bin_size,lo,hi', [(5, 100, 201, 300), (3, 40, 81, 500),
                                                  (100, 5, 5, 5), (MAX_BINS, 1, 9000, 9000)])
def test_bin_partitions_all_rows_in_one_bin(ctx, nbins, bin_size, lo, hi):
    """300 rows of one bin: every rank past the first 64 rows comes from the running counter."""
    rng = np.random.default_rng(lo)
    nt = rng.integers(lo, hi + 1, 300).astype(np.int32)
    assert len(set(_np_bins(nt, bin_size, nbins)[0])) == 1
    _check_partitions(ctx, nt, np.asarray([0, 300], np.int64), bin_size, nbins)
    # the same rows between two other partitions
    nt3 = np.concatenate([np.full(70, 5, np.int32), nt, np.full(3, 5, np.int32)])
    _check_partitions(ctx, nt3, np.asarray([0, 70, 370, 373], np.int64), bin_size, nbins)


def test_bin_limits(ctx):
    from lddl_amd._native import NativeError
    from lddl_amd.output import bin_partitions, bin_stable
    nt = torch.full((10,), 7, dtype=torch.int32).cuda()
    off = torch.tensor([0, 10], dtype=torch.int64).cuda()
    for call in (lambda: bin_partitions(ctx, nt, off, 1, MAX_BINS + 1),
                 lambda: bin_stable(ctx, nt, 1, MAX_BINS + 1)):
        with pytest.raises(NativeError, match='nbins {} > {} unsupported'.format(MAX_BINS + 1,
                                                                                 MAX_BINS)):
            call()
    # no partitions: empty outputs
    for kw in (dict(num_tokens=torch.zeros(0, dtype=torch.int32).cuda()),
               dict(num_tokens=None, tok_off=torch.zeros(1, dtype=torch.int64).cuda())):
        perm, bin_id, counts = bin_partitions(ctx, part_off=torch.zeros(1, dtype=torch.int64).cuda(),
                                              bin_size=8, nbins=16, **kw)
        assert perm.numel() == 0 and bin_id.numel() == 0 and tuple(counts.shape) == (0, 16)
        assert perm.dtype == bin_id.dtype == counts.dtype == torch.int64


@pytest.mark.parametrize('nbins,bin_size', [(1, 8), (3, 40), (64, 8), (MAX_BINS, 1)])
def test_bin_stable_edge_shapes(ctx, nbins, bin_size):
    """One and two tiles of 2048 rows and their edges; with and without the bin_id output; rows
    given as num_tokens and as token offsets."""
    from lddl_amd.output import bin_stable
    rng = np.random.default_rng(nbins + 1)
    for n in (0, 1, 64, 65, 2047, 2048, 2049, 4097):
        nt = rng.integers(5, nbins * bin_size + 51, n).astype(np.int32)
        eb, eo, ec = _np_bins(nt, bin_size, nbins)
        for with_bin_id in (True, False):
            for kw in (dict(num_tokens=torch.from_numpy(nt).cuda()),
                       dict(tok_off=torch.from_numpy(_tok_off(nt)).cuda())):
                perm, bin_id, counts = bin_stable(ctx, bin_size=bin_size, nbins=nbins,
                                                  with_bin_id=with_bin_id, **kw)
                what = (n, with_bin_id, sorted(kw))
                assert np.array_equal(perm.cpu().numpy(), eo), what
                assert np.array_equal(counts.cpu().numpy(), ec), what
                if with_bin_id:
                    assert np.array_equal(bin_id.cpu().numpy(), eb[eo]), what
                else:
                    assert bin_id is None


# ---- rendering --------------------------------------------------------------------------------
LENS_A = (1, 63, 64, 65, 128, 129, 509)
LENS_B = (1, 64, 65, 300)
MASK_COUNTS = (0, 1, 9, 10, 63, 64, 65, 99, 100, 999)


def _npy_reference_layout_ok():
    """np.save writes a 128-byte header for these arrays on this numpy (what put_npy restates);
    otherwise the comparison below would fail in the reference, not in the kernel."""
    for k in (0, 999):
        buf = io.BytesIO()
        np.save(buf, np.arange(k, dtype=np.uint16))
        b = buf.getvalue()
        assert len(b) == 128 + 2 * k, (k, len(b))
        assert b[:6] == b'\x93NUMPY' and b[127:128] == b'\n'


def _special_ids(vocab):
    """Ids the render table's edges hang on: the first and last id, the longest string, a
    one-byte string, a ## piece, a multi-byte UTF-8 string (and, wide vocab, ids > 65,535)."""
    nbytes = [len(t.encode('utf-8')) for t in vocab]
    ids = [0, len(vocab) - 1, int(np.argmax(nbytes)), nbytes.index(1),
           next(i for i, t in enumerate(vocab) if t.startswith('##')),
           next(i for i, t in enumerate(vocab) if len(t.encode('utf-8')) > len(t))]
    if len(vocab) > 65536:
        ids += [65535, 65536, 65537]
    return ids


def _synthetic_table(c, masking, seed):
    """(host dict as PairBatch.to_host(), PairBatch on the device): one row per (len A, len B)
    of LENS_A x LENS_B, mask counts cycling over MASK_COUNTS."""
    from lddl_amd.pairs import PairBatch
    rng = np.random.default_rng(seed)
    V = len(c.tokens)
    special = _special_ids(c.tokens)
    np_id = np.uint16 if c.id_bytes == 2 else np.int32

    def draw(n):
        ids = rng.integers(0, V, n)
        pick = rng.random(n) < 0.3
        ids[pick] = rng.choice(special, int(pick.sum()))
        return ids

    shapes = [(a, b) for a in LENS_A for b in LENS_B]
    n = len(shapes)
    ntok = np.asarray([a + b for a, b in shapes], np.int64)
    h = {'tok_off': np.concatenate([[0], np.cumsum(ntok)]).astype(np.int64),
         'len_a': np.asarray([a for a, _ in shapes], np.int32),
         'is_random_next': rng.integers(0, 2, n).astype(bool)}
    tokens = draw(int(ntok.sum()))
    big = int(h['tok_off'][shapes.index((509, 300))])
    tokens[big:big + len(special)] = special          # in A of the longest row ...
    tokens[big + 509:big + 509 + len(special)] = special[::-1]  # ... and in its B
    h['tokens'] = tokens.astype(np_id)
    if masking:
        nm = np.asarray([MASK_COUNTS[i % len(MASK_COUNTS)] for i in range(n)], np.int64)
        h['pos_off'] = np.concatenate([[0], np.cumsum(nm)]).astype(np.int64)
        h['pos'] = np.concatenate([np.sort(rng.choice(60000, k, replace=False)) for k in nm]
                                  ).astype(np.uint16)
        assert (h['pos'] > 255).any() and (h['pos'] < 256).any()
        labels = draw(int(nm.sum()))
        long_row = int(h['pos_off'][list(nm).index(999)])
        labels[long_row:long_row + len(special)] = special
        h['labels'] = labels.astype(np_id)
    for k in ('tokens', 'labels'):
        if k in h:
            assert set(special) <= set(h[k].astype(np.int64).tolist())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    ids = lambda a: t(a.view(np.int16) if c.id_bytes == 2 else a)  # noqa: E731
    pb = PairBatch(ids(h['tokens']), t(h['tok_off']), t(h['len_a']),
                   t(h['is_random_next'].astype(np.uint8)))
    assert pb.tokens.dtype == c.id_dtype
    if masking:
        pb.pos, pb.labels, pb.pos_off = t(h['pos'].view(np.int16)), ids(h['labels']), t(h['pos_off'])
        pb.n_masked = int(h['pos_off'][-1])
    return h, pb


def _row_sets(n, rng):
    """rows arguments of render: None (all rows in order), a permutation, a subset with
    duplicates, and 0 / 1 / 3 / 4 / 5 rows (four rows per workgroup)."""
    perm = rng.permutation(n).astype(np.int64)
    dup = rng.integers(0, n, 11).astype(np.int64)
    dup[3] = dup[7] = dup[0]
    return [None, perm, dup] + [rng.permutation(n)[:k].astype(np.int64) for k in (0, 1, 3, 4, 5)] \
        + [np.asarray([n - 1] * 5, np.int64)]


def _lens_to_off(strings):
    return np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.int64)


@pytest.mark.parametrize('wide', [False, True])
@pytest.mark.parametrize('masking', [True, False])
def test_render_synthetic_rows(ctx, wide_ctx, wide, masking):
    from lddl_amd.output import render
    _npy_reference_layout_ok()
    c = wide_ctx if wide else ctx
    h, pb = _synthetic_table(c, masking, seed=2 * wide + masking)
    rng = np.random.default_rng(5)
    for rows in _row_sets(pb.n_pairs, rng):
        exp = py_rows(h, c.tokens, rows)
        rd = render(c, pb, None if rows is None else torch.from_numpy(rows).cuda())
        assert rd.n == len(exp)
        for r in range(len(exp)):
            assert rd.row(r) == exp[r], (None if rows is None else rows.tolist(), r)
        enc = lambda k: [e[k].encode('utf-8') for e in exp]  # noqa: E731
        assert np.array_equal(rd.a_off, _lens_to_off(enc('A')))
        assert np.array_equal(rd.b_off, _lens_to_off(enc('B')))
        assert len(rd.a_bytes) == rd.a_off[-1] and len(rd.b_bytes) == rd.b_off[-1]
        if masking:
            assert np.array_equal(rd.l_off, _lens_to_off(enc('masked_lm_labels')))
            assert np.array_equal(rd.npy_off,
                                  _lens_to_off([e['masked_lm_positions'] for e in exp]))
            assert len(rd.l_bytes) == rd.l_off[-1] and len(rd.npy_bytes) == rd.npy_off[-1]
        else:
            assert rd.l_off is None and rd.npy_off is None


def test_render_rejects_other_id_width(ctx, wide_ctx):
    """A 2-byte pair table is not rendered by the 4-byte context (and the other way round)."""
    from lddl_amd.output import render
    for c, other in ((ctx, wide_ctx), (wide_ctx, ctx)):
        _, pb = _synthetic_table(other, False, seed=9)
        with pytest.raises(ValueError, match='byte ids'):
            render(c, pb)
