"""lddl_utf8_check (csrc/utf8.hip) against Python's strict UTF-8 decoder: the first offset the
decoder rejects (UnicodeDecodeError.start), on valid text, every malformed-sequence class and a
seeded fuzz; buffers of several workgroups with sequences split over every slice and workgroup
edge; and the CLI raising on malformed input as dask's read_text does."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _py_first_bad(b):
    try:
        b.decode('utf-8')
        return -1
    except UnicodeDecodeError as e:
        return e.start


def _gpu_first_bad(b):
    from lddl_amd.punkt import utf8_first_invalid
    t = torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda() if b else torch.zeros(
        0, dtype=torch.uint8, device='cuda')
    return utf8_first_invalid(t)


CASES = [b'', b'plain ascii', 'naïve café 漢字 \U0001F600 　'.encode(),
         b'\x80', b'a\xbf', b'\xc0\x80', b'\xc1\xbf', b'\xc2', b'\xc2\x41', b'\xe0\x80\x80',
         b'\xe0\x9f\xbf', b'\xed\xa0\x80', b'\xed\x9f\xbf', b'\xef\xbf', b'\xf0\x8f\xbf\xbf',
         b'\xf4\x90\x80\x80', b'\xf5\x80\x80\x80', b'\xff', b'abc\xe2\x82', b'\xe2\x82\xac\x80',
         b'\xf0\x9f\x98\x80\x80\x80\x80\x80', b'x' * 15 + b'\xe2\x82\xac' + b'y' * 30 + b'\x9f']


@pytest.mark.parametrize('i', range(len(CASES)))
def test_utf8_cases(i):
    b = CASES[i]
    assert _gpu_first_bad(b) == _py_first_bad(b)


def test_utf8_fuzz():
    rng = np.random.default_rng(7)
    good = 'the quick éè 中文 \U0001F680 brown'.encode()
    for _ in range(300):
        parts = []
        for _ in range(rng.integers(1, 40)):
            r = rng.random()
            if r < 0.7:
                parts.append(good[:rng.integers(0, len(good))])
            else:
                parts.append(bytes(rng.integers(0x7e, 0x100, rng.integers(1, 5)).astype(np.uint8)))
        b = b''.join(parts)
        assert _gpu_first_bad(b) == _py_first_bad(b), b


# ---- buffers of more than one workgroup (4096 bytes each: 256 threads x 16-byte slices) --------
BLOCK, SLICE = 4096, 16
UNIT = 'aé漢\U0001F600b'.encode()  # 1 + 2 + 3 + 4 + 1 = 11 bytes: coprime with 16
SIZES = {k: [BLOCK * k + d for d in (-1, 0, 1, 17)] for k in (1, 2, 257)}


def _valid(n, phase):
    """n bytes of valid text: `phase` ASCII bytes, then UNIT repeated, cut at a character
    boundary and padded with ASCII."""
    body = (UNIT * ((n - phase) // len(UNIT) + 1))[:n - phase]
    while body and (body[-1] & 0xC0) == 0x80:
        body = body[:-1]
    if body and body[-1] >= 0xC0:
        body = body[:-1]
    b = b'x' * phase + body
    b += b'y' * (n - len(b))
    assert len(b) == n and _py_first_bad(b) == -1
    return b


def _splits(b, edge):
    """{(bytes before, bytes after)} of the multi-byte sequences of valid `b` that straddle a
    multiple of `edge`."""
    a = np.frombuffer(b, np.uint8)
    out = set()
    for e in range(edge, len(a), edge):
        if (a[e] & 0xC0) != 0x80:
            continue
        s = e - 1
        while (a[s] & 0xC0) == 0x80:
            s -= 1
        ln = 2 if a[s] < 0xE0 else 3 if a[s] < 0xF0 else 4
        out.add((e - s, s + ln - e))
    return out


ALL_SPLITS = {(1, 1), (1, 2), (2, 1), (1, 3), (2, 2), (3, 1)}


class _DeviceText:
    """A buffer on the device that single bytes are planted into and restored from."""

    def __init__(self, b):
        self.host = bytearray(b)
        self.dev = torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()

    def first_bad(self, plants=()):
        from lddl_amd.punkt import utf8_first_invalid
        saved = [(p, self.host[p]) for p, _ in plants]
        for p, v in plants:
            self.host[p] = v
            self.dev[p] = v
        try:
            return utf8_first_invalid(self.dev), _py_first_bad(bytes(self.host))
        finally:
            for p, v in reversed(saved):
                self.host[p] = v
                self.dev[p] = v


@pytest.mark.parametrize('k', sorted(SIZES))
def test_utf8_valid_and_one_bad_byte_across_workgroups(k):
    """Valid text of 4096 k + d bytes in every phase, then one 0xFF or one stray 0x80 planted at
    the buffer's, a slice's and a workgroup's first and last bytes."""
    slice_splits, block_splits = set(), set()
    for n in SIZES[k]:
        for phase in range(4):
            b = _valid(n, phase)
            slice_splits |= _splits(b, SLICE)
            block_splits |= _splits(b, BLOCK)
            t = _DeviceText(b)
            assert t.first_bad() == (-1, -1), (n, phase)
            for bad in (0xFF, 0x80):
                for p in (0, 15, 16, 17, BLOCK - 1, BLOCK, BLOCK + 1, n - 1):
                    if p >= n:
                        continue
                    got, exp = t.first_bad([(p, bad)])
                    # (0x80 over a continuation byte can leave the text well-formed: exp == -1)
                    assert bad == 0x80 or 0 <= exp <= p
                    assert got == exp, (n, phase, hex(bad), p)
    assert slice_splits == ALL_SPLITS
    if k == 257:  # 256 workgroup edges: every split of every sequence length
        assert block_splits == ALL_SPLITS
    elif k == 2:
        assert block_splits


@pytest.mark.parametrize('k', [2, 257])
def test_utf8_two_bad_bytes_in_different_workgroups(k):
    """Each workgroup reports its own first bad offset: the lowest must win."""
    rng = np.random.default_rng(k)
    for n in SIZES[k]:
        t = _DeviceText(_valid(n, n % 4))
        n_blocks = (n + BLOCK - 1) // BLOCK
        for _ in range(6):
            b0, b1 = sorted(rng.choice(n_blocks, 2, replace=False))
            p0 = int(b0 * BLOCK + rng.integers(0, BLOCK))
            p1 = int(min(n - 1, b1 * BLOCK + rng.integers(0, BLOCK)))
            for ff, stray in ((p0, p1), (p1, p0)):
                got, exp = t.first_bad([(ff, 0xFF), (stray, 0x80)])
                assert 0 <= exp <= ff  # (the 0x80 may land on a continuation byte and be valid)
                assert got == exp, (n, ff, stray)
            got, exp = t.first_bad([(p0, 0xFF), (p1, 0xFF)])
            assert 0 <= exp <= p0 and got == exp, (n, p0, p1)


@pytest.mark.parametrize('k', [2, 257])
def test_utf8_truncated_tail_of_a_large_buffer(k):
    """A 2-, 3- or 4-byte sequence cut short by the end of a buffer of several workgroups."""
    seqs = ['é'.encode(), '漢'.encode(), '\U0001F600'.encode()]
    for n in SIZES[k]:
        for s in seqs:
            for keep in range(1, len(s)):
                b = _valid(n - keep, 1) + s[:keep]
                assert _py_first_bad(b) == n - keep
                assert _gpu_first_bad(b) == n - keep, (n, s, keep)
            b = _valid(n - len(s), 1) + s  # the whole sequence in the buffer's last bytes is fine
            assert _gpu_first_bad(b) == _py_first_bad(b) == -1


def test_utf8_four_byte_sequence_three_bytes_before_a_slice_edge():
    """F0 9F 98 | 80: the slice that starts on the last byte looks back three bytes for its lead.
    With that byte replaced by ASCII the lead (in the earlier slice) is the bad offset."""
    s = '\U0001F600'.encode()
    for edge in (SLICE, 5 * SLICE, BLOCK, BLOCK + SLICE, 2 * BLOCK):
        for tail in (b'z', 'é'.encode(), b''):
            b = b'q' * (edge - 3) + s + tail
            assert _py_first_bad(b) == -1
            assert _gpu_first_bad(b) == -1, (edge, tail)
            b = b'q' * (edge - 3) + s[:3] + b'A' + tail
            assert _py_first_bad(b) == edge - 3
            assert _gpu_first_bad(b) == edge - 3, (edge, tail)
            # three continuation bytes before the edge and no lead: the first of them is bad
            b = b'q' * (edge - 3) + b'\x9f\x98\x80\x80' + tail
            assert _gpu_first_bad(b) == _py_first_bad(b) == edge - 3


def test_cli_rejects_malformed_utf8(tmp_path):
    from conftest import VOCAB_UNCASED
    from lddl_amd.dask.bert import pretrain as P
    src = tmp_path / 'source' / 'en'
    src.mkdir(parents=True)
    (src / 'w.txt').write_bytes(b'wiki-1 good text here.\nwiki-2 bad \xff byte.\n')
    args = P.attach_args().parse_args(['--schedule', 'local', '--wikipedia', str(tmp_path / 'source'),
                                       '--sink', str(tmp_path / 'out'), '--vocab-file',
                                       VOCAB_UNCASED, '--sample-ratio', '1.0'])
    with pytest.raises(UnicodeDecodeError):
        P.main(args)
