"""The streaming tokenizer's non-ASCII ("slow") units against the oracle on a crafted corpus.

Units of <= 32 raw bytes with at most four non-ASCII code points are normalised from registers
(tokenize_dev.h, norm_regs); the others, and every one with LDDL_TOKENIZE_SLOW=loop, byte by byte
from the text. The corpus below holds every shape either path treats differently, counted on the
CPU before the GPU sees it, and runs with the knob in both positions through the plain kernel,
both memo instantiations, a one-workgroup grid and a small max_pieces.

Growing mappings (looked up in the committed tables, lddl_amd/assets/bert_norm_*.bin): the uncased
table maps 11,214 code points to more than one char (kMulti, all longer than their source, e.g.
a Hangul syllable of 3 bytes to 6 or 9 bytes of jamo) and 9 to a single longer one (U+023A, 2
bytes, to U+2C65, 3 bytes), so a unit of <= 32 raw bytes can pass 32 normalised bytes and the
corpus has such units; the cased table has no growing mapping, where the same units stay short.
"""
import numpy as np
import pytest

from conftest import VOCAB_CASED, VOCAB_UNCASED

pytestmark = pytest.mark.gpu

ASCII = b'internationalizationstrommethcounterrevolutionary'
CH2 = ['é'.encode(), 'β'.encode()]                 # accent stripped / kept (uncased)
CH3 = ['ḁ'.encode(), 'ก'.encode()]                 # U+1E01 (NFD: a + mark), Thai ko kai
CH4 = ['\U00010400'.encode(), '\U0001d400'.encode()]  # Deseret capital (lowercases), math bold A
HANGUL = '한'.encode()                             # kMulti (uncased): 3 bytes -> 9
A_STROKE = 'Ⱥ'.encode()                            # uncased: 2 bytes -> 3
DROPPED = ['\u00ad'.encode(), '\u200b'.encode(), b'\x01', b'\x7f', b'\x00']
HARD_ASCII = b'qzxqzxq'                            # in neither vocab (asserted): a hard unit
kChunk = 128                                       # the kernel claims sentences in chunks of 128


def _units():
    """(class, unit bytes) in a fixed order. No unit holds a separator."""
    out = []
    # every raw length 1..34, a 2- / 3- / 4-byte character at every position
    for L in range(1, 35):
        for w, chars in ((2, CH2), (3, CH3), (4, CH4)):
            for p in range(0, L - w + 1):
                ch = chars[(L + p) % 2]
                out.append(('len%d' % w, ASCII[:p] + ch + ASCII[p:L - w]))
    # invalid UTF-8 at every position of units of 1..34 bytes
    for L in range(1, 35):
        for p in range(L):
            out.append(('lone_cont', ASCII[:p] + b'\x80' + ASCII[p:L - 1]))
            out.append(('ff', ASCII[:p] + b'\xff' + ASCII[p:L - 1]))
        for lead in (b'\xc3', b'\xe2\x82', b'\xf0\x9f\x98', b'\xe2', b'\xf0'):
            if len(lead) <= L:
                # cut by the unit's end (a separator follows the unit)
                out.append(('lead_cut', ASCII[:L - len(lead)] + lead))
            for p in range(0, L - len(lead)):
                # followed by a byte that is no continuation
                out.append(('lead_bad', ASCII[:p] + lead + ASCII[p:L - len(lead)]))
    # dropped characters: alone, in runs, inside words
    for d in DROPPED:
        for n in (1, 2, 5, 10):
            if len(d) * n <= 34:
                out.append(('drop_only', d * n))
    out.append(('drop_only', b''.join(DROPPED)))
    for L in range(2, 33):
        for k, d in enumerate(DROPPED):
            p = (L * 7 + k) % (L - 1) + 1
            out.append(('drop_mixed', ASCII[:p] + d + ASCII[p:L] + CH2[k % 2]))
            out.append(('drop_mixed', d + ASCII[:L]))
    # the 32-byte boundary: multi-char mappings (<= 4 non-ASCII code points: the register path;
    # more: the loop), normalised lengths around 32 and past it
    for n in range(1, 8):
        for k in range(0, 33 - 3 * n):
            out.append(('multi', ASCII[:k // 2] + HANGUL * n + ASCII[:k - k // 2]))
    for n in range(1, 17):
        for k in (0, 1, 2, 32 - 2 * n):
            if k >= 0:
                out.append(('grow1', A_STROKE * n + ASCII[:k]))
    return out


def _pad(n):
    """n bytes of short ASCII words that end with a separator."""
    return (b'abcd ' * 20)[:n - 1] + b' ' if n else b''


def _corpus():
    units = _units()
    sents = []
    # ten units per sentence, plain words between
    for i in range(0, len(units), 10):
        parts = []
        for c, u in units[i:i + 10]:
            parts += [u, b'the']
        sents.append(b' '.join(parts))
    counts = {}
    for c, _ in units:
        counts[c] = counts.get(c, 0) + 1
    # bank and chunk boundaries: one unit of every class behind 0..70 bytes of ASCII
    reps = {}
    for c, u in units:
        if len(u) >= 9:
            reps.setdefault(c, u)
    pad_first = len(sents)
    for c, u in sorted(reps.items()):
        for n in range(71):
            sents.append(_pad(n) + u + b' end')
    counts['padded'] = len(sents) - pad_first
    # more than 64 hard units in one flush (the first 192 units of a chunk): each sentence starts
    # a chunk; slow units at hard index 63 and 64, and a run of them past 64
    slow = [CH2[0] + b'cole', b'caf' + CH2[0], CH3[0] + b'b', HANGUL + b'x', b'na\xc3', CH4[0],
            b'\x80abc', A_STROKE * 3]
    over = []
    for n_before in (62, 63, 64, 65, 100):
        parts = [HARD_ASCII] * n_before
        parts += [slow[(n_before + k) % len(slow)] for k in range(40)]
        parts += [b'the'] * 120 + [slow[0]] * 3
        over.append(b' '.join(parts))
    over.append(b' '.join(slow[k % len(slow)] for k in range(190)))
    over_at = []
    for s in over:
        while len(sents) % kChunk:
            sents.append(b'the end')
        over_at.append(len(sents))
        sents.append(s)
    counts['over64'] = len(over)
    text = np.frombuffer(b''.join(sents), np.uint8).copy()
    off = np.zeros(len(sents) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in sents])
    return text, off, counts, (pad_first, pad_first + counts['padded']), over_at


@pytest.fixture(scope='module')
def corpus():
    return _corpus()


@pytest.fixture(scope='module')
def ctxs():
    from lddl_amd.context import Context
    return {'uncased': Context(VOCAB_UNCASED, True), 'cased': Context(VOCAB_CASED, False)}


@pytest.fixture(scope='module')
def expected(corpus):
    """The oracle's output per (case, max_pieces), computed once."""
    from oracle import oracle as O
    text, off = corpus[0], corpus[1]
    out = {}
    for case, vocab in (('uncased', VOCAB_UNCASED), ('cased', VOCAB_CASED)):
        tok = O.Tokenizer(vocab, lowercase=case == 'uncased')
        for mp in (512, 9):
            out[case, mp] = tok.tokenize(text, off, max_pieces=mp)
        with open(vocab, 'rb') as f:
            assert HARD_ASCII not in f.read().split(), 'HARD_ASCII must not be a vocab word'
    return out


def test_corpus_holds_every_class(corpus):
    """Counted on the CPU: a generator change cannot empty the test unnoticed."""
    text, off, counts, (p0, p1), over_at = corpus
    assert text.size <= 2 << 20
    floor = {'len2': 500, 'len3': 500, 'len4': 450, 'lone_cont': 500, 'ff': 500, 'lead_cut': 150,
             'lead_bad': 2000, 'drop_only': 15, 'drop_mixed': 300, 'multi': 100, 'grow1': 40,
             'padded': 71 * 10, 'over64': 6}
    for c, n in floor.items():
        assert counts.get(c, 0) >= n, (c, counts.get(c, 0))
    # the padded units start at every offset of a 64-byte bank of their chunk, and some straddle
    starts, straddle = set(), 0
    for s in range(p0, p1):
        base = off[(s // kChunk) * kChunk]
        sent = bytes(text[off[s]:off[s + 1]])
        u0 = sent.rfind(b' ', 0, len(sent) - 4) + 1  # the unit before ' end'
        a = int(off[s] - base) + u0
        b = int(off[s] - base) + len(sent) - 5
        starts.add(a % 64)
        straddle += a // 64 != b // 64
    assert len(starts) == 64
    assert straddle >= 50
    # the over-64 sentences start their chunks: their first 192 units are one flush, in which the
    # slow units sit at hard index 62.. / 63.. / 64.. / 65.. / 100.. and 0..189
    assert len(over_at) == 6 and all(s % kChunk == 0 for s in over_at)


def _assert_same(ids, o, e, eo, text, off):
    if np.array_equal(o, eo) and np.array_equal(ids, e):
        return
    for k in range(len(off) - 1):
        a, b = ids[o[k]:o[k + 1]], e[eo[k]:eo[k + 1]]
        if not np.array_equal(a, b):
            raise AssertionError('sentence {} of {} ({!r}): got {} expected {}'.format(
                k, len(off) - 1, bytes(text[off[k]:off[k + 1]])[:300], a.tolist()[:60],
                b.tolist()[:60]))
    raise AssertionError('outputs differ')


MODES = {
    'default': {},
    'plain': {'LDDL_TOKENIZE_PATH': 'plain'},
    'memo1': {'LDDL_TOKENIZE_MEMO_SAMPLE': '1'},
    'memo64': {'LDDL_TOKENIZE_MEMO_SAMPLE': '64'},
    'grid1': {'LDDL_TOKENIZE_GRID': '1'},
    'memo64_grid1': {'LDDL_TOKENIZE_MEMO_SAMPLE': '64', 'LDDL_TOKENIZE_GRID': '1'},
    # the wave kernel takes its words from the same unit_word (always the byte-by-byte form)
    'wave': {'LDDL_TOKENIZE_PATH': 'wave'},
}


@pytest.mark.parametrize('slow', ['regs', 'loop'])
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('case', ['uncased', 'cased'])
def test_slow_units_vs_oracle(corpus, ctxs, expected, monkeypatch, case, mode, slow):
    text, off = corpus[0], corpus[1]
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv('LDDL_TOKENIZE_SLOW', slow)
    for mp in (512, 9):
        ids, o = ctxs[case].tokenize_host(text, off, max_pieces=mp)
        e, eo = expected[case, mp]
        _assert_same(ids, o, e, eo, text, off)


def test_slow_knob_unknown_raises(ctxs, monkeypatch):
    monkeypatch.setenv('LDDL_TOKENIZE_SLOW', 'fast')
    text = np.frombuffer(b'hello world', np.uint8)
    with pytest.raises(Exception, match='LDDL_TOKENIZE_SLOW'):
        ctxs['uncased'].tokenize_host(text, np.asarray([0, len(text)], np.int64))
