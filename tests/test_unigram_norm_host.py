"""SentencePiece unigram, normaliser and byte fallback, host side (no GPU):
`load_normalizer` and the reference (unigram_norm_ref.py) against sentencepiece on the golden
nmt_nfkc model, and the refusals of a malformed character map."""
import struct

import pytest

import unigram_norm_ref as R
import unigram_ref
from lddl_amd import unigram as U

M = '▁'
TEXTS = ['Ｈｅｌｌｏ\u3000ｗｏｒｌｄ', 'ﬁne … ½ ㌀ ﷺ', 'か\u3099 ｶﾞ', 'a\u00a0b\u200bc\u00add', 'x\t y\nz \x01 \x7f w',
         'the quick brown fox', 'Zürich 中丁 q']
BAD = [b'a\x80b', b'ab \xe4\xb8', b'\xed\xa0\x80 \xc0\xaf']


@pytest.fixture(scope='module')
def nfkc():
    keys, repls, byte_pieces = U.load_normalizer(R.NFKC_MODEL)
    pieces, scores, types, unk, _ = U.load_model(R.NFKC_MODEL)
    return dict(zip(keys, repls)), R.ByteTables(pieces, scores, types, unk, byte_pieces=byte_pieces)


def test_the_map_of_the_golden_model(nfkc):
    rules, ref = nfkc
    assert len(rules) > 100000 and max(map(len, rules)) <= 61  # LDDL_UNIGRAM_NORM_MAX_KEY
    assert rules['ﬁ'.encode()] == b'fi' and rules[b'\t'] == b' ' and len(rules['ﷺ'.encode()]) == 33
    assert ref.byte_pieces.shape == (256,)
    assert U.load_normalizer(unigram_ref.SYNTH_MODEL) == ([], [], None)  # `identity`


@pytest.mark.parametrize('s', TEXTS + BAD)
def test_reference_against_sentencepiece(nfkc, s):
    spm = pytest.importorskip('sentencepiece')
    sp = spm.SentencePieceProcessor(model_file=R.NFKC_MODEL)
    rules, ref = nfkc
    raw = s.encode() if isinstance(s, str) else s
    words = [w for w in R.normalize(rules, raw).split(b' ') if w]
    assert sp.normalize(raw) == b''.join(M.encode() + w for w in words)
    if isinstance(s, str):
        # word by word: SentencePiece carries the Viterbi sum across words (§32's deviation)
        for w in words:
            assert ref.encode_word(w) == sp.encode(w.decode()), w


def test_a_malformed_map_is_refused(tmp_path):
    raw = open(R.NFKC_MODEL, 'rb').read()
    spec = next(v for n, _, v in U._fields(raw) if n == 3)
    cm = next(v for k, _, v in U._fields(spec) if k == 2)
    size = struct.unpack('<I', cm[:4])[0]
    units = list(struct.unpack('<{}I'.format(size // 4), cm[4:4 + size]))

    def rules(units, blob=cm[4 + size:], size=size):
        return U._charsmap_rules(struct.pack('<I', size) + struct.pack('<{}I'.format(len(units)), *units) + blob)

    assert len(rules(units)[0]) > 100000
    with pytest.raises(ValueError, match='trie of'):
        rules(units, size=len(cm))  # the trie size past the blob
    with pytest.raises(ValueError, match='offset leaves'):
        rules([units[0] | 0x7FFFFC00 | 0x200] + units[1:])
    with pytest.raises(ValueError, match='past the blob'):
        rules(units, blob=cm[4 + size:4 + size + 8])
