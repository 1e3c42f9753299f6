"""SentencePiece unigram, host side (no GPU): the reference (unigram_ref.py) and
`load_model` against the `sentencepiece` package where it is installed, the refusals of
lddl_unigram_create and lddl_unigram_tokenize, and the argument errors of the loaders' unigram=.

The reference encodes every word from best[0] = 0.0f, as the header states; SentencePiece adds
in float32 along the whole sentence, so two paths of one word whose sums tie (`l` + `ll` against
`ll` + `l`) can round apart there. The word-by-word comparison is therefore exact, and the
whole-sentence one is exact up to the order of the pieces (measured on the 472 sentences below:
3 differ, each in the order of two pieces inside one tie)."""
import numpy as np
import pytest

import unigram_ref
from lddl_amd import unigram as U  # ImportError without the feature

M = '▁'
HAND = ['', '   ', 'a', ' a  b ', 'the  quick   fox', 'x' * 200, 'zq中文é \U0001F601\U0001F601a',
        'Hello, world! 1234', ' leading and trailing ']


def test_reference_and_load_model_match_sentencepiece():
    spm = pytest.importorskip('sentencepiece')
    from lddl_amd import synth
    sp = spm.SentencePieceProcessor(model_file=unigram_ref.SYNTH_MODEL)
    pieces, scores, types, unk, ascii_ws = U.load_model(unigram_ref.SYNTH_MODEL)
    assert pieces == [sp.id_to_piece(i).encode() for i in range(sp.get_piece_size())]
    assert scores.tolist() == [np.float32(sp.get_score(i)) for i in range(len(pieces))]
    assert unk == sp.unk_id() and not ascii_ws and 1900 <= len(pieces) <= 2100
    assert [i for i, t in enumerate(types) if t == U.CONTROL] == [sp.piece_to_id(p) for p in (
        '<pad>', '</s>', '<s>', '<mask>')]
    ref = unigram_ref.Tables(pieces, scores, types, unk)
    for s in HAND:
        assert ref.encode(s.encode()) == sp.encode(s), s
    corp = synth.generate(seed=5, n_bytes=60000, nonascii_frac=0.05, threads=1)
    text, so = corp.text.tobytes(), corp.sent_off
    assert corp.n_sent > 300
    for i in range(corp.n_sent):
        s = text[so[i]:so[i + 1]]
        got = ref.encode(s)
        assert got == [t for w in s.decode().split(' ') if w for t in sp.encode(w)], s
        assert sorted(got) == sorted(sp.encode(s.decode())), s


def refusal(pieces, scores, types=None, unk_id=0):
    from lddl_amd._native import NativeError
    with pytest.raises(NativeError) as e:
        U.create_native(*U.check_tables(pieces, scores, types, unk_id), False, 0)
    return str(e.value)


@pytest.mark.parametrize('pieces,scores,types,unk_id,msg', [
    (['<unk>', 'a'], [0, -1], None, 0, 'space mark E2 96 81 alone'),
    (['<unk>', M, 'a' + M + 'b'], [0, -1, -1], None, 0, 'interior'),
    (['<unk>', M], [0, -1], None, 2, 'outside the vocabulary'),
    (['<unk>', M], [0, -1], [1, 1], 0, 'not the one UNKNOWN'),
    (['<unk>', M, '<unk2>'], [0, -1, 0], [2, 1, 2], 0, 'not the one UNKNOWN'),
    (['<unk>', M, ''], [0, -1, -1], None, 0, 'is empty'),
    (['<unk>', M, 'a', 'a'], [0, -1, -1, -2], None, 0, 'repeats piece 2'),
    (['<unk>', M, 'a'], [0, -1, float('nan')], None, 0, 'not finite'),
    (['<unk>', M, 'a'], [0, -1, float('-inf')], None, 0, 'not finite'),
    (['<unk>', M] + ['a' * k for k in range(1, 18)], [0] + [-1] * 18, None, 0, 'nested'),
])
def test_create_refuses(pieces, scores, types, unk_id, msg):
    assert msg in refusal(pieces, scores, types, unk_id)


def test_native_refusals_with_null_pointers():
    import ctypes
    from lddl_amd._native import lib
    h = ctypes.c_void_p()
    assert lib.lddl_unigram_create(0, None, None, None, None, 1, 0, 0, ctypes.byref(h)) == -1
    assert lib.lddl_unigram_create(0, None, None, None, None, 1, 0, 0, None) == -1
    off, sc, ty = np.zeros(2, np.int64), np.zeros(1, np.float32), np.ones(1, np.int32)
    args = [a.ctypes.data for a in (np.zeros(1, np.uint8), off, sc, ty)]
    assert lib.lddl_unigram_create(0, *args, 0, 0, 0, ctypes.byref(h)) == -1  # n_pieces < 1
    assert lib.lddl_unigram_create(0, *args, 1, 0, 2, ctypes.byref(h)) == -1
    assert b'flags' in lib.lddl_last_error()
    assert lib.lddl_unigram_tokenize(None, None, None, 0, None, 0, None, 0, 512, None, None) == -1
    assert lib.lddl_unigram_word_stats(None, None, None, 0, None, 0, None, 0, None) == -1
    assert lib.lddl_unigram_info(None, None, None, None, None, None) == -1
    assert lib.lddl_unigram_cont_bits(None, None, None) == -1 and lib.lddl_unigram_destroy(None) == 0


def proto(fields):  # [(number, wire type, value)] -> bytes; lengths below 128
    out = b''
    for num, wt, v in fields:
        out += bytes([num << 3 | wt]) + (bytes([v]) if wt == 0 else bytes([len(v)]) + v if wt == 2 else v)
    return out


def model_bytes(model_type=1, flag=None, name=b'identity'):
    import struct
    piece = lambda p, s, t: (1, 2, proto([(1, 2, p), (2, 5, struct.pack('<f', s)), (3, 0, t)]))  # noqa: E731
    norm = [(1, 2, name)] + ([(flag, 0, 0)] if flag else [])
    return proto([piece(b'<unk>', 0, 2), piece(M.encode(), -1, 1), piece(b'ab', -2.5, 1),
                  piece(b'<x>', 0, 4), (2, 2, proto([(3, 0, model_type)])), (3, 2, proto(norm))])


def test_load_model_and_the_loaders_refuse_before_the_gpu(tmp_path, monkeypatch):
    from lddl_amd import bpe as B
    from lddl_amd.torch import get_roberta_pretrain_data_loader, get_t5_pretrain_data_loader
    monkeypatch.setattr(U, 'create_native', lambda *a, **k: pytest.fail('the GPU was touched'))
    files = {'good': model_bytes(), 'nfkc': model_bytes(name=b'nmt_nfkc'), 'bpe': model_bytes(2),
             'junk': b'\xff\xff\xff', 'empty': b'', 'no_prefix': model_bytes(flag=3),
             'extra_ws': model_bytes(flag=4), 'no_escape': model_bytes(flag=5)}
    for k, v in files.items():
        (tmp_path / k).write_bytes(v)
    p = lambda k: str(tmp_path / k)  # noqa: E731
    pieces, scores, types, unk, ascii_ws = U.load_model(p('good'))
    assert (pieces, types.tolist(), unk, ascii_ws) == ([b'<unk>', M.encode(), b'ab', b'<x>'], [2, 1, 1, 4], 0, False)
    assert scores.tolist() == [0, -1, -2.5, np.float32(3 * -1 - 0.1)]  # USER_DEFINED: length * max - 0.1
    assert U.load_model(p('nfkc'))[4] is True
    (tmp_path / 'shards').mkdir()
    (tmp_path / 'shards' / '0.txt').write_text('A chunk. Of two sentences.')
    for make in (get_roberta_pretrain_data_loader, get_t5_pretrain_data_loader):
        for k, err in [('missing', FileNotFoundError)] + [(k, ValueError) for k in list(files)[2:]]:
            with pytest.raises(err):
                U.UnigramContext(p(k))
            with pytest.raises(err):
                make(p('shards'), batch_size=4, unigram=p(k))
        with pytest.raises(ValueError, match='not both'):
            make(p('shards'), (B.SYNTH_VOCAB, B.SYNTH_MERGES), 4, unigram=unigram_ref.SYNTH_MODEL)
        with pytest.raises(ValueError, match='bpe must be'):
            make(p('shards'), batch_size=4)
        assert make(p('shards'), batch_size=4, unigram=unigram_ref.SYNTH_MODEL).files
    with pytest.raises(ValueError):
        U.UnigramContext.from_tables(['<unk>', M], [0.0])
