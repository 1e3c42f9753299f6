"""Byte-level BPE, host side (no GPU): the refusals of lddl_bpe_create, the argument
errors of `BpeContext` and of the loader's bpe=, the reference against the `regex` pattern and
HF tokenizers where they are installed, and the class table against unicodedata."""
import itertools
import json
import unicodedata

import numpy as np
import pytest

import bpe_ref
from lddl_amd import bpe as B  # ImportError without the feature

BASE = [bytes([b]) for b in range(256)]
ADVERSARIAL = ["a's 'll  x'd", " 's'm\n\n b", "a \n\n'ta1!?  ", "é x  y", "!'s''re 12ab ",
               "  ", "'", "a'l 've"] + [''.join(t) for t in itertools.product("as1 \n'!é", repeat=4)]


@pytest.mark.parametrize('tokens,merges,classes,msg', [
    (BASE[:65] + BASE[66:] + [b'ab'] * 2, [], None, 'single byte 0x41'),
    (BASE + [b'ab'], [[97, 98, 256], [97, 98, 256]], None, 'repeats the pair'),
    (BASE + [b'ab', b'abc'], [[256, 99, 257]], None, 'neither a base token'),
    (BASE + [b'ab'], [[97, 99, 256]], None, 'are not those of'),
    (BASE + [b'ab'], [[97, 98, 300]], None, 'outside the vocabulary'),
    (BASE, [], np.zeros(40, np.uint8), 'class table'),
])
def test_create_refuses(tokens, merges, classes, msg):
    from lddl_amd._native import NativeError
    with pytest.raises(NativeError, match=msg):
        B.create_native(tokens, np.array(merges, np.int32).reshape(-1, 3), 0, classes)


def test_create_refuses_ranks_of_2_to_the_26():
    import ctypes
    from lddl_amd._native import lib
    table = B.load_classes()
    off = np.arange(257, dtype=np.int64)
    blob = np.arange(256, dtype=np.uint8)
    one = np.zeros(3, np.int32)  # the count is refused before a line is read
    h = ctypes.c_void_p()
    assert lib.lddl_bpe_create(0, table.ctypes.data, len(table), blob.ctypes.data, off.ctypes.data,
                               256, one.ctypes.data, 1 << 26, ctypes.byref(h)) == -1
    assert b'2^26' in lib.lddl_last_error()
    assert lib.lddl_bpe_tokenize(None, None, None, 0, None, 0, None, 0, 512, None, None) == -1


def test_context_and_loader_refuse_bad_files_before_the_gpu(tmp_path, monkeypatch):
    from lddl_amd.torch import get_bart_pretrain_data_loader as make
    monkeypatch.setattr(B, 'create_native', lambda *a, **k: pytest.fail('the GPU was touched'))
    good = json.load(open(B.SYNTH_VOCAB, encoding='utf-8'))
    files = {'notjson': '{', 'list': '[1]', 'dup': json.dumps({'a': 0, 'b': 0}),
             'vocab': json.dumps(good), 'unknown': '#version: 0.2\nq zz\n', 'three': 'a b c\n'}
    for k, v in files.items():
        (tmp_path / k).write_text(v, encoding='utf-8')
    p = lambda k: str(tmp_path / k)  # noqa: E731
    bad = [(p('missing'), B.SYNTH_MERGES, FileNotFoundError), (B.SYNTH_VOCAB, None, FileNotFoundError),
           (p('notjson'), B.SYNTH_MERGES, ValueError), (p('list'), B.SYNTH_MERGES, ValueError),
           (p('dup'), B.SYNTH_MERGES, ValueError), (p('vocab'), p('unknown'), ValueError),
           (p('vocab'), p('three'), ValueError)]
    (tmp_path / 'shards').mkdir()
    (tmp_path / 'shards' / '0.txt').write_text('A chunk. Of two sentences.')
    for v, m, err in bad:
        with pytest.raises(err):
            B.BpeContext(v, m)
        with pytest.raises(err):
            make(p('shards'), None, 4, bpe=(v, m))
    for kw in (dict(bpe=B.SYNTH_VOCAB), dict(bpe=(B.SYNTH_VOCAB,)),
               dict(vocab_file=B.SYNTH_VOCAB, bpe=(B.SYNTH_VOCAB, B.SYNTH_MERGES))):
        with pytest.raises(ValueError):
            make(p('shards'), batch_size=4, **kw)
    assert make(p('shards'), None, 4, bpe=(B.SYNTH_VOCAB, B.SYNTH_MERGES)).format == 'txt'


def test_synthetic_vocabulary_files():
    tokens, vocab, merges = B.load_tables(B.SYNTH_VOCAB, B.SYNTH_MERGES)
    assert open(B.SYNTH_MERGES, encoding='utf-8').readline().startswith('#version:')
    assert 0 < len(merges) <= 4096 and all(vocab.get(s, -1) >= 0 for s in B.SPECIALS)
    assert sorted(t for t in tokens if len(t) == 1) == BASE


def test_reference_matches_regex_and_tokenizers():
    regex = pytest.importorskip('regex')
    pat = regex.compile(r"'s|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+")
    for s in ADVERSARIAL:
        assert bpe_ref.pretokens(s) == pat.findall(s), s
    # the installed regex module: \s is the White_Space property; U+001C-001F are not in it
    assert [c for c in range(0x250) if regex.match(r'\s', chr(c))] == sorted(
        c for c in bpe_ref.WHITE_SPACE if c < 0x250)
    tk = pytest.importorskip('tokenizers')
    hf = tk.Tokenizer(tk.models.BPE.from_file(B.SYNTH_VOCAB, B.SYNTH_MERGES))
    hf.pre_tokenizer = tk.pre_tokenizers.ByteLevel(add_prefix_space=False)
    tokens, _, merges = B.load_tables(B.SYNTH_VOCAB, B.SYNTH_MERGES)
    ref = bpe_ref.Tables(tokens, merges)
    for s in ADVERSARIAL[:8] + ['the quick brown fox, it said; we\'ll see 1234 times']:
        assert ref.encode(s.encode('utf-8')) == hf.encode(s).ids, s


def test_class_table_matches_unicodedata():
    raw = B.load_classes()
    if '.'.join(str(v) for v in raw[8:11]) != unicodedata.unidata_version:
        pytest.skip('the asset was built from another Unicode version')
    l1 = raw[32:32 + 2 * 4352].view(np.uint16)
    pages = raw[32 + 2 * 4352:].reshape(-1, 64)
    names = {'O': 0, 'L': 1, 'N': 2, 'S': 3}
    for cp in itertools.chain(range(0x3100), range(0xD7F0, 0xE010), range(0x1D7C0, 0x1D800),
                              range(0x1F5F0, 0x1F650), [0x10FFFF]):
        got = (pages[l1[cp >> 8], (cp & 255) >> 2] >> (2 * (cp & 3))) & 3
        assert got == names[bpe_ref.char_class(chr(cp))], hex(cp)
