"""The cl100k pre-tokenizer, host side (no GPU): the reference against the `regex`
pattern, `load_tokenizer_json` on a hand-written file, and the argument errors of the keywords."""
import json
import os
import random

import pytest

import bpe_cl_ref
from conftest import REPO
from lddl_amd import bpe as B

GOLDEN = os.path.join(REPO, 'tests', 'golden', 'bpe_cl_tokenizer.json')
CL100K = next(k for k, v in B.SPLIT_REGEX.items() if v == 'cl100k')
TABLE = {
    "don't 'the 'S xſ": ['don', "'t", " '", 'the', " '", 'S', ' xſ'],
    '12345 1234567x': ['123', '45', ' ', '123', '456', '7', 'x'],
    'a((b (c  (d': ['a', '((', 'b', ' (', 'c', ' ', ' (', 'd'],
    'x!!\n\n  y': ['x', '!!\n\n', ' ', ' y'],
    '  \n \n  x \n': ['  \n \n', ' ', ' x', ' \n'],
    '...\n\r \nz': ['...\n\r', ' \n', 'z'],
    '1½٣٤': ['1½٣', '٤'],
    "a'sb'REd": ['a', "'s", 'b', "'RE", 'd'],
    "x.'s": ['x', ".'", 's'],
    'a\xa0b　 c': ['a', '\xa0b', '　', ' c'],
    "'ſx": ["'ſ", 'x'],
}


def test_reference_matches_regex():
    regex = pytest.importorskip('regex')
    rng = random.Random(35)
    alphabet = ['a', 'é', '1', '٣', '½', "'", '(', '!', '.', ' ', '\t', '\n', '\r', '\xa0', '　', 'ſ', 'S']
    strings = list(TABLE) + [''.join(rng.choice(alphabet) for _ in range(rng.randint(1, 12)))
                             for _ in range(4000)]
    for group, rx in ((3, CL100K), (1, next(k for k, v in B.SPLIT_REGEX.items() if v == 'qwen2'))):
        pat = regex.compile(rx)
        for s in strings:
            assert bpe_cl_ref.pretokens(s, group) == pat.findall(s), (s, group)


def test_reference_on_the_stated_strings():
    for s, want in TABLE.items():
        assert bpe_cl_ref.pretokens(s) == want, s
    assert bpe_cl_ref.pretokens('12345', 1) == list('12345')


def test_tokenizer_json(tmp_path):
    tokens, vocab, merges, options = B.load_tokenizer_json(GOLDEN)
    assert tokens == [b'a', b'b', b'c', b'bc', b'abc', b' ', b' a', b'']
    assert merges.tolist() == [[1, 2, 3], [5, 0, 6]]  # "b c" and ["Ġ", "a"]
    assert options == dict(pattern='cl100k', ignore_merges=True, added={'<|end_of_text|>': 7})
    assert vocab['<|end_of_text|>'] == 7
    js = json.load(open(GOLDEN, encoding='utf-8'))
    split = js['pre_tokenizer']['pretokenizers'][0]['pattern']
    for rx, want in ((CL100K.replace('{1,3}', ''), 'qwen2'), (CL100K.replace('{1,3}', '{1,2}'), None)):
        split['Regex'] = rx
        (tmp_path / 't.json').write_text(json.dumps(js), encoding='utf-8')
        if want:
            assert B.load_tokenizer_json(str(tmp_path / 't.json'))[3]['pattern'] == want
        else:
            with pytest.raises(ValueError, match=r'\{1,2\}'):
                B.load_tokenizer_json(str(tmp_path / 't.json'))
    del js['model']['ignore_merges']
    split['Regex'] = CL100K
    (tmp_path / 't.json').write_text(json.dumps(js), encoding='utf-8')
    assert B.load_tokenizer_json(str(tmp_path / 't.json'))[3]['ignore_merges'] is False


def test_keywords_are_refused_before_the_gpu(tmp_path, monkeypatch):
    from lddl_amd.torch import get_gpt_pretrain_data_loader as make
    monkeypatch.setattr(B, 'create_native', lambda *a, **k: pytest.fail('the GPU was touched'))
    (tmp_path / '0.txt').write_text('One document.')
    files = (B.SYNTH_VOCAB, B.SYNTH_MERGES)
    for kw in (dict(pattern='o200k'), dict(digit_group=3), dict(pattern='cl100k', digit_group=2),
               dict(pattern='qwen2', digit_group=True), dict(ignore_merges=1)):
        with pytest.raises(ValueError):
            B.BpeContext(*files, **kw)
        with pytest.raises(ValueError):
            B.BpeContext.from_tables([], [], **kw)
        with pytest.raises(ValueError):
            make(str(tmp_path), files + (kw,), batch_size=2)
    for bpe in (files + (dict(device=0),), files + ('cl100k',), str(tmp_path / 'none.json')):
        with pytest.raises((ValueError, FileNotFoundError)):
            make(str(tmp_path), bpe, batch_size=2)
    assert B.check_options('qwen2') == ('cl100k', 1, False)
    assert B.check_options('cl100k', ignore_merges=True) == ('cl100k', 3, True)
    from lddl_amd._native import lib
    assert lib.lddl_bpe_set_pattern(None, b'cl100k', 3) == -1 and lib.lddl_bpe_set_whole_words(None, 1) == -1
