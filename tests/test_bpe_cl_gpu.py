"""The cl100k pre-tokenizer and ignore_merges on the GPU: `BpeContext` against the
sequential reference (bpe_cl_ref.py) at the shapes where a run's carry crosses tiles. The hand
table merges equal neighbours, so a misplaced boundary changes the ids; pretoken_stats counts
the starts besides."""
import numpy as np
import pytest

import bpe_cl_ref
import bpe_ref
from lddl_amd import bpe as B
from test_bpe_cl_host import TABLE

pytestmark = pytest.mark.gpu
ARABIC3 = '٣'  # U+0663, a digit of two bytes


def hand_tables():
    """The 256 byte tokens, doublings of the run characters up to 8, `abc` that no merge reaches
    (only b c -> bc) and a token of 70 spaces behind the 64 that the doublings reach."""
    tokens, merges = [bytes([b]) for b in range(256)], []

    def merge(l, r):
        tokens.append(l + r)
        merges.append([tokens.index(l), tokens.index(r), len(tokens) - 1])
    for c in (b'1', b' ', b'\n', b'!', ARABIC3.encode()):
        if len(c) == 2:
            merge(c[:1], c[1:])
        for k in range(3 if c != b' ' else 6):
            merge(c * 2 ** k, c * 2 ** k)
    merge(b'b', b'c')
    merge(b' ', b'a')
    return tokens + [b'abc', b' ' * 70], merges


CONTEXTS = {}


def context(name, **kw):
    key = (name,) + tuple(sorted(kw.items()))
    if key not in CONTEXTS:
        tokens, merges = hand_tables() if name == 'hand' else B.load_tables(B.SYNTH_VOCAB, B.SYNTH_MERGES)[::2]
        cl = kw.get('pattern', 'gpt2') != 'gpt2'
        ref = bpe_cl_ref.ClTables(tokens, merges, B.check_options(**kw)[1] or 3, kw.get('ignore_merges', False))
        if not cl:  # GPT-2's split under the whole-word lookup
            ref.pretokens = bpe_ref.pretokens
        CONTEXTS[key] = (B.BpeContext.from_tables(tokens, merges, **kw), ref)
    return CONTEXTS[key]


def check(docs, name='hand', **kw):
    """Every document (str, one sentence) in one call: ids against the reference's encode and
    the number of pre-tokens against its split."""
    import torch
    ctx, ref = context(name, **kw)
    raw = [d.encode('utf-8') for d in docs]
    off = np.zeros(len(raw) + 1, np.int64)
    np.cumsum([len(d) for d in raw], out=off[1:])
    text = np.frombuffer(b''.join(raw), np.uint8).copy()
    ids, out = ctx.tokenize_host(text, off, None, int(off[-1]))
    for d, (a, b) in enumerate(zip(out, out[1:])):
        assert ids[a:b].tolist() == ref.encode(raw[d]), (d, docs[d][:80])
    stats = ctx.pretoken_stats(*(torch.from_numpy(x).to(ctx.device) for x in (text, off)))
    assert stats[0].item() == sum(len(ref.pretokens(d)) for d in docs)


def tile(s):
    """s and a filler word up to the next multiple of 64 bytes: the next document starts a tile."""
    return s + ' ' + 'z' * ((-len(s.encode('utf-8')) - 1) % 64)


@pytest.mark.parametrize('digit', ['1', ARABIC3])
@pytest.mark.parametrize('pattern', ['cl100k', 'qwen2'])
def test_digit_runs_across_tiles(pattern, digit):
    docs = [tile('a' * at + digit * n + tail) for at in (61, 62, 63, 64, 255, 256)
            for n in (1, 2, 3, 4, 5, 6, 7, 64, 65, 130, 200) for tail in ('', 'x')]
    docs.append(tile('a' * 63 + digit * 4500 + 'x'))  # over 64 whole-run tiles: the carry walks
    docs += ['ab' + digit * 70, digit * 70 + 'x', digit * 4]  # a document starts inside a run
    check(docs, pattern=pattern)


@pytest.mark.parametrize('before', ['a', '!'])
def test_whitespace_runs_across_tiles(before):
    docs, ends = [], []
    for n in (1, 2, 63, 64, 65, 129, 300):
        for nl in (0, n - 1, min(n - 1, 70), None):  # first, last, in the tile after, absent
            run = ''.join('\n' if k == nl else ' ' for k in range(n))
            docs += [tile('b' * 59 + before + run + after) for after in ('a', '1', '(', '')]
            ends.append('b' * 59 + before + run)  # the run ends its document, another follows
    docs += [tile(before + '\n' * 200 + ' x'), tile('b' * 70 + before + '\n' * 200 + ' \n y')]
    # `before` is a tile's last byte and whole tiles of newlines follow: the empty run's carry
    docs += [tile('b' * 63 + before + '\n' * n + ' \n y') for n in (64, 70, 128, 4500)]
    # over 64 whole-run tiles each way: the carries walk
    docs += [tile(before + '\n' * 4500 + ' x')]
    docs += [tile(before + '\n' + ' ' * 4500 + tail) for tail in ('\nx', 'x')]
    check(docs + ends, pattern='cl100k')


@pytest.mark.parametrize('at', range(60, 67))
def test_local_rules_at_every_offset(at):
    check([tile('x' * (at - 1) + '\n' + s) for s in TABLE], pattern='cl100k')
    check([tile('x' * at + s) for s in TABLE], pattern='qwen2')


@pytest.mark.parametrize('pattern', ['gpt2', 'cl100k'])
def test_ignore_merges(pattern):
    words = [tile('q' * 61 + '\nabc'), 'abc', 'abd', 'xbc', 'q' * 62 + ' abc', 'q' * 61 + ' abc abc',
             ' ' * 70, ' ' * 71, 'a' + ' ' * 70, tile('q' * 30) + ' ' * 70]
    ctx, ref = context('hand', pattern=pattern, ignore_merges=True)
    abc, bc = ctx.tokens.index(b'abc'), ctx.tokens.index(b'bc')
    assert ctx.encode('abc') == [abc] and ctx.encode('abd') == [97, 98, 100]
    assert context('hand', pattern=pattern)[0].encode('abc') == [97, bc]
    assert ctx.encode(' ' * 70) == [ctx.tokens.index(b' ' * 70)]
    assert ctx.encode('q' * 61 + '\nabc')[-2:] == [10, abc]  # abc at bytes 62 .. 64: the second window
    check(words, pattern=pattern, ignore_merges=True)
    check(words, pattern=pattern)


@pytest.mark.parametrize('kw', [{}, dict(pattern='cl100k'), dict(pattern='cl100k', ignore_merges=True)],
                         ids=['default', 'cl100k', 'cl100k_whole'])
def test_synthetic_text(kw):
    from lddl_amd import synth
    corp = synth.generate(seed=35, n_bytes=1 << 18, nonascii_frac=0.05, threads=4)
    ctx, ref = context('synth', **kw)
    ids, off = ctx.tokenize_host(corp.text, corp.sent_off, corp.doc_sent_off, 1 << 18)
    text, so = corp.text.tobytes(), corp.sent_off
    for d in range(corp.n_doc):
        s0, s1 = corp.doc_sent_off[d], corp.doc_sent_off[d + 1]
        assert ids[off[s0]:off[s1]].tolist() == ref.encode(text[so[s0]:so[s1]]), d


def test_set_pattern_refuses_unknown_values():
    from lddl_amd._native import lib
    ctx = context('hand')[0]
    for args in ((b'o200k', 3), (b'cl100k', 2), (b'gpt2', 3)):
        assert lib.lddl_bpe_set_pattern(ctx.handle, *args) == -1 and lib.lddl_last_error()
    assert lib.lddl_bpe_set_whole_words(ctx.handle, 2) == -1
    assert ctx.encode('1111') == [ctx.tokens.index(b'1111')]  # still GPT-2's split


def test_gpt_loader_with_the_keywords(tmp_path):
    from lddl_amd.torch import get_gpt_pretrain_data_loader
    lines = ["Llama's 12345 tokens,\tsplit (here)!" * 3, 'second   document 2024', "THIRD'S the last one."]
    (tmp_path / '0.txt').write_text('\n'.join(lines))
    kw = dict(pattern='cl100k', ignore_merges=True)
    a = get_gpt_pretrain_data_loader(str(tmp_path), (B.SYNTH_VOCAB, B.SYNTH_MERGES, kw), batch_size=1,
                                     max_seq_length=32, shuffle_docs=False)
    rows = {tuple(x['input_ids'][0].tolist()) for x in a}  # a seeded permutation orders them
    ref, eos = context('synth', **kw)[1], a.bpe.special_ids['</s>']
    want = [i for ln in lines for i in ref.encode(ln.encode('utf-8')) + [eos]]
    assert len(want) > 64 and all(tuple(want[k:k + 32]) in rows for k in range(0, len(want) - 32, 32))


def test_tokenizer_json_context_and_loader(tmp_path):
    import json
    from lddl_amd.torch import get_gpt_pretrain_data_loader
    from test_bpe_cl_host import GOLDEN
    js = json.load(open(GOLDEN, encoding='utf-8'))
    for b, c in B.bytes_to_unicode().items():  # the golden file and the 256 byte tokens
        js['model']['vocab'].setdefault(c, 8 + b)
    (tmp_path / 'tokenizer.json').write_text(json.dumps(js), encoding='utf-8')
    ctx = B.BpeContext.from_tokenizer_json(str(tmp_path / 'tokenizer.json'))
    assert (ctx.pattern, ctx.ignore_merges, ctx.special_ids['<|end_of_text|>']) == ('cl100k', True, 7)
    assert ctx.tokens[7] == b'' and ctx.encode('abc a1234') == [4, 6, 8 + 49, 8 + 50, 8 + 51, 8 + 52]
    (tmp_path / '0.txt').write_text('abc a\nbc\nabc a a a a a')
    a = get_gpt_pretrain_data_loader(str(tmp_path), str(tmp_path / 'tokenizer.json'), batch_size=1,
                                     max_seq_length=4, shuffle_docs=False)
    rows = [x['input_ids'][0].tolist() for x in a]
    # abc, " a", <|end_of_text|> from added_tokens, bc, ...
    assert sorted(rows)[:2] == [[4, 6, 7, 3], [7, 4, 6, 6]]
