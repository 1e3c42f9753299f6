"""Byte-level BPE on the GPU: lddl_bpe_tokenize through `BpeContext`, ids and
sent_len bit for bit against the sequential reference (bpe_ref.py) at the shapes where the
kernels take another path; the BART loader with bpe=; lddl_bart_denoise_bits."""
import itertools
import os

import numpy as np
import pytest

import bpe_ref
from conftest import REPO
from lddl_amd import bpe as B  # ImportError without the feature

pytestmark = pytest.mark.gpu
MW = bpe_ref.MAX_WORD


def hand_table(*pairs):
    """The 256 byte tokens (id = byte) and one merge per (left, right) pair of byte strings."""
    tokens, merges = [bytes([b]) for b in range(256)], []
    for l, r in pairs:
        if l + r not in tokens:
            tokens.append(l + r)
        merges.append([tokens.index(l), tokens.index(r), tokens.index(l + r)])
    return tokens, merges


def doubling(a, b, n):  # (a, b), (ab, ab), (abab, abab), ...
    return [(a, b)] + [((a + b) * 2 ** k, (a + b) * 2 ** k) for k in range(n)]


TABLES = {
    'two': hand_table((b' ', b'a'), (b'a', b's')),
    'bc_ab': hand_table((b'b', b'c'), (b'a', b'b')),
    'ab_bc': hand_table((b'a', b'b'), (b'b', b'c')),
    'aa': hand_table((b'a', b'a'), (b'aa', b'aa'), (b'aaaa', b'aaaa'), (b'aa', b'a')),
    # two lines produce aba; (aba, b) ranks between them
    'ababa': hand_table((b'a', b'b'), (b'ab', b'a'), (b'b', b'a'), (b'aba', b'b'), (b'a', b'ba')),
    'edges': hand_table(*doubling(b'!', b'?', 5), (b'!?', b'!')),
}
CONTEXTS = {}


def context(name):
    if name not in CONTEXTS:
        if name == 'synth':
            CONTEXTS[name] = (B.BpeContext(B.SYNTH_VOCAB, B.SYNTH_MERGES),
                              bpe_ref.Tables(*B.load_tables(B.SYNTH_VOCAB, B.SYNTH_MERGES)[::2]))
        else:
            CONTEXTS[name] = (B.BpeContext.from_tables(*TABLES[name]), bpe_ref.Tables(*TABLES[name]))
    return CONTEXTS[name]


def check(name, docs, max_pieces=512, per_sentence=False):
    """docs: lists of sentences (str). Tokenizes them in one call and compares every sentence's
    ids and sent_len with the reference; per_sentence: without doc_sent_off."""
    import torch
    ctx, ref = context(name)
    docs = [[s.encode('utf-8') for s in d] for d in docs]
    if per_sentence:
        docs = [[s] for d in docs for s in d]
    sents = [s for d in docs for s in d]
    so = np.zeros(len(sents) + 1, np.int64)
    np.cumsum([len(s) for s in sents], out=so[1:])
    dso = np.zeros(len(docs) + 1, np.int64)
    np.cumsum([len(d) for d in docs], out=dso[1:])
    dev = lambda a: torch.from_numpy(a).to(ctx.device)  # noqa: E731
    ids, sl = ctx.tokenize(dev(np.frombuffer(b''.join(sents) or b' ', np.uint8).copy()), dev(so),
                           None if per_sentence else dev(dso), max_pieces)
    ids, sl = ids.cpu().numpy(), sl.cpu().numpy()
    want = [x for d in docs for x in ref.encode_sentences(d, max_pieces)]
    np.testing.assert_array_equal(sl, [len(x) for x in want])
    at = np.concatenate([so[i] + np.arange(len(x)) for i, x in enumerate(want)] or [[]]).astype(np.int64)
    np.testing.assert_array_equal(ids[at], np.concatenate(want or [[]]).astype(np.int32))
    return want


@pytest.mark.parametrize('per_sentence', [True, False], ids=['own_documents', 'eight_a_document'])
def test_boundaries_of_every_short_string(per_sentence):
    strings = [''.join(t) for n in range(6)
               for t in itertools.product("as1 \n'!é", repeat=n)]
    check('two', [strings[i:i + 8] for i in range(0, len(strings), 8)], per_sentence=per_sentence)


@pytest.mark.parametrize('name,words', [
    ('bc_ab', ['abc', 'abcabc', 'xyz']), ('ab_bc', ['abc', 'bcabc']),
    ('aa', ['a' * n for n in (1, 2, 3, 63, 64, 65, 127, 128, 129, MW, MW + 1, 2 * MW + 3)]),
    ('ababa', ['ababa', 'abab', 'bababab', 'ab' * 40, 'qrs'])])
def test_merges_on_hand_built_tables(name, words):
    check(name, [[w] for w in words])
    check(name, [[' '.join(words)]])
    check(name, [[aligned(p + w)] for w in words for p in ('', '!')])  # from lane 0 and lane 1


def aligned(s):
    """s, then one-byte pre-tokens (no letter, no punctuation) up to the next multiple of 64, one
    at least: the text after it starts a tile, in the same document or the next."""
    return s + ('1\n' * 32)[:64 - len(s) % 64]


def edge_docs():
    """A 5- and a 40-byte word from tile offsets 59, 60, 63 and 64, a 64- and a 65-byte word from
    offsets 0 and 1 (every document starts a tile), then two long words in one sentence and a
    pre-token over a sentence boundary."""
    pad = lambda k: ('a1' * 64)[:k]  # noqa: E731  (one pre-token per byte)
    docs = [[aligned(pad(k) + w)] for k in (59, 60, 63, 64) for w in ('!?!?!', '!?' * 20)]
    docs += [[aligned(pad(k) + '!?' * 32 + tail)] for k in (0, 1) for tail in ('', '!')]
    return docs + [['!?' * 100 + ' ' + '!' * 300 + ' a', 'b' * 70 + ' ']]


def test_tile_edges():
    check('edges', edge_docs())
    check('edges', [[''.join(s for d in edge_docs() for s in d)]])


def test_pretoken_stats_count_the_second_window_and_the_long_list():
    import torch
    ctx = context('edges')[0]
    docs, spans, pos = edge_docs(), [], 0
    for d in docs:
        for w in bpe_ref.pretokens(''.join(d)):
            spans.append((pos, len(w)))  # ASCII: characters are bytes
            pos += len(w)
    cross = [n for x, n in spans if x // 64 != (x + n - 1) // 64]
    text = np.frombuffer(''.join(s for d in docs for s in d).encode(), np.uint8).copy()
    ends = np.cumsum([0] + [len(s) for d in docs for s in d])
    dso = np.cumsum([0] + [len(d) for d in docs])
    got = ctx.pretoken_stats(*(torch.from_numpy(a).to(ctx.device) for a in (text, ends, dso)))
    assert got.tolist() == [len(spans), sum(n <= 64 for n in cross), sum(n > 64 for n in cross)]
    assert sum(n <= 64 for n in cross) >= 6 and sum(n > 64 for n in cross) >= 5


@pytest.mark.parametrize('max_pieces', [1, 7, 512])
def test_layout(max_pieces):
    long_sentence = 'a1' * 300  # 600 pieces
    check('two', [['', ' ', ' \n ', long_sentence, ''], ['as as. ', ' \n'], [], ['a']], max_pieces)
    check('two', [[long_sentence]], max_pieces)
    check('two', [['as ', 'a'] * 32 + ['as']], max_pieces)  # 65 sentences


def test_text_classes_with_the_synthetic_vocabulary():
    check('synth', [['\u0395\u03bb\u03bb\u03b7\u03bd\u03b9\u03ba\u03ac \u0420\u0443\u0441\u0441\u043a\u0438\u0439 \u4e2d\u6587\u5b57 ',
                     "it's \u00b2\u00bd\u2167 x2 e\u0301 \u00e9 ", 'a b\u00a0c\u3000d\u2028e \U0001F601!'],
                    ["we'll they've  I'm\n\n'd "]])


def test_synth_corpus_documents_concatenate_to_encode():
    from lddl_amd import synth
    corp = synth.generate(seed=77, n_bytes=1 << 20, nonascii_frac=0.05, threads=4)
    ctx, ref = context('synth')
    ids, off = ctx.tokenize_host(corp.text, corp.sent_off, corp.doc_sent_off, 1 << 20)
    text, so = corp.text.tobytes(), corp.sent_off
    for d in range(corp.n_doc):
        s0, s1 = corp.doc_sent_off[d], corp.doc_sent_off[d + 1]
        assert ids[off[s0]:off[s1]].tolist() == ref.encode(text[so[s0]:so[s1]]), d


def test_loader_with_bpe(tmp_path):
    import torch
    from lddl_amd.torch import get_bart_pretrain_data_loader
    text = ['Chunk number {} has words. It has {} sentences! Does it end? Yes {}.'.format(
        i, 'many ' * (i % 5), 'and on ' * i) for i in range(11)]
    for k in range(2):
        (tmp_path / '{}.txt'.format(k)).write_text('\n'.join(text[k::2]))
    make = lambda **kw: get_bart_pretrain_data_loader(  # noqa: E731
        str(tmp_path), None, 4, 256, bpe=(B.SYNTH_VOCAB, B.SYNTH_MERGES), **kw)
    a = make()
    batches = list(a)
    tbl, n_pieces = a.tokenize_round(a.files)
    perm = torch.from_numpy(a.order(0, 0, 11)).to(tbl[0].device)
    for step, x in enumerate(batches):
        want = a.denoise(tbl, perm[4 * step:4 * step + 4], x['input_ids'].shape[1], 0, step)
        assert all(torch.equal(x[k], want[k]) for k in x)
    ref, sp = context('synth')[1], a._bpe.special_ids
    chunks = [c for k in range(2) for c in text[k::2]]
    plain = make(mask_ratio=0.0, permute_sentence_ratio=0.0)
    rows = [r.tolist() for x in plain for r in x['input_ids']]
    order = plain.order(0, 0, 11)
    for row, c in zip(rows, order):
        body = [t for t in row if t not in (sp['<s>'], sp['</s>'], sp['<pad>'])]
        assert body == ref.encode(chunks[c].encode('utf-8'))


def test_denoise_bits_equals_denoise_with_the_context_bitmap():
    import torch
    from lddl_amd.context import Context, _ptr
    from lddl_amd.torch import bart_denoise
    vocab = os.path.join(REPO, 'lddl_amd', 'assets', 'vocab_synth_uncased_30522.txt')
    ctx = Context(vocab)
    cont = np.array([t.startswith('##') and len(t) > 2 for t in ctx.tokens])
    bits = np.packbits(np.pad(cont, (0, -len(cont) % 32)), bitorder='little').view(np.uint32)
    d_bits = torch.from_numpy(bits.astype(np.int32)).to(ctx.device)
    rng = np.random.default_rng(3)
    lens = [5, 0, 64, 65, 1, 30]
    so = np.concatenate([[0], np.cumsum([n + 2 for n in lens])]).astype(np.int64)
    dev = lambda a: torch.from_numpy(a).to(ctx.device)  # noqa: E731
    tab = [dev(rng.integers(1000, len(cont), so[-1]).astype(np.int32)), dev(so),
           dev(np.array(lens, np.int32)), dev(np.array([0, 2, 3, 6], np.int64))]

    class Bits(B.BpeContext):  # what bart_denoise reads of a BpeContext, without its tables
        __init__ = lambda self: None  # noqa: E731
        device, special_ids = ctx.device, dict(zip(('<s>', '</s>', '<pad>', '<mask>'), (
            ctx.special_ids[k] for k in ('[CLS]', '[SEP]', '[PAD]', '[MASK]'))))
        cont_bits = (_ptr(d_bits), len(cont))
        __len__ = lambda self: len(cont)  # noqa: E731
    a = bart_denoise(ctx, *tab, seq_len=104, mask=(0.3, 5, 1))
    b = bart_denoise(Bits(), *tab, seq_len=104, mask=(0.3, 5, 1))
    assert all(torch.equal(a[k], b[k]) for k in a)
