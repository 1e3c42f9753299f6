"""SentencePiece unigram, normaliser and byte fallback on the GPU:
`UnigramContext.normalize` byte for byte and `tokenize` on its output id for id against the
sequential reference (unigram_norm_ref.py, which test_unigram_norm_host.py ties to
sentencepiece), at the tile offsets where the kernels take another path; the T5 loader."""
import numpy as np
import pytest

import unigram_norm_ref as R
from lddl_amd import unigram as U
from test_unigram_gpu import TABLES, pad

pytestmark = pytest.mark.gpu
OFFS = (0, 61, 62, 63)
# the vocabulary `unk` of test_unigram_gpu.py and the 256 byte pieces
PIECES = TABLES['unk'][0] + ['<0x{:02X}>'.format(b) for b in range(256)]
SCORES = TABLES['unk'][1] + [0.0] * 256
TYPES = [2] + [1] * (len(TABLES['unk'][0]) - 1) + [6] * 256
BYTES = np.arange(len(TABLES['unk'][0]), len(PIECES), dtype=np.int32)
FDFA = 'صلى الله عليه وسلم'  # 33 bytes
RULES = {
    'hand': {'中': 'z', 'X': 'abababababab', 'ﷺ': FDFA, 'D': '', 'S': ' ', '丁丂': 'y', '丂': 'w', 'ab': '9',
             'pq': '1', 'qr': '2', 'rs': '3', 'st': '4', 'tu': '5'},
    'swap': {'ab': '1', 'ba': '2'},  # chains of different entries never merge on abab...
}
CONTEXTS = {}


def context(name):
    """(context, reference tables, rules as a dict of bytes or None)."""
    if name not in CONTEXTS:
        if name == 'nfkc':
            keys, repls, bp = U.load_normalizer(R.NFKC_MODEL)
            p, s, t, unk, _ = U.load_model(R.NFKC_MODEL)
            CONTEXTS[name] = (U.UnigramContext(R.NFKC_MODEL), R.ByteTables(p, s, t, unk, byte_pieces=bp),
                              dict(zip(keys, repls)))
        else:
            rules = {k.encode(): v.encode() for k, v in RULES[name].items()} if name in RULES else None
            bp = None if name == 'off' else BYTES
            ctx = U.UnigramContext.from_tables(PIECES, SCORES, TYPES, byte_pieces=bp,
                                               normalizer=rules and (list(rules), list(rules.values())))
            CONTEXTS[name] = (ctx, R.ByteTables(PIECES, SCORES, TYPES, byte_pieces=bp), rules)
    return CONTEXTS[name]


def check(name, docs, max_pieces=512):
    """docs: lists of sentences. One normalize and one tokenize call over all of them."""
    import torch
    ctx, ref, rules = context(name)
    sents = [s.encode('utf-8') if isinstance(s, str) else s for d in docs for s in d]
    dev = lambda a: torch.from_numpy(a).to(ctx.device)  # noqa: E731
    text = dev(np.frombuffer(b''.join(sents), np.uint8).copy())
    so = dev(np.cumsum([0] + [len(s) for s in sents], dtype=np.int64))
    want = sents
    if rules:
        text, so = ctx.normalize(text, so)
        want = [R.normalize(rules, s) for s in sents]
        assert so.tolist() == np.cumsum([0] + [len(s) for s in want]).tolist()
        assert bytes(text.cpu().numpy()) == b''.join(want)
    if not text.numel():
        return
    ids, sl = ctx.tokenize(text, so, None, max_pieces)
    ids, sl, so = ids.cpu().numpy(), sl.cpu().numpy(), so.cpu().numpy()
    exp = ref.encode_sentences(want, max_pieces)
    assert sl.tolist() == [len(x) for x in exp]
    for i, x in enumerate(exp):
        np.testing.assert_array_equal(ids[so[i]:so[i] + len(x)], x, err_msg=repr(sents[i][:80]))


def at_offsets(*sents):
    return [[pad(k).encode() + (s.encode() if isinstance(s, str) else s) for s in sents] for k in OFFS]


NFKC = ('Ｈｅｌｌｏ\u3000ｗｏｒｌｄ ﬁne … ½ ㌀ ﷺ か\u3099 ｶﾞ a\u00a0b\u200bc\u00add \t\nx\x01\x7f '
        'Zürich 中丁 q')
CASES = {
    'three_bytes_to_one': ('hand', at_offsets('x中y 中中 a中')),
    'one_byte_to_twelve': ('hand', at_offsets('XaX XX')),
    'past_the_lds_stage': ('hand', at_offsets('ﷺ' * 40 + 'a')),
    'deletion': ('hand', at_offsets('aDb DD Da D')),
    'replaced_by_a_space': ('hand', at_offsets('Sba', 'bSa', 'baS')),
    'key_over_a_tile_edge': ('hand', at_offsets('丁丂丂a 丁 丂丁丂')),
    'greedy_from_the_left': ('hand', at_offsets('pqrstu qrstu apqrst')),
    # the boundary itself moves: `a` ends a sentence at bytes 1, 62, 63 and 64
    'no_match_over_a_sentence_end': ('hand', [[pad(k) + 'ba', 'b', 'ab'] for k in OFFS]),
    'stray_and_truncated_bytes': ('hand', at_offsets(b'a\x80b', b'ba\xe4\xb8', b'\xadb \xed\xa0\x80 \xc0\xaf')),
    'clean_tile_next_to_a_dirty_one': ('hand', at_offsets('b' * 64 + '中' * 5 + 'é' * 70 + 'a')),
    'empty_sentences': ('hand', [['', 'a', ''], [], ['', '']]),
    'entries_that_never_merge': ('swap', at_offsets('ab' * 100, 'b' + 'ab' * 100 + 'b')),
    'golden_model': ('nfkc', at_offsets(NFKC, b'a\x80b \xe4\xb8')),
    'byte_fallback': ('bytes', at_offsets('q', 'aqb', 'z中丁丁b', '丁丁', 'a' * 40 + '丁' + 'b' * 40)),
    'off_switch': ('off', at_offsets('qab qqa', 'z中丁丁b')),
}


@pytest.mark.parametrize('name', sorted(CASES))
@pytest.mark.parametrize('joined', [False, True], ids=['own_docs', 'joined'])
def test_against_the_reference(name, joined):
    table, docs = CASES[name]
    check(table, [[b''.join(s.encode() if isinstance(s, str) else s for d in docs for s in d)]] if joined else docs)


def test_edge_calls():
    import torch
    ctx, _, _ = context('hand')
    check('hand', [])  # no text, no sentence
    check('bytes', [['a丁丁b', 'q']], max_pieces=3)  # the cut falls inside a byte run
    text = torch.from_numpy(np.frombuffer('XX'.encode(), np.uint8).copy()).to(ctx.device)
    so = torch.tensor([0, 2], device=ctx.device)
    with pytest.raises(Exception, match='below the planned size'):
        ctx.normalize(text, so, out_cap=23)
    info = ctx.info()
    assert (info['rules'], info['max_key'], info['max_repl'], info['byte_fallback']) == (13, 6, 33, True)
    assert not context('off')[0].info()['byte_fallback']


def test_byte_pieces_are_continuations():
    ctx, off = context('bytes')[0], context('off')[0]
    assert off.continuation_ids() == [2, 3, 4, 5, 6]  # a, b, qa, aqq and the CJK piece
    assert ctx.continuation_ids() == [2, 3, 4, 5, 6] + BYTES.tolist()


def test_t5_loader_normalises(tmp_path):
    from lddl_amd.torch import get_t5_pretrain_data_loader
    lines = ['Ｃｈｕｎｋ number {} has words. It ﬁnds {} sentences! Does it end? Yes {}.'.format(
        i, 'many ' * (i % 5), 'and on ' * i) for i in range(12)]
    (tmp_path / '0.txt').write_text('\n'.join(lines), encoding='utf-8')
    a = get_t5_pretrain_data_loader(str(tmp_path), None, 4, 64, unigram=R.NFKC_MODEL)
    batches = list(a)
    _, ref, rules = context('nfkc')
    V = len(a.bpe)
    table, plan, n = a.plan_round(a.files)
    want = R.normalize(rules, ''.join(lines).encode())  # no rule of these lines meets a sentence end
    so, sep, po, bs = (t.cpu().numpy() for t in (table[1], plan.sent_sep, plan.piece_off, plan.block_sent))
    assert so[-1] == len(want)
    eos = a.bpe.special_ids['</s>']
    blocks = []
    for b in range(n):
        row = []
        for s in range(bs[b], bs[b + 1]):
            row += ref.encode(want[so[s]:so[s + 1]])[:po[s + 1] - po[s] - sep[s]] + [eos] * sep[s]
        blocks.append(row)
    order, got = a.order(0, 0, n), 0
    for x in batches:
        for inp, lab, ns, nt in zip(*(x[k].tolist() for k in ('input_ids', 'labels', 'src_lengths', 'tgt_lengths'))):
            inp, lab = inp[:ns - 1], lab[:nt - 1]  # without the closing </s>
            cuts = [i for i, t in enumerate(lab) if t >= V] + [len(lab)]
            noise = {lab[i]: lab[i + 1:j] for i, j in zip(cuts, cuts[1:])}
            assert [u for t in inp for u in (noise[t] if t >= V else [t])] == blocks[order[got]]
            got += 1
    assert got == n > 4
