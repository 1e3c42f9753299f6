"""SentencePiece unigram on the GPU: lddl_unigram_tokenize through `UnigramContext`,
ids and sent_len bit for bit against the sequential reference (unigram_ref.py, which
test_unigram_host.py ties to sentencepiece) at the shapes where the kernels take another path;
the T5 loader with unigram=."""
import numpy as np
import pytest

import unigram_ref
from lddl_amd import unigram as U  # ImportError without the feature

pytestmark = pytest.mark.gpu
M = '▁'
A16 = ['a' * k for k in range(1, 17)]
TABLES = {  # name: (pieces, scores); piece 0 is <unk>
    'nest': (['<unk>', M] + A16, [0, -1] + [-1 - 0.37 * k for k in range(16)]),
    'tie': (['<unk>', M, 'a', 'b', 'c', 'ab', 'bc'], [0, -1, -1, -5, -1, -2, -2]),
    # float32: -16777216 + -1 rounds back to -16777216, a tie that the earlier start wins;
    # float64 would prefer the other path by 1
    'f32': (['<unk>', M, M + 'x', 'yz', M + 'xy', 'z'], [0, -1, -16777216, -1, -16777215, -1]),
    'unk': (['<unk>', M, 'a', 'b', 'qa', 'aqq', '中'], [0, -2, -1, -1, -30, -3, -2]),
    'bare': (['<unk>', M, 'a', 'b', 'c', 'ab'], [0, -1, -1, -1, -1, -1.5]),
}
CONTEXTS = {}


def context(name, ascii_ws=False):
    key = (name, ascii_ws)
    if key not in CONTEXTS:
        if name == 'synth':
            p, s, t, unk, _ = U.load_model(unigram_ref.SYNTH_MODEL)
            CONTEXTS[key] = (U.UnigramContext.from_tables(p, s, t, unk, ascii_ws),
                             unigram_ref.Tables(p, s, t, unk, ascii_ws))
        else:
            CONTEXTS[key] = (U.UnigramContext.from_tables(*TABLES[name], ascii_ws=ascii_ws),
                             unigram_ref.Tables(*TABLES[name], ascii_ws=ascii_ws))
    return CONTEXTS[key]


def check(name, docs, max_pieces=512, with_docs=True, ascii_ws=False):
    """docs: lists of sentences (str or bytes). Tokenizes them in one call and compares every
    sentence's ids and sent_len with the reference."""
    import torch
    ctx, ref = context(name, ascii_ws)
    sents = [s.encode('utf-8') if isinstance(s, str) else s for d in docs for s in d]
    so = np.zeros(len(sents) + 1, np.int64)
    np.cumsum([len(s) for s in sents], out=so[1:])
    dso = np.zeros(len(docs) + 1, np.int64)
    np.cumsum([len(d) for d in docs], out=dso[1:])
    dev = lambda a: torch.from_numpy(a).to(ctx.device)  # noqa: E731
    ids, sl = ctx.tokenize(dev(np.frombuffer(b''.join(sents) or b' ', np.uint8).copy()), dev(so),
                           dev(dso) if with_docs else None, max_pieces)
    ids, sl = ids.cpu().numpy(), sl.cpu().numpy()
    want = ref.encode_sentences(sents, max_pieces)
    np.testing.assert_array_equal(sl, [len(x) for x in want])
    for i, x in enumerate(want):
        np.testing.assert_array_equal(ids[so[i]:so[i] + len(x)], x, err_msg=repr(sents[i][:80]))
    return want


def word(n):  # n bytes of letters the synthetic vocabulary cuts into several pieces
    return ('thequickbrownfoxjumpsoverthelazydog' * 40)[:n]


def pad(k):  # k bytes of one-letter words: the text behind it starts at tile offset k % 64
    return ('a ' * 64)[:k]


SLICE = 'ab' * 511 + 'aézz'  # 1,027 bytes; byte 1,024 is inside the e-acute: cut at 1,023
CASES = {
    'lengths_at_offset_0': ('synth', [[word(n) + ' ' + word(3)] for n in (1, 61, 62, 64, 65, 200)]),
    'lengths_at_offset_60': ('synth', [[pad(60) + word(n) + ' x'] for n in (1, 4, 5, 61, 64, 65, 200)]),
    'lengths_at_offset_63': ('synth', [[pad(63) + word(n), 'x' + word(n)] for n in (1, 2, 62, 64, 65)]),
    'slices': ('synth', [[word(1025) + ' ' + SLICE], [pad(63) + SLICE + ' ' + word(2049)]]),
    'character_over_a_tile_edge': ('synth', [[pad(k) + 'x中éy\U0001F601 z'] for k in (60, 61, 62, 63)]),
    'sixteen_nested': ('nest', [['a' * n for n in (1, 15, 16, 17, 33, 70)] + [pad(50) + 'a' * 40]]),
    'tie_goes_to_the_earlier_start': ('tie', [['abc', 'abc abcabc', 'cab bca']]),
    'float32_not_float64': ('f32', [['xyz', ' xyz xyz']]),
    'unknown': ('unk', [['q', 'qqq', 'aqb', 'qa', 'qab qqa', 'aqq', 'aqqq', 'z中丁丁b', '丁']]),
    'stray_and_truncated_bytes': ('unk', [[b'a\x80b', b'\x80', b'a\xe4\xb8', b'\xe4\xb8\xada\xe4 \xb8\xad',
                                         b'\xc0a \xf5', b'q\xbf\xbf\xbf\xbfq']]),
    'sentence_first_words_and_spaces': ('synth', [['the fox', ' the fox', 'the', 'fox', '  the   fox  ', '', ' ', '    ']]),
    'more_pieces_than_bytes': ('bare', [['a b c', 'a', 'ab c a']]),
    'empty_input_sentences': ('bare', [['', ''], [], ['']]),
}


@pytest.mark.parametrize('name', sorted(CASES))
@pytest.mark.parametrize('with_docs', [True, False], ids=['docs', 'no_docs'])
def test_against_the_reference(name, with_docs):
    table, docs = CASES[name]
    check(table, docs, with_docs=with_docs)
    check(table, [[s for d in docs for s in d]], with_docs=with_docs)  # other tile offsets


@pytest.mark.parametrize('ascii_ws', [False, True])
def test_tab_is_a_space_only_with_ascii_ws(ascii_ws):
    want = check('bare', [['ab\tab  ', 'ab\n\rc\x0c ', '\t']], ascii_ws=ascii_ws)
    assert (0 in want[0]) == (not ascii_ws)  # the tab is an unknown character of one word


@pytest.mark.parametrize('max_pieces', [1, 7])
def test_max_pieces(max_pieces):
    check('synth', [['the quick brown fox ' * 6, '', 'a'], [word(200)]], max_pieces)


def test_word_stats_count_the_second_window_and_the_long_list():
    import torch
    ctx = context('synth')[0]
    sents = [pad(60) + word(5) + ' ' + word(3), pad(57) + word(70) + ' ', word(64), word(65) + ' a']
    text = ''.join(sents).encode()
    spans, pos = [], 0
    for s in sents:  # ASCII; a word ends with its sentence
        for w in s.split(' '):
            spans += [(pos, len(w))] if w else []
            pos += len(w) + 1
        pos -= 1
    cross = [n for x, n in spans if x // 64 != (x + n - 1) // 64]
    dev = lambda a: torch.from_numpy(np.asarray(a, np.int64)).to(ctx.device)  # noqa: E731
    got = ctx.word_stats(torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(ctx.device),
                         dev(np.cumsum([0] + [len(s) for s in sents])))
    assert got.tolist() == [len(spans), sum(n <= 64 for n in cross), sum(n > 64 for n in cross)]
    assert sum(n <= 64 for n in cross) >= 2 and sum(n > 64 for n in cross) >= 2


def test_t5_loader_with_unigram(tmp_path):
    from lddl_amd.torch import get_t5_pretrain_data_loader, t5_lengths
    lines = ['Chunk number {} has words. It has {} sentences! Does it end? Yes {}.'.format(
        i, 'many ' * (i % 5), 'and on ' * i) for i in range(12)]
    for k in range(3):
        (tmp_path / '{}.txt'.format(k)).write_text('\n'.join(lines[k::3]))
    a = get_t5_pretrain_data_loader(str(tmp_path), None, 4, 64, unigram=unigram_ref.SYNTH_MODEL)
    batches = list(a)
    ref, V = context('synth')[1], len(a.bpe)
    table, plan, n = a.plan_round(a.files)
    text = ''.join(s for k in range(3) for s in lines[k::3]).encode()
    so, sep, po, bs = (t.cpu().numpy() for t in (table[1], plan.sent_sep, plan.piece_off, plan.block_sent))
    eos = a.bpe.special_ids['</s>']
    blocks = []
    for b in range(n):
        row = []
        for s in range(bs[b], bs[b + 1]):
            keep = po[s + 1] - po[s] - sep[s]
            row += ref.encode(text[so[s]:so[s + 1]])[:keep] + [eos] * sep[s]
        blocks.append(row)
    order, got = a.order(0, 0, n), 0
    for x in batches:
        assert (x['input_ids'].shape[1], x['labels'].shape[1]) == t5_lengths(plan.seq_len - 2)
        for inp, lab, ns, nt in zip(*(x[k].tolist() for k in ('input_ids', 'labels', 'src_lengths', 'tgt_lengths'))):
            inp, lab = inp[:ns - 1], lab[:nt - 1]  # without the closing </s>
            assert all(t < V or V <= t < V + 100 for t in inp + lab)
            cuts = [i for i, t in enumerate(lab) if t >= V] + [len(lab)]
            noise = {lab[i]: lab[i + 1:j] for i, j in zip(cuts, cuts[1:])}
            row = [u for t in inp for u in (noise[t] if t >= V else [t])]
            assert row == blocks[order[got]]
            got += 1
    assert got == n > 4
