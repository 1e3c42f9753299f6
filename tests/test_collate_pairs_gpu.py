"""collate_pairs (lddl_collate_pairs / lddl_collate_pairs_masked) against the string path, bit
for bit: the same pairs rendered to the reference's strings (output.render) and collated by
_to_encoded_inputs / encode_packed must give the same tensors, every key."""
import numpy as np
import pytest
import torch

from conftest import VOCAB_UNCASED

pytestmark = pytest.mark.gpu

LONG = 'pneumonoultramicroscopicsilicovolcanoconiosisxqzvantidisestablishmentarianismzzq'
HAND = [
    # literal special tokens and an emoji ([UNK])
    ['The token [MASK] stands in the text as it is.', 'So do [CLS] and [UNK] and [SEP] here.',
     'An emoji \U0001F600 maps to nothing the vocab knows.', 'The end of it.'],
    # 60 one-piece words, then a word of many pieces: as A / B it lies across slot 64
    [' '.join(['the'] * 60) + '.', LONG + ' ' + LONG + ' and then some more words follow.',
     'Short one.', LONG + ' again ' + LONG + '.'],
    [LONG + ' ' + LONG + ' ' + LONG + '.', 'B begins here ' + LONG + '.', 'And one more.'],
]
SEED, COUNTER = 0x1234_5678_9ABC, (3 << 32) | 7


def _table(ctx, corp, seq, masking, nparts=3, dup=2):
    from lddl_amd.pairs import make_pairs
    so = torch.from_numpy(corp.sent_off).cuda()
    ids, sl = ctx.tokenize(torch.from_numpy(corp.text).cuda(), so)
    part = np.linspace(0, corp.n_doc, nparts + 1).astype(np.int64)
    return make_pairs(ctx, so, ids, sl, torch.from_numpy(corp.doc_sent_off).cuda(),
                      torch.from_numpy(part).cuda(), torch.arange(21, 21 + nparts).cuda(), seq=seq,
                      dup=dup, masking=masking, rng='replay')


@pytest.fixture(scope='module')
def ctx():
    from lddl_amd.context import Context
    return Context(VOCAB_UNCASED)


@pytest.fixture(scope='module')
def tables(ctx):
    """{(seq, masking): (PairBatch, its host copy)} over ~300 KB of synthetic text with the
    hand-written documents in the middle; made once, never changed."""
    from lddl_amd import synth
    docs = synth.generate(seed=314, n_bytes=300_000, nonascii_frac=0.02, threads=4).documents()
    half = len(docs) // 2
    corp = synth.from_documents(docs[:half] + HAND + docs[half:])
    out = {}
    for seq in (128, 512):
        for masking in (False, True):
            pb = _table(ctx, corp, seq, masking)
            out[seq, masking] = (pb, pb.to_host())
    return out


def _tuples(ctx, pb, rows):
    """The reference's samples of output rows `rows`: (A, B, is_random_next[, positions,
    labels]) as the parquet shards hold them."""
    from lddl_amd import output
    rd = output.render(ctx, pb, rows)
    out = []
    for r in range(rd.n):
        d = rd.row(r)
        t = (d['A'], d['B'], d['is_random_next'])
        if pb.pos is not None:
            t += (d['masked_lm_positions'], d['masked_lm_labels'])
        out.append(t)
    return out


def _same(got, ref):
    assert set(got) == set(ref)
    for k in ref:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        assert torch.equal(got[k], ref[k]), k


def _check_plain(ctx, pb, rows, align=8):
    from lddl_amd.torch.bert import _to_encoded_inputs
    from lddl_amd.torch.online import collate_pairs
    ref = _to_encoded_inputs(_tuples(ctx, pb, rows), ctx, sequence_length_alignment=align,
                             ignore_index=-1)
    got = collate_pairs(ctx, pb, rows, sequence_length_alignment=align, ignore_index=-1)
    _same(got, ref)
    assert 'labels' in got if pb.pos is not None else 'special_tokens_mask' in got
    # with the width passed in and the checks off (the loader's call): the same
    _same(collate_pairs(ctx, pb, rows, align, -1, seq_len=ref['input_ids'].shape[1], check=False),
          ref)
    return ref


def _check_masked(ctx, pb, rows, p, ww, ignore=-1):
    from lddl_amd.torch.bert import encode_packed
    from lddl_amd.torch.online import collate_pairs
    from lddl_amd.torch.packing import PackedBatch
    ref = encode_packed(PackedBatch(_tuples(ctx, pb, rows)), ctx, 8, ignore,
                        mask=(p, SEED, COUNTER), whole_word=ww)
    got = collate_pairs(ctx, pb, rows, 8, ignore, mask=(p, SEED, COUNTER), whole_word=ww)
    _same(got, ref)
    return ref


def _rows(idx):
    return torch.tensor(list(idx), dtype=torch.int64, device='cuda')


def _mixed_rows(h, n, rng):
    """n rows (n >= 3): the shortest and the longest pair, a repeated index, the rest random,
    in a random order."""
    nt = h['num_tokens']
    idx = [int(nt.argmin()), int(nt.argmax())]
    idx += [int(x) for x in rng.integers(0, len(nt), max(n - 3, 0))]
    idx.append(idx[-1])
    idx = idx[:n]
    rng.shuffle(idx)
    return idx


@pytest.mark.parametrize('seq', [128, 512])
@pytest.mark.parametrize('masking', [False, True])
@pytest.mark.parametrize('B', [1, 5, 9])
def test_plain_and_static_equal_the_string_path(ctx, tables, seq, masking, B):
    pb, h = tables[seq, masking]
    rng = np.random.default_rng(seq + B)
    idx = [int(h['num_tokens'].argmax())] if B == 1 else _mixed_rows(h, B, rng)
    ref = _check_plain(ctx, pb, _rows(idx))
    if B > 1:  # the longest pair of a seq-S table fills the row: L == S exactly
        assert ref['input_ids'].shape == (B, seq)
        assert int(ref['attention_mask'][idx.index(int(h['num_tokens'].argmax()))].sum()) == seq
    if masking:
        assert int((ref['labels'] != -1).sum()) > 0


@pytest.mark.parametrize('masking', [False, True])
def test_widths_72_and_unaligned_and_identity_rows(ctx, tables, masking):
    """L = 72 (not a multiple of the wave), a width that is no multiple of 8 (alignment 1), and
    rows=None over a small table of its own (the identity)."""
    from lddl_amd.balance import HipOps, _gather_table
    pb, h = tables[128, masking]
    nt = h['num_tokens']
    top = np.flatnonzero((nt > 64) & (nt <= 72))
    assert len(top), 'the corpus has no pair of 65..72 tokens'
    low = np.flatnonzero(nt <= 64)[:6]
    idx = [int(top[0])] + [int(x) for x in low]
    ref = _check_plain(ctx, pb, _rows(idx))
    assert ref['input_ids'].shape[1] == 72
    odd = np.flatnonzero(nt % 8 == 3)
    ref = _check_plain(ctx, pb, _rows([int(odd[0])] * 2), align=1)
    assert ref['input_ids'].shape[1] == int(nt[odd[0]])
    small = _gather_table(HipOps(ctx), pb, None, _rows(idx))
    _same(_check_plain(ctx, small, None), _check_plain(ctx, pb, _rows(idx)))


def test_width_8_from_a_two_sentence_document(ctx):
    from lddl_amd import synth
    corp = synth.from_documents([['It is.', 'To.']])  # 3 + 2 pieces, 8 with the specials
    for masking in (False, True):
        pb = _table(ctx, corp, 128, masking, nparts=1, dup=3)
        assert pb.n_pairs >= 1 and int(pb.num_tokens.max()) <= 8, pb.num_tokens
        ref = _check_plain(ctx, pb, None)
        assert ref['input_ids'].shape[1] == 8
        if not masking:
            for ww in (False, True):
                _check_masked(ctx, pb, None, 0.5, ww)


def _ww_rows(ctx, h):
    """Rows in which whole-word masking has something to get wrong: a continuation piece at slot
    64 (a word across the 64-slot window), and a B that begins with a continuation piece."""
    cont = np.array([t.startswith('##') and len(t) > 2 for t in ctx.tokens])
    tok, off, na = h['tokens'].astype(np.int64), h['tok_off'], h['len_a'].astype(np.int64)
    straddle, b_cont = [], []
    for q in range(len(na)):
        n = off[q + 1] - off[q]
        for x in (64,):  # slot 64 = A token 63, or B token 62 - na... as the kernel lays it out
            k = x - 1 if x <= na[q] else x - 2
            if x != na[q] + 1 and x - 1 != na[q] + 1 and x - 1 >= 1 and k < n and \
                    cont[tok[off[q] + k]]:
                straddle.append(q)
        if na[q] < n and cont[tok[off[q] + na[q]]]:
            b_cont.append(q)
    return straddle, b_cont


@pytest.mark.parametrize('seq', [128, 512])
@pytest.mark.parametrize('p', [0.0, 0.15, 1.0])
@pytest.mark.parametrize('ww', [False, True])
def test_dynamic_masking_equals_the_string_path(ctx, tables, seq, p, ww):
    pb, h = tables[seq, False]
    straddle, b_cont = _ww_rows(ctx, h)
    assert straddle, 'no word lies across slot 64'
    rng = np.random.default_rng(seq)
    idx = _mixed_rows(h, 6, rng) + straddle[:2] + b_cont[:1]
    ref = _check_masked(ctx, pb, _rows(idx), p, ww)
    masked = ref['labels'] != -1
    if p == 0.0:
        assert not masked.any()
    if p == 1.0:  # every real token, no special slot
        assert int(masked.sum()) == int(sum(h['num_tokens'][i] - 3 for i in idx))
    for B in (1, 5):  # the waves-per-block count from both sides, another ignore_index
        _check_masked(ctx, pb, _rows(idx[:B]), p, ww, ignore=-100)


def test_whole_word_differs_from_plain_where_words_have_pieces(ctx, tables):
    """The whole-word rule is live: on rows with continuation pieces the two modes differ, and
    a masked continuation's head is masked."""
    from lddl_amd.torch.online import collate_pairs
    pb, h = tables[128, False]
    straddle, _ = _ww_rows(ctx, h)
    rows = _rows(straddle[:9])
    a = collate_pairs(ctx, pb, rows, mask=(0.15, SEED, COUNTER), whole_word=False)
    b = collate_pairs(ctx, pb, rows, mask=(0.15, SEED, COUNTER), whole_word=True)
    assert not torch.equal(a['labels'], b['labels'])
    for k in ('token_type_ids', 'attention_mask', 'next_sentence_labels'):
        assert torch.equal(a[k], b[k])


def test_hand_made_window_edges_equal_the_string_path(ctx):
    """test_online_seqpack_gpu.edge_samples (a [SEP] on slot 63 and on slot 64, '##' pieces that
    begin A and B, the smallest pair) as a table of its own against the string path, in every
    mode. The ids are ASCII words and pieces: each string is one vocab line, so the rendered
    sample splits and looks up to the ids it came from."""
    from test_online_seqpack_gpu import _pair_batch, _with_static, edge_samples
    toks = ctx.tokens
    words = np.array([i for i in range(1000, 6000) if toks[i].isascii() and toks[i].isalpha()])
    cont = np.array([i for i, t in enumerate(toks)
                     if t.startswith('##') and t.isascii() and t[2:].isalnum()][:500])
    assert len(words) > 1000 and len(cont) == 500
    rng = np.random.default_rng(11)
    samples, _ = edge_samples(rng, words, cont)
    pb = _pair_batch(ctx, samples)
    assert _check_plain(ctx, pb, None)['input_ids'].shape == (5, 72)
    for ww in (False, True):
        _check_masked(ctx, pb, None, 0.5, ww)
    at = [[1, 62, 64, 68], [1, 63, 65], [1, 62], [63], [1, 3]]
    _check_plain(ctx, _pair_batch(ctx, [_with_static(rng, words, s, p)
                                        for s, p in zip(samples, at)]), None)


def test_four_byte_ids(tmp_path):
    """A vocab of more than 65,534 lines: 4-byte ids in the table (lddl_ctx_id_bytes)."""
    from lddl_amd import synth
    from lddl_amd.context import Context
    with open(VOCAB_UNCASED) as f:
        lines = f.read().splitlines()
    big = tmp_path / 'vocab_big.txt'
    big.write_text('\n'.join(lines + ['[extra{}]'.format(i) for i in range(40000)]) + '\n')
    wide = Context(str(big))
    assert wide.id_bytes == 4
    docs = synth.generate(seed=27, n_bytes=80_000, threads=2).documents()
    corp = synth.from_documents(docs + HAND)
    for masking in (False, True):
        pb = _table(wide, corp, 128, masking)
        assert pb.tokens.dtype == torch.int32
        h = pb.to_host()
        idx = _mixed_rows(h, 9, np.random.default_rng(4))
        _check_plain(wide, pb, _rows(idx))
        if not masking:
            for ww in (False, True):
                ref = _check_masked(wide, pb, _rows(idx), 0.5, ww)
                # random replacement ids come from the whole vocab, above 65,535 too
                assert int(ref['input_ids'].max()) < len(wide)
    narrow = Context(VOCAB_UNCASED)
    with pytest.raises(ValueError, match='4-byte'):
        from lddl_amd.torch.online import collate_pairs
        collate_pairs(narrow, pb)


def test_host_checks(ctx, tables):
    from lddl_amd.pairs import PairBatch
    from lddl_amd.torch.online import collate_pairs
    pb, h = tables[128, True]
    nt = h['num_tokens']
    q = int(np.flatnonzero((nt > 16) & (np.diff(h['pos_off']) > 0))[0])
    L = (int(nt[q]) - 1) // 8 * 8 + 8
    rows = _rows([q])
    with pytest.raises(ValueError, match='does not fit'):  # a pair longer than seq_len
        collate_pairs(ctx, pb, rows, seq_len=8)
    with pytest.raises(IndexError, match='the table has'):
        collate_pairs(ctx, pb, _rows([0, pb.n_pairs]))
    with pytest.raises(IndexError, match='the table has'):
        collate_pairs(ctx, pb, _rows([-1]))
    bad = PairBatch(pb.tokens, pb.tok_off, pb.len_a, pb.is_random_next, pb.pos.clone(),
                    pb.labels, pb.pos_off)
    bad.pos[int(h['pos_off'][q + 1]) - 1] = L  # the row's last position, now past the row
    with pytest.raises(IndexError, match='masked_lm_positions'):
        collate_pairs(ctx, bad, rows)
    collate_pairs(ctx, bad, _rows([q + 1 if q + 1 < pb.n_pairs else q - 1]))  # other rows: fine
    # an empty batch: empty tensors of the asked width
    for table in (pb, tables[128, False][0]):
        e = collate_pairs(ctx, table, _rows([]), seq_len=16)
        assert e['input_ids'].shape == (0, 16) and e['next_sentence_labels'].shape == (0,)
        e = collate_pairs(ctx, table, _rows([]), mask=(0.15, 1, 2))
        assert e['input_ids'].shape[0] == 0 and ('labels' in e)


def test_abi_refusals(ctx, tables):
    """-1 before anything is launched: NULL context, NULL required output, static inputs in
    part; batch <= 0 returns 0."""
    from lddl_amd._native import lib
    from lddl_amd.context import _ptr, _stream
    pb, _ = tables[128, True]
    o = [torch.full((2, 16), 77, dtype=torch.long, device='cuda') for _ in range(4)]
    nsl = torch.zeros(2, dtype=torch.long, device='cuda')
    tab = (_ptr(pb.tokens), _ptr(pb.tok_off), _ptr(pb.len_a), _ptr(pb.is_random_next))
    st = (_ptr(pb.pos), _ptr(pb.labels), _ptr(pb.pos_off))
    outs = (_ptr(o[0]), _ptr(o[1]), _ptr(o[2]))

    def plain(c, static, stm, lab, n=2, first=outs[0]):
        return lib.lddl_collate_pairs(c, _stream(), *tab, *static, None, n, 16, first, outs[1],
                                      outs[2], stm, lab, _ptr(nsl), -1)
    assert plain(None, st, None, _ptr(o[3])) == -1
    assert b'null ctx' in lib.lddl_last_error()
    assert plain(ctx.handle, st, None, None) == -1                       # static: labels missing
    assert plain(ctx.handle, (None, None, None), None, _ptr(o[3])) == -1  # no special_tokens_mask
    assert plain(ctx.handle, (st[0], None, st[2]), None, _ptr(o[3])) == -1
    assert plain(ctx.handle, st, None, _ptr(o[3]), first=None) == -1
    assert plain(ctx.handle, st, None, _ptr(o[3]), n=0) == 0

    def masked(c, lab, n=2):
        return lib.lddl_collate_pairs_masked(c, _stream(), *tab, None, n, 16, *outs, lab,
                                             _ptr(nsl), 0.15, -1, len(ctx), 1, 2, 0)
    assert masked(None, _ptr(o[3])) == -1
    assert masked(ctx.handle, None) == -1
    assert masked(ctx.handle, _ptr(o[3]), n=-3) == 0
    torch.cuda.synchronize()
    assert all(int((t != 77).sum()) == 0 for t in o)  # nothing was launched
