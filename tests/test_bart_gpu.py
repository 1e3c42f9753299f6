"""BART chunk aggregation on the GPU (csrc/bart.hip through lddl_bart_count / lddl_bart_fill over
the class table of csrc/punkt.hip, lddl_amd/bart.py) and the `preprocess_bart_pretrain` command
against the reference's output (tests/golden/bart.json, made by tests/golden/make_bart_golden.py
from the reference's own `_get_sequences` and `save`)."""
import json
import os
import random

import numpy as np
import pytest

from alloc_util import allocated, needs_torch_arena
from conftest import GOLDEN, VOCAB_UNCASED

pytestmark = pytest.mark.gpu

SPACES = [chr(cp) for cp in range(0x110000) if chr(cp).isspace()]  # the 29 of str.isspace()


@pytest.fixture(scope='module')
def ctx():
    from lddl_amd import punkt
    from lddl_amd.context import Context
    c = Context(VOCAB_UNCASED, True)
    punkt.set_params(c, None)
    return c


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(GOLDEN, 'bart.json'), encoding='utf-8') as f:
        return json.load(f)


@pytest.fixture(scope='module')
def corpus(golden, tmp_path_factory):
    """The golden input files on disk, and an (empty) Punkt parameter file: what nltk runs
    untrained, which is how the golden was made."""
    root = tmp_path_factory.mktemp('bart_corpus')
    for rel, text in golden['files'].items():
        fn = root / rel
        fn.parent.mkdir(parents=True, exist_ok=True)
        fn.write_bytes(text.encode('utf-8'))
    (root / 'punkt.json').write_text('{}')
    return root


def cli_args(corpus, sink, **kw):
    from lddl_amd.dask.bart import pretrain
    argv = ['--wikipedia', str(corpus / 'wikipedia'), '--books', str(corpus / 'books'),
            '--sink', str(sink), '--punkt-params', str(corpus / 'punkt.json'),
            '--schedule', 'local']
    for k, v in kw.items():
        # (the last character of a size is its unit, as in the reference: '3000' would be 300)
        argv += ['--' + k.replace('_', '-'), str(v) + ('b' if k == 'block_size' else '')]
    return pretrain.attach_args().parse_args(argv)


# ---- the reference's loop, on stripped sentences (lddl/dask/bart/pretrain.py:82-128) ------------

def ref_aggregate(docs, target_seq_length):
    target = target_seq_length - 3
    out = []
    for sents in docs:
        res, chunk, n = [], '', 0
        for s in filter(None, (s.strip() for s in sents)):
            chunk += ' ' + s
            n += len(s.split())
            if n >= target:
                res.append((chunk, n))
                chunk, n = '', 0
        if n > 0:
            res.append((chunk, n))
        out.append(res)
    return out


def layout(docs):
    """docs: lists of raw sentences (whitespace attached) -> text, sent_off, doc_sent_off."""
    enc = [s.encode('utf-8') for d in docs for s in d]
    text = np.frombuffer(b''.join(enc), np.uint8) if enc else np.zeros(0, np.uint8)
    sent_off = np.concatenate([[0], np.cumsum([len(e) for e in enc])]).astype(np.int64)
    dso = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    return text, sent_off, dso


def gpu_aggregate(ctx, text, sent_off, dso, tsl, shift=0):
    """bart.aggregate on host arrays -> [(chunk, num_tokens)] per document, after checking the
    layout invariants. shift: bytes in front of the text, so that it starts off a 16-byte
    boundary."""
    import torch
    from lddl_amd import bart
    buf = torch.from_numpy(np.concatenate([np.full(shift, 0x41, np.uint8), text])).cuda()
    t = buf[shift:]
    out, co, nt, dco = bart.aggregate(ctx, t, torch.from_numpy(sent_off).cuda(),
                                      torch.from_numpy(dso).cuda(), tsl)
    out, co, nt, dco = out.cpu().numpy(), co.cpu().numpy(), nt.cpu().numpy(), dco.cpu().numpy()
    assert co[0] == 0 and (np.diff(co) > 0).all() and co[-1] == len(out)
    assert dco[0] == 0 and (np.diff(dco) >= 0).all() and dco[-1] == len(co) - 1 == len(nt)
    chunks = bart.chunk_strings(out, co)
    assert [len(c.split()) for c in chunks] == nt.tolist()
    last = np.zeros(len(nt), bool)
    last[dco[1:][np.diff(dco) > 0] - 1] = True
    assert (nt[~last] >= tsl - 3).all()
    return [list(zip(chunks[dco[d]:dco[d + 1]], nt[dco[d]:dco[d + 1]].tolist()))
            for d in range(len(dco) - 1)]


def hand_docs():
    rng = random.Random(1234)
    docs = []
    for w in SPACES:  # each whitespace code point as separator, leading and trailing
        docs.append([w + 'ab' + w + 'cd' + w + w + 'é' + w, w, 'x' + w + 'y', w + w + 'z'])
    docs.append(['é ñ ü. ', '中 文 字 ', '\U0001f600 \U0001f601\u3000\U0001f602 ', 'añ中\U0001f600 b'])
    docs.append(['  ', 'first. ', '   ', '', 'second one. ', '\t', 'third', ' \u00a0'])
    docs.append(['ab', 'cd', 'e f', 'g', '中', '文 x', 'y'])  # touching sentences
    docs.append([])
    docs.append(['a', 'b', ' ', 'c', '\n', 'd'])  # 1-byte sentences
    docs.append([])
    docs.append([])
    # one sentence of ~70,000 bytes: words of 1-37 characters, 1-4 bytes each, every kind of
    # separator, so that words and separators cross every 16-byte, 64-byte and tile boundary
    parts, n = [], 0
    while n < 70_000:
        word = ''.join(rng.choice('ab.é中\U0001f600') for _ in range(rng.randint(1, 37)))
        sep = ''.join(rng.choice(SPACES) for _ in range(rng.randint(1, 3)))
        parts.append(word + sep)
        n += len((word + sep).encode('utf-8'))
    docs.append(['odd. ', ''.join(parts), 'after it. '])
    docs.append(['w{} '.format(k) for k in range(1000)])  # 1,000 one-word sentences
    docs.append([' '.join(['t'] * rng.randint(1, 9)) + '. ' for _ in range(333)])
    docs.append(['   '] * 70 + ['lone '] + ['  '] * 130 + ['pair of '] + [' '] * 5)
    docs.append([])
    docs.append(['last doc'])
    return docs


HAND_TARGETS = [3, 2, 0, 4, 7, 11, 35, 130, 2003]  # thresholds 0, -1, -3, 1, 4, 8, 32, 127, 2000


@pytest.fixture(scope='module')
def hand():
    docs = hand_docs()
    return docs, layout(docs)


@pytest.mark.parametrize('tsl', HAND_TARGETS)
def test_hand_built_layouts(ctx, hand, tsl):
    docs, (text, so, dso) = hand
    got = gpu_aggregate(ctx, text, so, dso, tsl)
    exp = ref_aggregate(docs, tsl)
    bad = [d for d in range(len(docs)) if got[d] != exp[d]]
    assert not bad, (bad[:5], got[bad[0]][:3], exp[bad[0]][:3])


def test_thousand_sentence_document_targets(ctx):
    """1,000 one-word sentences: 250 chunks of 4 words at threshold 4, and one chunk that spans
    sixteen 64-sentence steps at threshold 2,000."""
    docs = [['w{} '.format(k) for k in range(1000)]]
    text, so, dso = layout(docs)
    got4 = gpu_aggregate(ctx, text, so, dso, 7)
    assert got4 == ref_aggregate(docs, 7) and len(got4[0]) == 250
    got = gpu_aggregate(ctx, text, so, dso, 2003)
    assert got == ref_aggregate(docs, 2003) and len(got[0]) == 1 and got[0][0][1] == 1000


def test_unaligned_text_and_no_documents(ctx, hand):
    """Text that starts off a 16-byte boundary takes the shifted tiling; n_doc = 0 and documents
    without sentences give empty tables."""
    import torch
    from lddl_amd import bart
    docs, (text, so, dso) = hand
    for shift in (1, 7):
        assert gpu_aggregate(ctx, text, so, dso, 11, shift=shift) == ref_aggregate(docs, 11)
    z = np.zeros(1, np.int64)
    assert gpu_aggregate(ctx, np.zeros(0, np.uint8), z, z, 128) == []
    assert gpu_aggregate(ctx, np.zeros(0, np.uint8), z, np.zeros(4, np.int64), 128) == [[], [], []]
    assert gpu_aggregate(ctx, np.frombuffer(b' \t ', np.uint8), np.asarray([0, 2, 3], np.int64),
                         np.asarray([0, 1, 2], np.int64), 128) == [[], []]
    with pytest.raises(ValueError):
        bart.aggregate(ctx, torch.zeros(4, dtype=torch.uint8).cuda(),
                       torch.tensor([0, 3, 2]).cuda(), torch.tensor([0, 2]).cuda(), 128)


def test_past_two_gib(ctx):
    """Offsets into text and output past 2**31: 2,200,000 sentences of 1,000 bytes, each 125
    words 'aaaaaaa '. Every sentence becomes ' ' + its 999 stripped bytes, so the output is the text
    moved right by one byte."""
    import torch
    from lddl_amd import bart
    n_sent, per = 2_200_000, 1000
    text = torch.full((n_sent * per,), 0x61, dtype=torch.uint8, device='cuda')
    text[7::8] = 0x20
    so = torch.arange(n_sent + 1, dtype=torch.int64, device='cuda') * per
    dso = torch.arange(0, n_sent + 1, 100, dtype=torch.int64, device='cuda')
    out, co, nt, dco = bart.aggregate(ctx, text, so, dso, 128)
    assert out.numel() == n_sent * per > 1 << 31
    assert int(out[0]) == 0x20 and torch.equal(out[1:], text[:-1])
    assert torch.equal(co, so) and bool((nt == 125).all()) and nt.numel() == n_sent
    assert torch.equal(dco, dso)
    out2, co2, nt2, _ = bart.aggregate(ctx, text, so, dso, 3 + 250 * 100)  # one chunk per document
    assert torch.equal(out2, out) and torch.equal(co2, so[::100]) and bool((nt2 == 12500).all())


# ---- golden parity ---------------------------------------------------------------------------

@pytest.fixture(scope='module')
def segmented(ctx, golden, corpus):
    """Per block size: the partitions' lines (whole stripped lines are the articles) through
    punkt.segment, once; every target aggregates the same tensors."""
    import torch
    from lddl_amd import punkt
    from lddl_amd.dask import readers
    from lddl_amd.dask.bart import pretrain
    out = {}
    for bs in sorted({c['block_size'] for c in golden['cases']}):
        blocks = pretrain.plan_partitions(cli_args(corpus, corpus / 'unused', block_size=bs))
        parts = [readers.read_block(b, as_bytes=True) for b in blocks]
        lines = [x for p in parts for x in p]
        text = torch.from_numpy(np.frombuffer(b''.join(lines), np.uint8).copy()).cuda()
        doc_off = np.concatenate([[0], np.cumsum([len(x) for x in lines])]).astype(np.int64)
        so, dso = punkt.segment(ctx, text, torch.from_numpy(doc_off).cuda())
        pdo = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
        out[bs] = (text, so, dso, pdo)
    return out


def test_golden_has_the_cases(golden):
    assert sorted({c['target_seq_length'] for c in golden['cases']}) == [3, 11, 35, 128, 512]
    assert len({c['block_size'] for c in golden['cases']}) == 2 and len(golden['cases']) == 10
    import re
    assert max(len(re.split(r'[.?!]\s', line)) for t in golden['files'].values()
               for line in t.split('\n')) > 200  # the long article


@pytest.mark.parametrize('case', range(10))
def test_golden_parity(ctx, golden, segmented, case):
    from lddl_amd import bart
    c = golden['cases'][case]
    text, so, dso, pdo = segmented[c['block_size']]
    out, co, nt, dco = bart.aggregate(ctx, text, so, dso, c['target_seq_length'])
    per_doc = bart.chunk_strings(out.cpu().numpy(), co.cpu().numpy(), dco.cpu().numpy())
    got = [[s for d in per_doc[pdo[p]:pdo[p + 1]] for s in d] for p in range(len(pdo) - 1)]
    assert len(got) == len(c['partitions'])
    bad = [p for p in range(len(got)) if got[p] != c['partitions'][p]]
    assert not bad, (bad, got[bad[0]][:2], c['partitions'][bad[0]][:2])
    assert (nt.cpu().numpy() == [len(s.split()) for p in got for s in p]).all()


# ---- allocator balance ---------------------------------------------------------------------

@needs_torch_arena
def test_bart_blocks_balance(ctx, hand):
    """The pending aggregation's blocks come from torch's allocator at lddl_bart_count and go
    back at lddl_bart_fill, whether it fills the outputs or cancels (null outputs)."""
    import ctypes
    import torch
    from lddl_amd import bart
    from lddl_amd._native import check, lib
    from lddl_amd.context import _ptr, _stream
    docs, (text, so, dso) = hand
    t, s, d = (torch.from_numpy(x).cuda() for x in (text, so, dso))
    before = allocated()
    res = bart.aggregate(ctx, t, s, d, 11)
    n_exp = res[1].numel() - 1
    del res
    assert allocated() == before
    n_chunks, n_out = ctypes.c_int64(), ctypes.c_int64()
    check(lib.lddl_bart_count(ctx._h, _stream(), _ptr(t), t.numel(), _ptr(s), s.numel() - 1,
                              _ptr(d), d.numel() - 1, 8, ctypes.byref(n_chunks),
                              ctypes.byref(n_out)))
    assert n_chunks.value == n_exp and allocated() > before
    assert lib.lddl_bart_count(ctx._h, _stream(), _ptr(t), t.numel(), _ptr(s), s.numel() - 1,
                               _ptr(d), d.numel() - 1, 8, ctypes.byref(n_chunks),
                               ctypes.byref(n_out)) < 0  # one fill per count
    check(lib.lddl_bart_fill(ctx._h, _stream(), None, None, None, None))
    assert allocated() == before
    assert lib.lddl_bart_fill(ctx._h, _stream(), None, None, None, None) < 0  # nothing pending
    res = bart.aggregate(ctx, t, s, d, 11)  # the context aggregates again after the cancel
    assert res[1].numel() - 1 == n_exp


def test_needs_punkt_tables():
    import ctypes
    import torch
    from lddl_amd._native import NativeError, check, lib
    from lddl_amd.context import Context, _ptr, _stream
    c = Context(VOCAB_UNCASED, True)  # lddl_punkt_set_params never called
    z = torch.zeros(2, dtype=torch.int64).cuda()
    a, b = ctypes.c_int64(), ctypes.c_int64()
    with pytest.raises(NativeError, match='lddl_punkt_set_params'):
        check(lib.lddl_bart_count(c._h, _stream(), _ptr(z), 0, _ptr(z), 0, _ptr(z), 0, 5,
                                  ctypes.byref(a), ctypes.byref(b)))
    c.close()


# ---- the command, in process ---------------------------------------------------------------

@pytest.mark.parametrize('case', range(10))
def test_cli_txt_is_byte_identical(golden, corpus, tmp_path, case):
    from lddl_amd.dask.bart import pretrain
    c = golden['cases'][case]
    pretrain.main(cli_args(corpus, tmp_path / 'out', output_format='txt',
                           target_seq_length=c['target_seq_length'], block_size=c['block_size']))
    assert sorted(os.listdir(tmp_path / 'out')) == sorted(c['txt'])
    for fn, exp in c['txt'].items():
        assert (tmp_path / 'out' / fn).read_bytes() == exp.encode('utf-8'), fn


@pytest.mark.parametrize('case,batch_bytes', [(1, 512 << 20), (3, 1500), (8, 30000)])
def test_cli_parquet(golden, corpus, tmp_path, case, batch_bytes):
    """1,500 bytes per GPU batch is one partition of the 1,000-byte blocks at a time."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from lddl_amd.dask.bart import pretrain
    c = golden['cases'][case]
    pretrain.main(cli_args(corpus, tmp_path / 'out', target_seq_length=c['target_seq_length'],
                           block_size=c['block_size'], gpu_batch_bytes=batch_bytes))
    assert sorted(os.listdir(tmp_path / 'out')) == c['parquet_files']
    for p, rows in enumerate(c['partitions']):
        t = pq.read_table(str(tmp_path / 'out' / 'part.{}.parquet'.format(p)))
        assert t.schema.names == ['sentences'] and t.schema.types == [pa.string()]
        assert t.column('sentences').to_pylist() == rows, p
    md = pq.read_metadata(str(tmp_path / 'out' / '_metadata'))
    assert md.num_rows == sum(len(r) for r in c['partitions'])


def test_cli_invalid_utf8(tmp_path):
    from lddl_amd.dask.bart import pretrain
    src = tmp_path / 'books'
    src.mkdir()
    (src / 'a.txt').write_bytes(b'b-0 A fine line. Another.\nb-1 A broken \xff byte. Here.\n')
    (tmp_path / 'punkt.json').write_text('{}')
    args = pretrain.attach_args().parse_args(['--books', str(src), '--sink', str(tmp_path / 'o'),
                                              '--punkt-params', str(tmp_path / 'punkt.json')])
    with pytest.raises(UnicodeDecodeError):
        pretrain.main(args)


# ---- the context's state: unset tables, a pending aggregation, a closed context --------------

def small_layout():
    """Two documents of three short sentences, as lddl_segment_fill lays them out."""
    import torch
    docs = [['One two. ', 'Three four five. ', 'Six. '], ['Seven eight nine. ', 'Ten. ', 'Eleven twelve.']]
    text, so, dso = layout(docs)
    return docs, tuple(torch.from_numpy(x.copy()).cuda() for x in (text, so, dso))


def raw_bart_count(c, t, s, d, target_words):
    import ctypes
    from lddl_amd._native import lib
    from lddl_amd.context import _ptr, _stream
    n_chunks, n_out = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = lib.lddl_bart_count(c._h, _stream(), _ptr(t), t.numel(), _ptr(s), s.numel() - 1, _ptr(d),
                             d.numel() - 1, target_words, ctypes.byref(n_chunks), ctypes.byref(n_out))
    return rc, n_chunks.value, n_out.value


def small_chunks(out, co, nt, dco):
    from lddl_amd import bart
    chunks = bart.chunk_strings(out.cpu().numpy(), co.cpu().numpy())
    dco, nt = dco.cpu().numpy(), nt.cpu().numpy().tolist()
    return [list(zip(chunks[dco[k]:dco[k + 1]], nt[dco[k]:dco[k + 1]])) for k in range(len(dco) - 1)]


def test_count_needs_set_params_then_works():
    from lddl_amd import bart, punkt
    from lddl_amd._native import lib
    from lddl_amd.context import Context
    docs, (t, s, d) = small_layout()
    c = Context(VOCAB_UNCASED, True)  # lddl_punkt_set_params never called
    rc, _, _ = raw_bart_count(c, t, s, d, 4)
    assert rc == -1
    assert lib.lddl_last_error().decode() == ('Punkt parameters not set (lddl_punkt_set_params): '
                                              'lddl_bart_count needs the character classes')
    punkt.set_params(c, None)
    assert small_chunks(*bart.aggregate(c, t, s, d, 7)) == ref_aggregate(docs, 7)
    c.close()


def test_second_count_is_refused_and_the_fill_returns_the_first(ctx):
    import torch
    from lddl_amd._native import check, lib
    from lddl_amd.context import _ptr, _stream
    docs, (t, s, d) = small_layout()
    rc, n_chunks, n_out = raw_bart_count(ctx, t, s, d, 4)  # target_seq_length 7
    assert rc == 0
    rc2, _, _ = raw_bart_count(ctx, t, s, d, 1)  # (one chunk per sentence, were it counted)
    assert rc2 == -1
    assert lib.lddl_last_error().decode() == 'an aggregation is pending: call lddl_bart_fill first'
    out = torch.empty(n_out, dtype=torch.uint8, device='cuda')
    co = torch.empty(n_chunks + 1, dtype=torch.int64, device='cuda')
    nt = torch.empty(n_chunks, dtype=torch.int32, device='cuda')
    dco = torch.empty(d.numel(), dtype=torch.int64, device='cuda')
    check(lib.lddl_bart_fill(ctx._h, _stream(), _ptr(out), _ptr(co), _ptr(nt), _ptr(dco)))
    assert small_chunks(out, co, nt, dco) == ref_aggregate(docs, 7)


@needs_torch_arena
def test_closing_the_context_returns_a_pending_aggregation():
    from lddl_amd import punkt
    from lddl_amd.context import Context
    _, (t, s, d) = small_layout()
    c = Context(VOCAB_UNCASED, True)
    punkt.set_params(c, None)
    before = allocated()
    rc, n_chunks, _ = raw_bart_count(c, t, s, d, 4)
    assert rc == 0 and n_chunks >= 2 and allocated() > before
    c.close()  # between count and fill
    assert allocated() == before
