"""GPU Punkt segmentation parity (csrc/segment.hip through lddl_segment_count/_fill, with the
tables of csrc/punkt.hip) against nltk's spans (tests/golden/punkt.npz) and the oracle, the
segmented path end to end (segment -> tokenize -> NSP pairs + static masking) against the
oracle, and the context's Punkt state: unset, pending, replaced, closed."""
import json
import os

import numpy as np
import pytest

from alloc_util import allocated, needs_torch_arena
from conftest import GOLDEN, VOCAB_UNCASED

pytestmark = pytest.mark.gpu


def reference_sentences(text, doc_off, st, en, cnt):
    """sent_tokenize + strip + drop empty (pretrain.py:86-88) from (nltk / oracle) spans."""
    out, k = [], 0
    for d in range(len(doc_off) - 1):
        b0 = int(doc_off[d])
        ss = [bytes(text[b0 + st[j]:b0 + en[j]]).decode('utf-8').strip()
              for j in range(k, k + int(cnt[d]))]
        out.append([s for s in ss if s])
        k += int(cnt[d])
    return out


@pytest.fixture(scope='module')
def ctx():
    from lddl_amd.context import Context
    return Context(VOCAB_UNCASED, True)


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(GOLDEN, 'punkt.npz')) as z:
        g = dict(z)
    with open(os.path.join(GOLDEN, 'punkt_params.json')) as f:
        g['params'] = json.load(f)
    return g


def gpu_sentences(ctx, text, doc_off, params=None):
    import torch
    from lddl_amd import punkt
    punkt.set_params(ctx, punkt.PunktParams.from_dict(params) if params else None)
    t = torch.from_numpy(np.ascontiguousarray(text)).cuda()
    do = torch.from_numpy(np.ascontiguousarray(doc_off, np.int64)).cuda()
    so, ds = punkt.segment(ctx, t, do)
    so, ds = so.cpu().numpy(), ds.cpu().numpy()
    # layout invariants: contiguous, monotone, covering the batch, 1+ sentence per document
    assert so[0] == doc_off[0] and so[-1] == doc_off[-1]
    assert (np.diff(so) >= 0).all()
    assert np.array_equal(so[ds[:-1]], doc_off[:-1])
    assert (np.diff(ds) >= 1).all()
    return punkt.stripped_sentences(text, so, ds)


@pytest.mark.parametrize('name', ['untrained', 'trained'])
def test_segment_matches_nltk(ctx, golden, name):
    prm = golden['params'] if name == 'trained' else None
    got = gpu_sentences(ctx, golden['text'], golden['doc_off'], prm)
    exp = reference_sentences(golden['text'], golden['doc_off'], golden[name + '_start'],
                              golden[name + '_end'], golden[name + '_count'])
    assert len(got) == len(exp)
    bad = [d for d in range(len(exp)) if got[d] != exp[d]]
    assert not bad, (len(bad), bad[:5], [(got[d], exp[d]) for d in bad[:2]])


def test_segment_synthetic_vs_oracle(ctx):
    from lddl_amd import synth
    from oracle import oracle as O
    text, doc_off = synth.generate_doc_text(seed=31, n_bytes=8 << 20, nonascii_frac=0.05, threads=8)
    got = gpu_sentences(ctx, text, doc_off)
    st, en, cnt = O.Punkt().spans(text, doc_off)
    assert got == reference_sentences(text, doc_off, st, en, cnt)


def test_segment_dense_enders_vs_oracle(ctx):
    """Runs of sentence enders (every byte a qualified ender: "?!?!?! x") and long runs that
    cross the 4-KB slab and the 64-byte context windows; documents back to back, so a write
    outside a document's candidate slots would corrupt its neighbour."""
    from oracle import oracle as O
    import random
    rng = random.Random(5)
    docs = ['?!' * 40 + ' x', '?' * 301 + ' Y', '.!?' * 50 + ') Z. ' + '!' * 7, 'a.)' * 100,
            ('word' * 300 + '. Next. ') * 3, '"' * 70 + 'x.' + ')' * 70 + ' Y',
            ' '.join('w{}?!'.format(i) for i in range(700)), 'x' * 5000 + '. A ' + 'b' * 4500 + '.']
    docs += [''.join(rng.choice('?!.) "ab') for _ in range(rng.randint(1, 200))) for _ in range(300)]
    enc = [d.encode() for d in docs]
    doc_off = np.concatenate([[0], np.cumsum([len(e) for e in enc])]).astype(np.int64)
    text = np.frombuffer(b''.join(enc), np.uint8)
    got = gpu_sentences(ctx, text, doc_off)
    st, en, cnt = O.Punkt().spans(text, doc_off)
    exp = reference_sentences(text, doc_off, st, en, cnt)
    bad = [d for d in range(len(exp)) if got[d] != exp[d]]
    assert not bad, (bad[:5], [(got[d][:3], exp[d][:3]) for d in bad[:2]])


def test_segment_empty_and_whitespace_documents(ctx):
    docs = ['', '   ', 'One. Two.', '　', 'x', 'End.) ', '']
    enc = [d.encode() for d in docs]
    doc_off = np.concatenate([[0], np.cumsum([len(e) for e in enc])]).astype(np.int64)
    text = np.frombuffer(b''.join(enc), np.uint8)
    got = gpu_sentences(ctx, text, doc_off)
    assert got == [[], [], ['One.', 'Two.'], [], ['x'], ['End.)'], []]


def test_segmented_path_end_to_end(ctx):
    """GPU segment -> tokenize -> pairs (whitespace kept between sentences) equals the oracle
    on the reference's stripped sentences."""
    import torch
    from lddl_amd import punkt, synth
    from lddl_amd.pairs import make_pairs
    from oracle import oracle as O
    text, doc_off = synth.generate_doc_text(seed=77, n_bytes=1 << 20, nonascii_frac=0.05, threads=8)
    punkt.set_params(ctx, None)
    t = torch.from_numpy(text).cuda()
    so, ds = punkt.segment(ctx, t, torch.from_numpy(doc_off).cuda())
    ids, sl = ctx.tokenize(t, so)
    n_doc = len(doc_off) - 1
    part = np.asarray([0, n_doc // 3, n_doc], np.int64)
    seeds = np.asarray([5, 6], np.int64)
    pb = make_pairs(ctx, so, ids, sl, ds, torch.from_numpy(part).cuda(),
                    torch.from_numpy(seeds).cuda(), seq=128, dup=2, masking=True).to_host()
    # oracle: nltk-equivalent spans -> stripped sentences -> compact corpus -> tokenize -> pairs
    st, en, cnt = O.Punkt().spans(text, doc_off)
    docs = reference_sentences(text, doc_off, st, en, cnt)
    corp = synth.from_documents(docs)
    tok = O.Tokenizer(VOCAB_UNCASED)
    e_ids, e_off = tok.tokenize(corp.text, corp.sent_off)
    lens = np.diff(e_off)
    keep = lens > 0
    k_off = np.concatenate([[0], np.cumsum(lens[keep])])
    kept_pos = np.concatenate([[0], np.cumsum(keep)])
    ds_h = np.concatenate([[0], np.cumsum([len(d) for d in docs])])
    toks, nts = [], []
    for p in range(2):
        kd = kept_pos[ds_h[part[p]:part[p + 1] + 1]]
        kd = np.concatenate([kd[:1], kd[1:][np.diff(kd) > 0]])
        out = O.partition_pairs(kd, k_off, e_ids, int(seeds[p]), 2, 128, True, tok.vocab_size,
                                *(tok.token_id(x) for x in ('[CLS]', '[SEP]', '[MASK]')))
        toks.append(out['tokens'])
        nts.append(out['num_tokens'])
    np.testing.assert_array_equal(pb['num_tokens'], np.concatenate(nts))
    np.testing.assert_array_equal(pb['tokens'], np.concatenate(toks))


@needs_torch_arena
def test_segment_blocks_balance(ctx, golden):
    """The pending segmentation's blocks come from torch's allocator at lddl_segment_count and go
    back at lddl_segment_fill, whether it fills the outputs or cancels (null outputs)."""
    import ctypes
    import torch
    from lddl_amd import punkt
    from lddl_amd._native import check, lib
    from lddl_amd.context import _ptr, _stream
    punkt.set_params(ctx, None)
    text = torch.from_numpy(np.ascontiguousarray(golden['text'])).cuda()
    doc_off = torch.from_numpy(np.ascontiguousarray(golden['doc_off'], np.int64)).cuda()
    before = allocated()
    so, ds = punkt.segment(ctx, text, doc_off)
    exp = so.numel() - 1
    assert exp >= int(golden['untrained_count'].sum())  # (an empty document still has one span)
    del so, ds
    assert allocated() == before
    n_sent = ctypes.c_int64()
    check(lib.lddl_segment_count(ctx._h, _stream(), _ptr(text), text.numel(), _ptr(doc_off),
                                 doc_off.numel() - 1, ctypes.byref(n_sent)))
    assert n_sent.value == exp and allocated() > before
    check(lib.lddl_segment_fill(ctx._h, _stream(), None, None))
    assert allocated() == before
    so, ds = punkt.segment(ctx, text, doc_off)  # the context segments again after the cancel
    assert so.numel() - 1 == exp


# ---- the context's Punkt state: unset, pending, replaced, closed -----------------------------

SMALL_DOCS = ['Dr. Who came in. He sat down. Then he left.',
              'It was e.g. a test. Mr. J. Smith spoke. The end.']


def small_corpus():
    """Two documents of three short sentences whose cuts the golden parameters change ('dr',
    'e.g' and 'mr' are abbreviations there)."""
    import torch
    enc = [d.encode() for d in SMALL_DOCS]
    doc_off = np.concatenate([[0], np.cumsum([len(e) for e in enc])]).astype(np.int64)
    text = np.frombuffer(b''.join(enc), np.uint8)
    return text, doc_off, torch.from_numpy(text.copy()).cuda(), torch.from_numpy(doc_off).cuda()


def oracle_sentences(text, doc_off, params=None):
    from oracle import oracle as O
    st, en, cnt = O.Punkt(params).spans(text, doc_off)
    return reference_sentences(text, doc_off, st, en, cnt)


def raw_count(c, t, do):
    """lddl_segment_count itself (punkt.segment sets the parameters when none were set)."""
    import ctypes
    from lddl_amd._native import lib
    from lddl_amd.context import _ptr, _stream
    n = ctypes.c_int64(-1)
    rc = lib.lddl_segment_count(c._h, _stream(), _ptr(t), t.numel(), _ptr(do), do.numel() - 1,
                                ctypes.byref(n))
    return rc, n.value


def test_count_needs_set_params_then_works():
    from lddl_amd._native import lib
    from lddl_amd.context import Context
    text, doc_off, t, do = small_corpus()
    c = Context(VOCAB_UNCASED, True)  # lddl_punkt_set_params never called
    rc, _ = raw_count(c, t, do)
    assert rc == -1
    assert lib.lddl_last_error().decode() == 'Punkt parameters not set (lddl_punkt_set_params)'
    assert gpu_sentences(c, text, doc_off) == oracle_sentences(text, doc_off)
    c.close()


def test_second_count_is_refused_and_the_fill_returns_the_first(ctx):
    import torch
    from lddl_amd import punkt
    from lddl_amd._native import check, lib
    from lddl_amd.context import _ptr, _stream
    text, doc_off, t, do = small_corpus()
    punkt.set_params(ctx, None)
    rc, n_sent = raw_count(ctx, t, do)
    assert rc == 0
    # another batch: were it counted, the fill below would write its offsets
    other = torch.from_numpy(np.frombuffer(b'One. Two. Three. Four. Five.', np.uint8).copy()).cuda()
    rc2, _ = raw_count(ctx, other, torch.tensor([0, other.numel()]).cuda())
    assert rc2 == -1
    assert lib.lddl_last_error().decode() == 'a segmentation is pending: call lddl_segment_fill first'
    so = torch.empty(n_sent + 1, dtype=torch.int64, device='cuda')
    ds = torch.empty(do.numel(), dtype=torch.int64, device='cuda')
    check(lib.lddl_segment_fill(ctx._h, _stream(), _ptr(so), _ptr(ds)))
    assert punkt.stripped_sentences(text, so.cpu().numpy(), ds.cpu().numpy()) == \
        oracle_sentences(text, doc_off)
    assert lib.lddl_segment_fill(ctx._h, _stream(), _ptr(so), _ptr(ds)) == -1  # nothing pending
    assert lib.lddl_last_error().decode() == 'no pending segmentation (lddl_segment_count)'


def test_set_params_replaces_the_tables(ctx, golden):
    """Trained parameters, then none: the tables of the first call are gone."""
    text, doc_off, _, _ = small_corpus()
    trained = gpu_sentences(ctx, text, doc_off, golden['params'])
    assert trained == oracle_sentences(text, doc_off, golden['params'])
    untrained = gpu_sentences(ctx, text, doc_off)
    assert untrained == oracle_sentences(text, doc_off) and untrained != trained
    got = gpu_sentences(ctx, golden['text'], golden['doc_off'])
    assert got == reference_sentences(golden['text'], golden['doc_off'], golden['untrained_start'],
                                      golden['untrained_end'], golden['untrained_count'])


@needs_torch_arena
def test_closing_the_context_returns_a_pending_segmentation(golden):
    from lddl_amd import punkt
    from lddl_amd.context import Context
    _, _, t, do = small_corpus()
    c = Context(VOCAB_UNCASED, True)
    punkt.set_params(c, punkt.PunktParams.from_dict(golden['params']))
    before = allocated()
    rc, n_sent = raw_count(c, t, do)
    assert rc == 0 and n_sent >= 2 and allocated() > before
    c.close()  # between count and fill
    assert allocated() == before
