"""N-gram static masking in the pair planner (make_pairs(..., span=...)): every pair's
positions and labels against the numpy restatement of the definition (span_static_ref), bit for
bit, on a small corpus and on crafted id streams; the pairs themselves against the per-token run."""
import numpy as np
import pytest
import torch

import span_static_ref as ref
from test_ww_static_gpu import cont_ids, crafted, id_pools, partition_docs, restored

pytestmark = pytest.mark.gpu

SEED = 4242
SPANS = {'1': 1, '3': 3, 'onehot16': [0.0] * 15 + [1.0], 'geometric': None}  # (None: geometric())


@pytest.fixture(scope='module')
def ctx():
    from conftest import VOCAB_UNCASED
    from lddl_amd.context import Context
    return Context(VOCAB_UNCASED, True)


@pytest.fixture(scope='module')
def corpus(ctx):
    """64 KiB of synth text in partitions of 16 KiB."""
    from lddl_amd import synth
    corp = synth.generate(seed=78, n_bytes=64 << 10, nonascii_frac=0.01, threads=4)
    part = partition_docs(corp, 16 << 10)
    sent_off = torch.from_numpy(corp.sent_off).to(ctx.device)
    ids, sent_len = ctx.tokenize(torch.from_numpy(corp.text).to(ctx.device), sent_off)
    return dict(part=part, seeds=np.arange(len(part) - 1, dtype=np.int64) * 7919 + 12345,
                sent_off=sent_off, ids=ids, sent_len=sent_len,
                doc_off=torch.from_numpy(corp.doc_sent_off).to(ctx.device))


def run(ctx, b, seq, ratio, **kw):
    from lddl_amd.pairs import make_pairs
    pb = make_pairs(ctx, b['sent_off'], b['ids'], b['sent_len'], b['doc_off'],
                    torch.from_numpy(b['part']).to(ctx.device),
                    torch.from_numpy(b['seeds']).to(ctx.device), seq=seq, dup=2, masking=True,
                    masked_lm_ratio=ratio, rng='native', native_seed=SEED, **kw)
    out = pb.to_host()
    assert pb.n_masked == out['pos_off'][-1] == len(out['pos']) == len(out['labels'])
    return out


def check(ctx, b, seq, ratio, span, plain=None, paths=()):
    """The span run of `b` against the reference (which must reach `paths`) and the per-token run."""
    from lddl_amd.torch.span import geometric, parse
    span = parse(geometric() if span is None else span)
    plain = plain or run(ctx, b, seq, ratio)
    got = run(ctx, b, seq, ratio, span=span)
    for k in ('tok_off', 'len_a', 'is_random_next', 'part_off'):
        np.testing.assert_array_equal(got[k], plain[k], err_msg=k)
    orig = restored(plain)
    np.testing.assert_array_equal(restored(got), orig)
    cum = np.array(span.params(ratio).cum, np.float32)
    pos, lab, pos_off, stats = ref.expect(plain, orig, cum, SEED, b['seeds'], ctx.vocab['[CLS]'],
                                          ctx.vocab['[SEP]'], cont_ids(ctx))
    print(seq, ratio, span, len(plain['len_a']), 'pairs', stats)
    assert all(stats[k] > 0 for k in paths), stats  # the reference alone reaches them
    for k, want in (('pos_off', pos_off), ('pos', pos), ('labels', lab)):
        np.testing.assert_array_equal(got[k], want, err_msg=k)
    return got


_PLAIN = {}


@pytest.mark.parametrize('seq', [67, 68, 128, 512])
@pytest.mark.parametrize('span,ratio', [(s, 0.15) for s in SPANS] + [('3', 1.0), ('onehot16', 1.0)])
def test_corpus_matches_reference(ctx, corpus, seq, span, ratio):
    plain = _PLAIN.get((seq, ratio)) or _PLAIN.setdefault((seq, ratio), run(ctx, corpus, seq, ratio))
    assert len(plain['len_a']) > 20 and len(plain['part_off']) > 2
    got = check(ctx, corpus, seq, ratio, SPANS[span], plain)
    if span == '1':  # N = 1 is whole-word masking, in every array
        ww = run(ctx, corpus, seq, ratio, whole_word=True)
        for k in ww:
            np.testing.assert_array_equal(got[k], ww[k], err_msg=k)


def crafted_streams(ctx):
    """name -> (docs, partitions, seq, ratio, span, the paths the reference must reach)."""
    W, C = id_pools(ctx)
    rng = np.random.default_rng(9)
    w = lambda k=1: [int(x) for x in rng.choice(W, k)]  # noqa: E731
    c = lambda k: [int(x) for x in rng.choice(C, k)]  # noqa: E731
    sep = [ctx.vocab['[SEP]']]
    long_words = [[sum((w(int(rng.integers(1, 6))) + w() + c(69) for _ in range(2)), [])
                   for _ in range(5)] for _ in range(12)]
    literal = [[sum((w(2) + sep + w(3) + c(1) for _ in range(4)), []) for _ in range(5)]
               for _ in range(12)]
    one_word = [[w() + c(2), w() + c(3)] for _ in range(40)]
    cont_only = [[c(30) for _ in range(4)] for _ in range(10)]
    return {'words_of_70': (long_words, 2, 512, 0.15, 3, ('shrunk', 'shrunk_to_0', 'slot64')),
            'literal_sep': (literal, 2, 128, 0.15, 3, ('special_inside', 'overlap')),
            'one_word_a_b': (one_word, 1, 128, 1.0, [0.0, 1.0], ('ab',)),
            'continuations_only': (cont_only, 1, 128, 0.15, 3, ('below',))}


@pytest.mark.parametrize('name', ['words_of_70', 'literal_sep', 'one_word_a_b',
                                  'continuations_only'])
def test_crafted_matches_reference(ctx, name):
    docs, n_part, seq, ratio, span, paths = crafted_streams(ctx)[name]
    got = check(ctx, crafted(ctx, docs, n_part), seq, ratio, span, paths=paths)
    assert len(got['len_a']) >= 20
    if name == 'continuations_only':
        assert got['pos_off'][-1] == 0
