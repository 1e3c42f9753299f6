"""BART denoising, host side (no GPU): lddl_denoise_params_make against a numpy
bisection, the refusals of the two entry points, and the argument errors of `bart_denoise` and
`get_bart_pretrain_data_loader`, raised before the GPU is touched."""
import ctypes
import os

import numpy as np
import pytest

from conftest import REPO
from lddl_amd.torch import denoise as D  # ImportError without the feature
from denoise_oracle import solve_p_start

VOCAB = os.path.join(REPO, 'lddl_amd', 'assets', 'vocab_synth_uncased_30522.txt')
WEIGHTS = {'poisson3': D.poisson_weights(3.0), 'onehot1': [0, 1], 'onehot16': [0] * 16 + [1],
           'half_zero': [2, 1, 1]}


def _make(ratio, weights, n=None):
    from lddl_amd._native import DenoiseParams, lib
    dp = DenoiseParams()
    w = None if weights is None else (ctypes.c_double * len(weights))(*weights)
    n = len(weights) - 1 if n is None else n
    return lib.lddl_denoise_params_make(ratio, n, w, ctypes.byref(dp)), dp


@pytest.mark.parametrize('name', list(WEIGHTS))
@pytest.mark.parametrize('ratio', [0.3, 0.05])
def test_p_start_matches_a_numpy_bisection(name, ratio):
    w = np.asarray(WEIGHTS[name], np.float64)
    st, dp = _make(ratio, list(w))
    assert st == 0 and dp.n == len(w) - 1 and ctypes.sizeof(dp) == 4 + 4 + 4 * 16
    want = solve_p_start(ratio, w)
    # the cast of the double solution: half a float32 ulp, and the two bisections' last bits
    assert abs(float(dp.p_start) - want) <= np.spacing(np.float32(want)) * 0.5 + 1e-12
    cum = np.cumsum(w / w.sum())
    assert list(dp.cum)[:dp.n] == [float(np.float32(min(c, 1.0))) for c in cum[:-1]]
    assert all(c == 1.0 for c in list(dp.cum)[dp.n:])


def test_defaults_and_the_ends_of_the_range():
    a, b = _make(0.3, None, 10)[1], _make(0.3, WEIGHTS['poisson3'])[1]
    assert a.n == b.n == 10 and a.p_start == b.p_start and list(a.cum) == list(b.cum)
    w = WEIGHTS['half_zero']  # q = (0.5, 0.25): p_start = 1 reaches 1 - 0.5 * 0.75
    assert _make(0.0, w)[1].p_start == 0.0 and _make(0.625, w)[1].p_start == 1.0
    assert _make(0.626, w)[0] == -1
    assert _make(0.0, [1, 0])[0] == 0 and _make(0.01, [1, 0])[0] == -1  # only insertions


def test_bad_params_are_refused():
    from lddl_amd._native import lib
    ok = WEIGHTS['poisson3']
    for ratio, w, n in [(0.3, None, 0), (0.3, None, 17), (0.3, [0.5, -0.1, 0.6], None),
                        (0.3, [0.0, 0.0], None), (0.3, [float('nan'), 1.0], None),
                        (0.3, [float('inf'), 1.0], None), (-0.01, ok, None), (1.01, ok, None),
                        (float('nan'), ok, None)]:
        assert _make(ratio, w, n)[0] == -1 and lib.lddl_last_error(), (ratio, w, n)
    assert lib.lddl_denoise_params_make(0.3, 10, None, None) == -1


def test_entry_point_refuses_values_before_it_needs_a_context():
    from lddl_amd._native import DenoiseParams, lib
    good = _make(0.3, None, 10)[1]

    def call(params=good, L=16, stride=16, perm=1.0, rnd=0.1, vocab=30522):
        p = None if params is None else ctypes.cast(ctypes.pointer(params), ctypes.c_void_p)
        st = lib.lddl_bart_denoise(None, None, None, None, None, None, None, 4, L, None, None,
                                   None, None, None, 1, 2, 0, 3, 2, -100, vocab, 7, 0, stride,
                                   perm, rnd, p)
        return st, lib.lddl_last_error().decode()
    assert call() == (-1, 'null ctx')  # every value passed
    bad = [DenoiseParams(), DenoiseParams(), DenoiseParams(), DenoiseParams()]
    for dp, (n, p, c0, c_last) in zip(bad, [(0, .5, 1, 1), (3, 1.5, 1, 1), (3, .5, .9, 1),
                                            (3, .5, 1, .5)]):
        dp.n, dp.p_start = n, p
        dp.cum[:] = [c0, 0.5] + [1.0] * 13 + [c_last]  # falling, or not 1 past n
    for kw in [dict(params=None)] + [dict(params=dp) for dp in bad] + [
            dict(L=1), dict(L=(1 << 24) + 1, stride=1 << 25), dict(stride=15), dict(perm=1.5),
            dict(perm=float('nan')), dict(rnd=-0.1), dict(vocab=0)]:
        st, msg = call(**kw)
        assert st == -1 and msg != 'null ctx', (kw, msg)


@pytest.fixture
def no_gpu(monkeypatch):
    import lddl_amd.context as C

    def boom(*a, **k):
        raise AssertionError('the GPU was touched')
    monkeypatch.setattr(C.Context, '__init__', boom)


@pytest.mark.parametrize('kw', [
    dict(mask=0.3), dict(mask=(1.5, 0, 0)), dict(permute_sentence_ratio=-0.1),
    dict(random_ratio=2), dict(poisson_lambda=0), dict(span_weights=[1.0]),
    dict(span_weights=[0.1] * 18), dict(span_weights=[0, 0]), dict(span_weights=[1, -1]),
    dict(span_weights='ab'), dict(sequence_length_alignment=0), dict(seq_len=1)])
def test_helper_refuses_bad_arguments_before_the_gpu(no_gpu, kw):
    with pytest.raises(ValueError):
        D.bart_denoise(None, None, None, None, None, **kw)


def test_loader_refuses_bad_arguments_before_the_gpu(no_gpu, tmp_path):
    from lddl_amd.torch import get_bart_pretrain_data_loader as make
    with pytest.raises(FileNotFoundError, match='shards'):
        make(str(tmp_path), VOCAB, 4)
    for i in (10, 9):
        (tmp_path / '{}.txt'.format(i)).write_text('A chunk. Of two sentences.')
    with pytest.raises(FileNotFoundError):
        make(str(tmp_path), str(tmp_path / 'vocab.txt'), 4)
    for kw in (dict(batch_size=0), dict(batch_size=4, max_seq_length=1),
               dict(batch_size=4, mask_ratio=1.2), dict(batch_size=4, rank=0),
               dict(batch_size=4, rank=2, world=2), dict(batch_size=4, round_bytes=0),
               dict(batch_size=4, span_weights=[0, 0]), dict(batch_size=4, special_ids={'bos': 1})):
        with pytest.raises(ValueError):
            make(str(tmp_path), VOCAB, **kw)
    loader = make(str(tmp_path), VOCAB, 4)
    assert [os.path.basename(f) for f in loader.files] == ['9.txt', '10.txt']
    assert loader.format == 'txt'
