"""N-gram static masking, host surface: the `span` keyword of the pair entry points,
the CLI flag and its checks, and mask_span_native_kernel's launch shape on the CPU."""
import inspect
import os
import shutil
import subprocess

import pytest

from conftest import REPO


def test_pair_entry_points_take_span_keyword_only():
    from lddl_amd import pairs
    for fn in (pairs.make_pairs, pairs.tokenize_and_pair_chunked):
        prm = inspect.signature(fn).parameters['span']
        assert prm.default is None and prm.kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(pairs.make_pairs).parameters)[16:] == ['whole_word', 'span']


@pytest.mark.parametrize('kw,match', [
    (dict(masking=False, rng='native', span=3), 'span needs masking'),
    (dict(masking=True, rng='replay', span=3), "span needs rng='native'"),
    (dict(masking=True, rng='native', span=0), 'span'),
    (dict(masking=True, rng='native', span=[0.5, 0.4]), 'sum to'),
    (dict(masking=True, rng='native', span=17), 'span')])
def test_pair_entry_points_refuse_before_the_native_call(kw, match):
    """No context, tensor or GPU is touched: every other argument is None."""
    from lddl_amd import pairs
    with pytest.raises(ValueError, match=match):
        pairs.make_pairs(None, *(None,) * 6, **kw)
    with pytest.raises(ValueError, match=match):
        pairs.tokenize_and_pair_chunked(None, *(None,) * 5, **kw)


def test_flag_parses_and_defaults_off():
    from lddl_amd.dask.bert import pretrain as P
    ap = P.attach_args()
    assert ap.parse_args(['--sink', 'x']).ngram_masking is None
    assert ap.parse_args(['--sink', 'x', '--ngram-masking', '3']).ngram_masking == '3'
    assert P.parse_ngram_spec('3') == 3
    assert P.parse_ngram_spec('0.5, 0.25,0.25') == [0.5, 0.25, 0.25]


@pytest.mark.parametrize('extra,match', [
    (['--ngram-masking', '3'], 'needs --masking'),
    (['--ngram-masking', '3', '--masking'], 'needs --masking and --rng native'),
    (['--ngram-masking', '3', '--masking', '--rng', 'replay'], 'rng native'),
    (['--ngram-masking', '3', '--rng', 'native'], 'needs --masking'),
    (['--ngram-masking', 'three', '--masking', '--rng', 'native'], 'ngram-masking'),
    (['--ngram-masking', '17', '--masking', '--rng', 'native'], 'ngram-masking'),
    (['--ngram-masking', '0.5,0.6', '--masking', '--rng', 'native'], 'ngram-masking')])
def test_main_refuses_bad_combinations_and_specs(extra, match):
    """At the top of main, before any GPU work (this test runs without a GPU)."""
    from lddl_amd.dask.bert import pretrain as P
    with pytest.raises(ValueError, match=match):
        P.main(P.attach_args().parse_args(['--sink', '/tmp/x'] + extra))


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_native_span_shape(tmp_path):
    exe = str(tmp_path / 'native_span_shape_check')
    cmd = ['g++', '-std=c++17', '-g', '-Wall', '-fsanitize=address,undefined',
           '-fno-sanitize-recover=undefined', '-I' + os.path.join(REPO, 'lddl_amd', 'csrc'),
           os.path.join(REPO, 'tests', 'native_span_shape_check.cpp'), '-o', exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and 'warning' not in r.stdout, r.stdout
    r = subprocess.run([exe, '5', '67', '68', '128', '512', '4096'], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and 'native_span_shape_check ok' in r.stdout, r.stdout
