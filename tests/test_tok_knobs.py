"""The tokenizer's environment knobs (csrc/tok_knobs.h: accepted values, rejected values and their
messages, and the word memo's sample size) on the CPU: tests/tok_knobs_check.cpp is compiled
together with csrc/errors.cpp with AddressSanitizer + UBSan and run as a plain executable."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_tok_knob_rules(tmp_path):
    exe = str(tmp_path / 'tok_knobs_check')
    csrc = os.path.join(ROOT, 'lddl_amd', 'csrc')
    # errors.cpp includes the generated build_id.h: the tree's when it was built, else this one
    (tmp_path / 'build_id.h').write_text('#pragma once\n#define LDDL_BUILD_ID "tok_knobs_check"\n')
    cmd = ['g++', '-std=c++17', '-g', '-Wall', '-fsanitize=address,undefined',
           '-fno-sanitize-recover=undefined', '-I' + csrc, '-I' + os.path.join(ROOT, 'include'),
           '-I' + str(tmp_path), os.path.join(ROOT, 'tests', 'tok_knobs_check.cpp'),
           os.path.join(csrc, 'errors.cpp'), '-o', exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert 'warning' not in r.stdout, r.stdout
    env = {k: v for k, v in os.environ.items() if not k.startswith('LDDL_')}
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120,
                       env=env)
    assert r.returncode == 0, r.stdout
    assert 'tok_knobs_check ok' in r.stdout, r.stdout
