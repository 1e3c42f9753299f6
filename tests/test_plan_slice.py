"""The time-sliced plan's host decisions (csrc/plan_split.h: whether a plan is sliced, the quantum
and the hand-off ring's size) on the CPU: tests/plan_slice_check.cpp is compiled with
AddressSanitizer + UBSan and run as a plain executable."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_plan_slice_rules(tmp_path):
    exe = str(tmp_path / 'plan_slice_check')
    cmd = ['g++', '-std=c++17', '-g', '-Wall', '-fsanitize=address,undefined',
           '-fno-sanitize-recover=undefined', '-I' + os.path.join(ROOT, 'lddl_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'plan_slice_check.cpp'), '-o', exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert 'warning' not in r.stdout, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert 'plan_slice_check ok' in r.stdout, r.stdout
