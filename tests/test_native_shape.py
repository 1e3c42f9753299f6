"""The native planner's launch shapes (csrc/native_shape.h: the walk tables' LDS words and the
grid, block and LDS size of the two mask kernels) on the CPU: tests/native_shape_check.cpp is
compiled with AddressSanitizer + UBSan and run as a plain executable."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_native_shape_rules(tmp_path):
    exe = str(tmp_path / 'native_shape_check')
    cmd = ['g++', '-std=c++17', '-g', '-Wall', '-fsanitize=address,undefined',
           '-fno-sanitize-recover=undefined', '-I' + os.path.join(ROOT, 'lddl_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'native_shape_check.cpp'), '-o', exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert 'warning' not in r.stdout, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert 'native_shape_check ok' in r.stdout, r.stdout
