"""The split plan's host decisions (csrc/plan_split.h: where the planner's partitions are cut, the
output capacities predicted from the head range, and which mode a replay plan runs in:
plan_replay_mode) on the CPU: tests/plan_split_check.cpp is
compiled with AddressSanitizer + UBSan and run as a plain executable."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_plan_split_rules(tmp_path):
    exe = str(tmp_path / 'plan_split_check')
    cmd = ['g++', '-std=c++17', '-g', '-Wall', '-fsanitize=address,undefined',
           '-fno-sanitize-recover=undefined', '-I' + os.path.join(ROOT, 'lddl_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'plan_split_check.cpp'), '-o', exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert 'warning' not in r.stdout, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert 'plan_split_check ok' in r.stdout, r.stdout
