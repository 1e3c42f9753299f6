"""The arena's block owners (csrc/arena.h: ArenaScope, ArenaTmp) on the CPU: tests/arena_check.cpp
is compiled with AddressSanitizer + UBSan and run as a plain executable over a counting
malloc-backed allocator. It exits non-zero unless every block was freed exactly once."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get('ROCM_PATH', '/opt/rocm')


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
@pytest.mark.skipif(not os.path.exists(os.path.join(ROCM, 'include', 'hip', 'hip_runtime_api.h')),
                    reason='needs the ROCm headers')
def test_arena_owners_free_every_block_once(tmp_path):
    exe = str(tmp_path / 'arena_check')
    cmd = ['g++', '-std=c++17', '-g', '-Wall', '-fsanitize=address,undefined',
           '-fno-sanitize-recover=undefined', '-D__HIP_PLATFORM_AMD__',
           '-I' + os.path.join(ROCM, 'include'), '-I' + os.path.join(ROOT, 'lddl_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'arena_check.cpp'), '-o', exe,
           '-L' + os.path.join(ROCM, 'lib'), '-lamdhip64', '-Wl,-rpath,' + os.path.join(ROCM, 'lib'),
           '-lpthread']
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert 'warning' not in r.stdout, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert 'arena_check ok' in r.stdout, r.stdout
