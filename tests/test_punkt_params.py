"""The host side of lddl_punkt_set_params (csrc/punkt_params.h: the class table's validation, the
parameter records' parser and its open-addressing table, every refusal and its message) on the
CPU: tests/punkt_params_check.cpp is compiled together with csrc/errors.cpp with AddressSanitizer
+ UBSan and run as a plain executable on the shipped table and the golden parameters' records."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ASSETS, GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_punkt_param_parser(tmp_path):
    from lddl_amd.punkt import PunktParams
    exe = str(tmp_path / 'punkt_params_check')
    csrc = os.path.join(ROOT, 'lddl_amd', 'csrc')
    # errors.cpp includes the generated build_id.h: the tree's when it was built, else this one
    (tmp_path / 'build_id.h').write_text('#pragma once\n#define LDDL_BUILD_ID "punkt_params_check"\n')
    cmd = ['g++', '-std=c++17', '-g', '-Wall', '-fsanitize=address,undefined',
           '-fno-sanitize-recover=undefined', '-I' + csrc, '-I' + os.path.join(ROOT, 'include'),
           '-I' + str(tmp_path), os.path.join(ROOT, 'tests', 'punkt_params_check.cpp'),
           os.path.join(csrc, 'errors.cpp'), '-o', exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert 'warning' not in r.stdout, r.stdout
    with open(os.path.join(GOLDEN, 'punkt_params.json')) as f:
        records = PunktParams.from_dict(json.load(f)).records()
    assert records
    (tmp_path / 'records.bin').write_bytes(records)
    r = subprocess.run([exe, os.path.join(ASSETS, 'punkt_props.bin'), str(tmp_path / 'records.bin')],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert 'punkt_params_check ok' in r.stdout, r.stdout
