"""Host side of the BART preprocessor (lddl_amd/dask/bart/pretrain.py): the command line against
the reference's parser (tests/golden/bart.json, made by tests/golden/make_bart_golden.py), the
whitespace class the kernels use, and the writers' framing of the device buffers."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import ASSETS, GOLDEN, REPO


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(GOLDEN, 'bart.json'), encoding='utf-8') as f:
        return json.load(f)


def test_attach_args_match_reference(golden):
    from lddl_amd.dask.bart import pretrain
    acts = {a.option_strings[0]: a for a in pretrain.attach_args()._actions
            if a.option_strings and a.dest != 'help'}
    assert len(golden['args']) == 14
    for opt, ref in golden['args'].items():
        assert opt in acts, opt
        a = acts[opt]
        default = os.cpu_count() if ref['default'] == 'os.cpu_count()' else ref['default']
        assert a.dest == ref['dest'] and a.default == default, opt
        assert bool(a.required) == ref['required'], opt
        assert (None if a.choices is None else list(a.choices)) == ref['choices'], opt
    # what lddl_amd adds, as in the BERT command
    assert set(acts) - set(golden['args']) == {'--gpu-batch-bytes', '--read-threads',
                                               '--write-threads', '--punkt-params'}
    ns = pretrain.attach_args().parse_args(['--sink', 'x', '--block-size', '2K'])
    assert ns.block_size == 2048 and ns.open_webtext is None


def test_space_class_is_str_isspace():
    """Bit 0 of the Punkt class table is what str.strip() / str.split() call whitespace."""
    t = np.fromfile(os.path.join(ASSETS, 'punkt_props.bin'), np.uint8)
    _, n_pages, _ = struct.unpack('<III', bytes(t[4:16]))
    l1 = t[16:16 + 0x2200].view(np.uint16).astype(np.int64)
    pages = t[16 + 0x2200:16 + 0x2200 + 256 * n_pages]
    cps = np.arange(0x110000, dtype=np.int64)
    bit = pages[l1[cps >> 8] * 256 + (cps & 255)] & 1
    space = [cp for cp in range(0x110000) if chr(cp).isspace()]
    assert len(space) == 29
    exp = np.zeros(0x110000, np.uint8)
    exp[space] = 1
    keep = (cps < 0xD800) | (cps > 0xDFFF)
    assert np.array_equal(bit[keep], exp[keep])
    # the kernels look a code point up only when its UTF-8 form starts with C2, E1, E2 or E3
    assert {chr(cp).encode('utf-8')[0] for cp in space if cp >= 128} <= {0xC2, 0xE1, 0xE2, 0xE3}
    assert max(len(chr(cp).encode('utf-8')) for cp in space) == 3
    # the ASCII members are the kernels' bit mask
    assert [cp for cp in space if cp < 128] == [c for c in range(64) if (0x00000001F0003E00 >> c) & 1]


def test_module_help_without_gpu():
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, '-m', 'lddl_amd.dask.bart.pretrain', '--help'], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=REPO)
    assert r.returncode == 0, r.stderr
    assert '--target-seq-length' in r.stdout and '--open-webtext' in r.stdout


def test_plan_matches_reference_partitions(golden, tmp_path):
    """The planned blocks are the reference's partitions: as many as it produced, and empty where
    its partition holds no chunk for want of a line."""
    import argparse
    from lddl_amd.dask import readers
    from lddl_amd.dask.bart import pretrain
    for rel, text in golden['files'].items():
        fn = tmp_path / rel
        fn.parent.mkdir(parents=True, exist_ok=True)
        fn.write_bytes(text.encode('utf-8'))
    for bs in sorted({c['block_size'] for c in golden['cases']}):
        case = next(c for c in golden['cases'] if c['block_size'] == bs)
        args = argparse.Namespace(wikipedia=str(tmp_path / 'wikipedia'), wikipedia_lang='en',
                                  books=str(tmp_path / 'books'), common_crawl=None,
                                  open_webtext=None, block_size=bs, num_blocks=None)
        blocks = pretrain.plan_partitions(args)
        assert len(blocks) == len(case['partitions'])
        lines = [readers.read_block(b, as_bytes=True) for b in blocks]
        assert [not ls for ls in lines] == [not p for p in case['partitions']]
    assert any(not p for c in golden['cases'] for p in c['partitions'])  # an empty partition


def test_string_column_and_txt_framing(tmp_path):
    """The Arrow column is built over the buffers (chunked when the bytes pass the limit of one
    array) and the text file joins the rows with newlines, none after the last."""
    import pyarrow as pa
    from lddl_amd.dask.bart import pretrain
    rows = [' a b', ' ccc', ' \u3000d', ' e' * 10, ' f']
    enc = [r.encode('utf-8') for r in rows]
    data = np.frombuffer(b'pad' + b''.join(enc), np.uint8)
    off = np.concatenate([[3], 3 + np.cumsum([len(e) for e in enc])]).astype(np.int64)
    col = pretrain.string_column(data, off, 0, len(rows))
    assert col.type == pa.string() and col.num_chunks == 1 and col.to_pylist() == rows
    col = pretrain.string_column(data, off, 1, 5, limit=9)  # forces several arrays
    assert col.num_chunks > 1 and col.to_pylist() == rows[1:]
    assert pretrain.string_column(data, off, 2, 2).to_pylist() == []
    for r0, r1 in ((0, 5), (1, 2), (3, 3)):
        fn = pretrain.write_txt_part(str(tmp_path / 'x.txt'), data, off, r0, r1)
        with open(fn, 'rb') as f:
            assert f.read().decode('utf-8') == '\n'.join(rows[r0:r1])
    fn = pretrain.write_parquet_part(str(tmp_path / 'p.parquet'), data, off, 0, 5)
    import pyarrow.parquet as pq
    t = pq.read_table(fn)
    assert t.schema.names == ['sentences'] and t.schema.types == [pa.string()]
    assert t.column('sentences').to_pylist() == rows
