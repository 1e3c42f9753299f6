"""bench.py host logic (no GPU): the --gpus N launcher and the CPU-baseline core grant."""
import os
import subprocess
import sys

import pytest

from conftest import REPO

sys.path.insert(0, REPO)
import bench  # noqa: E402


def test_launcher_spawns_n_ranks():
    cmd = bench.launch_command(['--gpus', '4', '--steps', '2'], {}, n_devices=8, gpus=4)
    assert cmd[:3] == [sys.executable, '-m', 'torch.distributed.run']
    assert cmd[cmd.index('--nproc-per-node') + 1] == '4'
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1'
    assert cmd[-3:] == ['--gpus', '4', '--steps', '2'][-3:]
    assert os.path.samefile(cmd[cmd.index('--gpus') - 1], os.path.join(REPO, 'bench.py'))


def test_launcher_noop_inside_a_rank_or_single_gpu():
    assert bench.launch_command(['--gpus', '1'], {}, 8, 1) is None
    assert bench.launch_command(['--gpus', '2'], {'WORLD_SIZE': '2'}, 8, 2) is None
    with pytest.raises(SystemExit):  # an outer launcher with a different world size
        bench.launch_command(['--gpus', '4'], {'WORLD_SIZE': '2'}, 8, 4)


def test_launcher_refuses_more_ranks_than_gpus():
    with pytest.raises(SystemExit, match='only 1 GPU'):
        bench.launch_command(['--gpus', '2'], {}, 1, 2)
    # the one-GPU rehearsal shares cuda:0 between ranks
    assert bench.launch_command(['--gpus', '2'], {'LDDL_BENCH_SHARE_DEVICE': '1'}, 1, 2)


def test_launcher_end_to_end_without_gpus():
    """`python bench.py --gpus 2` on a box with no GPU fails loudly instead of running one rank."""
    env = dict(os.environ)
    env.pop('WORLD_SIZE', None)
    env.pop('LDDL_BENCH_SHARE_DEVICE', None)
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '2'], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode != 0 and 'visible' in r.stderr


def test_granted_cores():
    cores, how = bench.granted_cores()
    assert 1 <= cores <= len(os.sched_getaffinity(0))
    assert 'sched_getaffinity' in how and 'os.cpu_count()' in how


def test_pmc_json_matches_actual_batch_and_template_names():
    """The committed PMC passes are found by the batch's actual byte count and the planner's
    template instantiation is found by its base name (bench.py `traffic` / `issue_roofline`)."""
    kernels, src, meta = bench.load_pmc((10_000_000_000, 10_000_001_451))
    assert src is not None and kernels and set(meta) == {'build_id', 'git_head'}
    plan = bench.pmc_entry(kernels, 'plan_replay_kernel')
    assert plan.get('SQ_INSTS_SALU') and plan.get('hbm_bytes_per_launch')
    assert bench.pmc_entry(kernels, 'tokenize_batch_kernel').get('SQ_INSTS_VALU')
    assert bench.pmc_entry(kernels, 'no_such_kernel') == {}


def test_partition_prefix():
    """c4_exchange's sub-batch: whole leading partitions within the byte budget, at least one."""
    import types
    import numpy as np
    sent_off = np.arange(0, 1001, 10, dtype=np.int64)       # 100 sentences of 10 bytes
    doc_sent_off = np.arange(0, 101, 2, dtype=np.int64)     # 50 documents of 2 sentences
    corp = types.SimpleNamespace(sent_off=sent_off, doc_sent_off=doc_sent_off)
    part = np.arange(0, 51, 5, dtype=np.int64)              # 10 partitions of 100 bytes
    assert bench.partition_prefix(corp, part, 350) == 3
    assert bench.partition_prefix(corp, part, 400) == 4
    assert bench.partition_prefix(corp, part, 10) == 1
    assert bench.partition_prefix(corp, part, 10 ** 9) == 10


def test_dump_outputs_sample_of_a_pair_batch(tmp_path):
    """--dump-outputs: counts, exact sums (uint16 ids in int16 storage), the partition offsets and
    a seeded sample of pairs with their ragged token / position / label rows, the same files for
    the same seed."""
    import numpy as np
    import torch
    from lddl_amd.pairs import PairBatch
    g = np.random.default_rng(7)
    n = 50
    tl = g.integers(2, 9, n)
    ml = g.integers(0, 3, n)
    tok_off = np.concatenate([[0], np.cumsum(tl)]).astype(np.int64)
    pos_off = np.concatenate([[0], np.cumsum(ml)]).astype(np.int64)
    tokens = g.integers(0, 65536, tok_off[-1]).astype(np.uint16)  # ids above 32767 too
    labels = g.integers(0, 65536, pos_off[-1]).astype(np.uint16)
    pos = g.integers(0, 128, pos_off[-1]).astype(np.uint16)
    len_a = g.integers(1, 3, n).astype(np.int32)
    rn = g.integers(0, 2, n).astype(np.uint8)
    t = torch.from_numpy
    pb = PairBatch(t(tokens.view(np.int16)), t(tok_off), t(len_a), t(rn), t(pos.view(np.int16)),
                   t(labels.view(np.int16)), t(pos_off), 11, 5, t(np.asarray([0, 20, n])), 0.0,
                   int(pos_off[-1]))
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), [pb], seed=3, rank=0, world=1, n_sample=16)
    got = {f[:-4]: np.load(tmp_path / 'a' / f) for f in sorted(os.listdir(tmp_path / 'a'))}
    for k, v in got.items():
        assert v.dtype in (np.float32, np.float64), k
        assert np.array_equal(v, np.load(tmp_path / 'b' / (k + '.npy'))), k
    assert got['counts'].tolist() == [n, tok_off[-1], pos_off[-1], 11, 5]
    assert got['sums'].tolist() == [tokens.sum(dtype=np.int64), len_a.sum(), rn.sum(),
                                    pos.sum(dtype=np.int64), labels.sum(dtype=np.int64)]
    assert got['part_off'].tolist() == [0, 20, n]
    q = got['sample_pair'].astype(np.int64)
    assert len(q) == 16 and (np.diff(q) > 0).all() and q[-1] < n
    assert np.array_equal(got['sample_tok_off'], tok_off[q])
    assert np.array_equal(got['sample_pos_off'], pos_off[q])
    assert np.array_equal(got['sample_num_tokens'], tl[q] + 3)
    assert np.array_equal(got['sample_num_masked'], ml[q])
    assert np.array_equal(got['sample_len_a'], len_a[q])
    assert np.array_equal(got['sample_is_random_next'], rn[q])
    rows = lambda a, off: np.concatenate([a[off[i]:off[i + 1]] for i in q])  # noqa: E731
    assert np.array_equal(got['sample_tokens'], rows(tokens, tok_off))
    assert np.array_equal(got['sample_pos'], rows(pos, pos_off))
    assert np.array_equal(got['sample_labels'], rows(labels, pos_off))


def test_plain_run_options():
    """--steps 0 and --dump-outputs of a workload without a dump are refused before any work."""
    for argv in (['--steps', '0'], ['--workload', 'c3', '--dump-outputs', 'x']):
        r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py')] + argv,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 2 and 'bench.py: error' in r.stderr, r.stderr[-2000:]


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` prints the headline line without the lines
    that --full adds, times exactly K steps, and --dump-outputs writes the last step's sample,
    consistent with the line's own counts."""
    import json
    import numpy as np
    env = dict(os.environ)
    env.pop('WORLD_SIZE', None)
    env.pop('LDDL_BENCH_SHARE_DEVICE', None)
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', '3',
                        '--warmup', '1', '--batch-bytes', '20000000', '--dump-outputs',
                        str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith('{')][-1])
    assert line['steps'] == 3 and len(line['stages_ms']['per_step_pairs']) == 3
    assert line['ms_per_step'] > 0 and line['unit'] == 'output tokens/s'
    for k in ('cpu_baseline', 'alt_rng', 'with_segmentation', 'pcie_inclusive', 'ref_partitioning'):
        assert k not in line, k
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    n_pairs, n_tok = int(got['counts'][0]), int(got['counts'][1])
    assert n_pairs == line['config']['pairs']
    # value = output tokens ([CLS] / [SEP] included) of the K steps over their time
    assert abs(line['value'] * line['ms_per_step'] * 1e-3 - (n_tok + 3 * n_pairs)) < 1e-6 * n_tok
    assert got['part_off'][-1] == n_pairs and len(got['part_off']) == line['config']['partitions'] + 1
    assert got['sample_num_tokens'].sum() == len(got['sample_tokens']) + 3 * len(got['sample_pair'])
    assert got['sample_num_masked'].sum() == len(got['sample_pos']) == len(got['sample_labels'])
    assert got['sample_tokens'].max() < 30522 and (got['sample_num_tokens'] <= 128).all()


@pytest.mark.gpu
def test_bench_c4_exchange_subline_two_ranks():
    """`bench.py --gpus 2` in the one-GPU rehearsal (LDDL_BENCH_SHARE_DEVICE=1: two ranks on
    cuda:0, gloo through host tensors): the C2 line carries the c4_exchange sub-line, with rows
    moved between the ranks and every bin's shards within one row."""
    import json
    env = dict(os.environ, LDDL_BENCH_SHARE_DEVICE='1')
    env.pop('WORLD_SIZE', None)
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '2', '--steps', '1',
                        '--warmup', '0', '--batch-bytes', '60000000', '--exchange-bytes', '40000000',
                        '--full', '--no-alt-rng', '--no-segmented-line', '--no-extra-lines'],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith('{')][-1])
    assert line['n_gpus'] == 2
    ex = line['c4_exchange']
    assert ex['backend'] == 'gloo' and ex['num_shards'] == 16
    assert ex['moved_rows'] > 0 and ex['rows'] > ex['moved_rows']
    assert ex['shard_counts_spread'] <= 1
    assert ex['exchange_ms'] >= 0
