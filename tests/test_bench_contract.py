"""The driver's bench.py contract on the CPU (gloo): launched by torch.distributed.run with one
process per rank, or self-spawning its ranks from ``--gpus N``, bench.py prints exactly ONE JSON
line (rank 0) with the whole-job value, n_gpus = N, and ZeRO-3 active at N > 1."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ['--steps', '1', '--warmup', '1', '--model', 'gpt3-tiny', '--micro-batch', '2', '--seq', '64']


def _json_lines(out):
    return [json.loads(l) for l in out.splitlines() if l.startswith('{')]


def _env():
    # the contract is rehearsed on the CPU also where a GPU is present: the ranks of a two-rank
    # run would share the one GPU (RCCL refuses that), so the devices are hidden from bench.py
    env = dict(os.environ, OMP_NUM_THREADS='2', PRA_BENCH_TIMEOUT='200',
               HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    return env


def _check(lines, n):
    assert len(lines) == 1, lines
    r = lines[0]
    assert r['n_gpus'] == n and r['steps'] == 1 and r['warmup'] == 1
    assert r['value'] > 0 and r['ms_per_step'] > 0 and r['higher_is_better'] is True
    assert r['config']['global_batch'] == 2 * n
    assert r['config']['zero3_active'] is (n > 1)
    return r


@pytest.mark.timeout(300)
def test_bench_under_torchrun_two_ranks():
    # (--standalone: torchrun picks a free rendezvous port itself, no race with parallel tests)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--standalone', '--local-addr', '127.0.0.1',
           '--nnodes=1', '--nproc-per-node', '2', 'bench.py', '--gpus', '2'] + ARGS
    p = subprocess.run(cmd, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, p.stderr[-3000:]
    _check(_json_lines(p.stdout), 2)


@pytest.mark.timeout(300)
def test_bench_self_spawned_ranks():
    p = subprocess.run([sys.executable, 'bench.py', '--gpus', '2'] + ARGS, cwd=ROOT, env=_env(),
                       capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, p.stderr[-3000:]
    _check(_json_lines(p.stdout), 2)


@pytest.mark.timeout(300)
def test_bench_dump_outputs_repeatable_and_full_flag(tmp_path):
    """``--dump-outputs DIR`` writes the last timed step's outputs as float32 ``.npy``; the same
    arguments give the same inputs, so on the CPU two runs agree; ``--steps`` sets the number of
    timed steps; ``--full`` is accepted and keeps the result line."""
    import numpy as np
    args = ['--steps', '2', '--warmup', '1'] + ARGS[4:]
    env = _env()   # (CPU: float atomics make two GPU runs differ in the last bits)
    res = []
    for d, extra in (('a', []), ('b', ['--full'])):
        p = subprocess.run([sys.executable, 'bench.py'] + args + ['--dump-outputs', str(tmp_path / d)] + extra,
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=280)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = _json_lines(p.stdout)
        assert len(lines) == 1, lines
        res.append(lines[0])
    for r in res:
        assert r['steps'] == 2 and r['warmup'] == 1 and r['ms_per_step'] > 0
        assert r['unit'] == 'tokens/s' and r['dtype'] == 'bf16' and r['higher_is_better'] is True
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == ['loss.npy', 'losses.npy', 'params_sample.npy'] == sorted(os.listdir(tmp_path / 'b'))
    total = 0
    for n in names:
        x, y = np.load(tmp_path / 'a' / n), np.load(tmp_path / 'b' / n)
        assert x.dtype == np.float32 and x.size > 0 and np.isfinite(x).all()
        np.testing.assert_allclose(x, y, rtol=1e-5, atol=1e-6)
        total += x.nbytes
    assert total <= 64 << 20
    losses = np.load(tmp_path / 'a' / 'losses.npy')
    assert losses.shape == (2,)                      # one loss per timed step
    assert abs(float(np.load(tmp_path / 'a' / 'loss.npy')[0]) - res[0]['final_loss']) < 1e-3
    assert losses[-1] == np.load(tmp_path / 'a' / 'loss.npy')[0]


@pytest.mark.timeout(300)
def test_bench_single_rank_defaults_shape():
    p = subprocess.run([sys.executable, 'bench.py'] + ARGS, cwd=ROOT, env=_env(), capture_output=True,
                       text=True, timeout=280)
    assert p.returncode == 0, p.stderr[-3000:]
    r = _check(_json_lines(p.stdout), 1)
    assert r['dtype'] == 'bf16' and r['scaling'] == 'weak' and 'synthetic' in r['data']
