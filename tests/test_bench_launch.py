"""bench.py launch contract: `python bench.py --gpus N` without a launcher must start N ranks itself (it used to run ONE rank
and print n_gpus: 1).  CPU: the rendezvous-only --dry-run over gloo; GPU: two ranks sharing cuda:0 over gloo run real steps."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra, timeout):
    """Runs bench.py once; any failure fails the test."""
    env = dict(os.environ, **env_extra)
    env.pop('WORLD_SIZE', None); env.pop('RANK', None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]           # exactly ONE JSON line, from rank 0
    return json.loads(lines[0])


def test_bench_self_launches_two_ranks_dry_run():
    out = _run(['--gpus', '2', '--dry-run'], {'DBX_DIST_BACKEND': 'gloo'}, 300)
    assert out['n_gpus'] == 2 and out['rank_sum'] == 3 and out['backend'] == 'gloo'


def test_bench_single_rank_dry_run():
    out = _run(['--gpus', '1', '--dry-run'], {}, 300)
    assert out['n_gpus'] == 1


@pytest.mark.gpu
def test_bench_two_ranks_on_one_gpu_gloo():
    out = _run(['--gpus', '2', '--steps', '2', '--warmup', '1', '--batch', '4', '--full', '--no-cpu-baseline', '--no-inference'],
               {'DBX_DIST_BACKEND': 'gloo'}, 1200)
    assert out['n_gpus'] == 2 and out['config']['global_batch'] == 8 and out['value'] > 0
    assert out['roofline']['kernel'] and 0 < out['roofline']['frac'] < 1


@pytest.mark.gpu
def test_bench_plain_run_times_steps_and_dumps_outputs(tmp_path):
    """A plain run (no --full) prints the headline line only, and --dump-outputs writes what the last timed step computed: the loss of
    the line, finite fp32 gradients and parameters, under 64 MB in all.  A second run with the same arguments sees the same inputs
    (seeded data, draws and dropout hash) and must write bitwise the same files."""
    import numpy as np
    args = ['--gpus', '1', '--steps', '3', '--warmup', '1', '--batch', '4']
    dumps, lines = [tmp_path / 'a', tmp_path / 'b'], []
    for d in dumps:
        lines.append(_run(args + ['--dump-outputs', str(d)], {}, 1200))
    out = lines[0]
    assert out['steps'] == 3 and out['ms_per_step'] > 0 and out['value'] > 0 and out['full'] is False
    assert {'metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'} <= set(out)
    assert not {'roofline', 'tolerance', 'inference', 'cpu_baseline', 'bf16'} & set(out)
    d = dumps[0]
    files = {f.name for f in d.iterdir()}
    assert files == {'loss.npy', 'grad.npy', 'param.npy'}, files
    assert sum(f.stat().st_size for f in d.iterdir()) <= 64 << 20
    loss = np.load(d / 'loss.npy')
    assert loss.dtype == np.float64 and loss.shape == (1,) and round(float(loss[0]), 2) == out['config']['loss']
    for name in ('grad', 'param'):
        a = np.load(d / (name + '.npy'))
        assert a.dtype == np.float32 and a.ndim == 1 and a.size > 0 and np.isfinite(a).all(), name
    assert np.abs(np.load(d / 'grad.npy')).max() > 0
    # run to run: identical line figures of the step's results, identical files
    assert lines[1]['config']['loss'] == out['config']['loss'] and lines[1]['config']['grad_absmax'] == out['config']['grad_absmax']
    assert {f.name for f in dumps[1].iterdir()} == files
    for name in sorted(files):
        a, b = np.load(dumps[0] / name), np.load(dumps[1] / name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name


def _run_expect_failure(args, env_extra, timeout):
    import time
    env = dict(os.environ, **env_extra)
    env.pop('WORLD_SIZE', None); env.pop('RANK', None)
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, capture_output=True, text=True, timeout=timeout, env=env)
    dt = time.time() - t0
    assert r.returncode != 0, r.stdout[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{')]
    errs = [l for l in lines if 'error' in l]
    assert errs, 'no parsable failure line:\n' + r.stdout[-2000:] + r.stderr[-3000:]
    assert not any('value' in l for l in lines)         # no bench line next to a failure line
    return errs[0], dt


def test_bench_failed_collective_setup_reports_one_json_line():
    """The N > 1 path must never hang or die with only a traceback: here the RCCL backend is asked for on a box where it cannot
    come up (no GPU: the process group constructor refuses) -- rank 0 prints {"error": ..., "rccl": {...}} and the job exits non-zero."""
    import torch
    if torch.cuda.is_available():
        pytest.skip('CPU-only variant (the GPU box runs test_bench_two_ranks_nccl_on_one_gpu_fails_fast)')
    err, dt = _run_expect_failure(['--gpus', '2', '--dry-run'], {'DBX_DIST_BACKEND': 'nccl', 'DBX_DIST_TIMEOUT_S': '30'}, 300)
    assert err['rccl']['world'] == 2 and err['rccl']['timeout_s'] == 30.0 and 'DBX_DIST_BACKEND' in err['rccl']['env']
    assert dt < 150


@pytest.mark.gpu
def test_bench_two_ranks_nccl_on_one_gpu_fails_fast():
    """Two RCCL ranks on ONE GPU cannot form a communicator (duplicate device): the first collective fails or stalls -- the bounded
    process-group timeout / the watchdog around the first all-reduce turn that into one JSON failure line within the bound, not the
    ten-minute default hang.  (The first real N > 1 RCCL run happens on the driver's multi-GPU box with nobody watching.)"""
    import torch
    if torch.cuda.device_count() != 1:
        pytest.skip('needs exactly one visible GPU')
    err, dt = _run_expect_failure(['--gpus', '2', '--steps', '1', '--warmup', '0', '--batch', '2', '--no-cpu-baseline', '--no-inference'],
                                  {'DBX_DIST_BACKEND': 'nccl', 'DBX_DIST_TIMEOUT_S': '60'}, 400)
    assert err['rccl']['world'] == 2 and err['rccl']['gpus_visible'] == 1
    assert dt < 150, dt
