"""World size 8 (BASELINE configs[3]): eight ranks over gloo, one per GPU.  Functional coverage of the N = 8 path only (rank slices,
the positive-count all-reduce, bucket order, every rank's parameters equal after a step, the bench's launch contract) -- no scaling
number.  Needs eight GPUs: eight device contexts time-slicing one device died in driver code (a fault in torch's fill kernel at
start-up, an illegal-instruction abort mid-run) about once in three runs, with kernels that pass at world sizes 1 and 2.  With fewer
GPUs these tests skip; world 2 on one GPU: tests/test_hip_dist.py, tests/test_bench_launch.py; world 8's rank slices, positive count
and sharded loss, in one CPU process: tests/test_dist_gloo.py."""
import pytest

from test_bench_launch import _run
from test_hip_dist import run_ranks_equal_one_process

pytestmark = pytest.mark.gpu


def _need_gpus(k):
    import torch
    found = torch.cuda.device_count()
    if found < k:
        pytest.skip('needs %d GPUs (one rank per device), found %d' % (k, found))


def test_eight_ranks_equal_one_process(tmp_path):
    _need_gpus(8)
    run_ranks_equal_one_process(tmp_path, 8)


def test_bench_eight_ranks_on_one_gpu_gloo():
    """configs[3]'s world size: 8 ranks over gloo, one per GPU, 2 patches each (global batch 16): rank slices, the positive-count
    all-reduce, bucket order and the max-over-ranks timing at world 8.  No scaling number."""
    _need_gpus(8)
    out = _run(['--gpus', '8', '--steps', '2', '--warmup', '1', '--batch', '2', '--full', '--no-cpu-baseline', '--no-inference'],
               {'DBX_DIST_BACKEND': 'gloo'}, 1200)
    assert out['n_gpus'] == 8 and out['config']['global_batch'] == 16 and out['value'] > 0
    assert out['rccl']['world'] == 8 and out['rccl']['collective']
