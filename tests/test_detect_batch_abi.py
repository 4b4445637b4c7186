"""CPU-side checks of the batched decode entry points (dbx_detect_batch, dbx_detect_batch_scratch_bytes) and of detect_batch's
argument checks: every bad argument is refused on the host, with an error code and a message, before anything is launched."""
import ctypes as C

import pytest
import torch

from densebox_amd import _lib


def _call(L, score=0x1000, loc=0x2000, lm_heat=None, lm_loc=None, batch=2, rows=60, cols=60, K=10, dets=0x3000, det_cols=5,
          topk=0x4000, keep=0x5000, scratch=0x6000):
    vp = lambda a: None if a is None else C.c_void_p(a)       # noqa: E731
    return L.dbx_detect_batch(vp(score), vp(loc), vp(lm_heat), vp(lm_loc), batch, rows, cols, K, 0.4, vp(dets), det_cols,
                              vp(topk), vp(keep), vp(scratch), None)


@pytest.mark.parametrize('bad', [
    dict(score=None), dict(loc=None), dict(dets=None), dict(topk=None), dict(keep=None), dict(scratch=None),
    dict(batch=0), dict(batch=-3),
    dict(K=0), dict(K=-1), dict(K=60 * 60 + 1), dict(rows=2, cols=3, K=7),
    dict(det_cols=4), dict(det_cols=6), dict(det_cols=13), dict(det_cols=12, lm_heat=0x7000),
    dict(det_cols=5 + 8, rows=0, lm_heat=0x7000),
])
def test_detect_batch_rejects_bad_arguments_without_touching_the_gpu(bad):
    L = _lib.lib()
    rc = _call(L, **bad)
    assert rc == -1, bad
    msg = L.dbx_last_error()
    assert b'detect_batch' in msg, msg
    with pytest.raises(RuntimeError, match='detect_batch'):
        _lib.check(rc)


def test_detect_batch_scratch_is_linear_in_batch_with_256_byte_slices():
    L = _lib.lib()
    for rows, cols, K in ((60, 60, 10), (60, 60, 1000), (128, 128, 10), (270, 480, 10), (270, 480, 1000), (25, 33, 7), (1, 1, 1)):
        one = L.dbx_detect_batch_scratch_bytes(1, rows, cols, K)
        assert one % 256 == 0, (rows, cols, K, one)
        assert one >= L.dbx_detect_scratch_bytes(rows, cols, K)             # each slice holds the single-image layout
        assert one - L.dbx_detect_scratch_bytes(rows, cols, K) < 256
        for B in (2, 3, 32, 256):
            assert L.dbx_detect_batch_scratch_bytes(B, rows, cols, K) == B * one


def test_detect_batch_python_argument_checks():
    """Empty batches, lists that mix uint8 and float images and malformed tensors are refused before any device work."""
    import densebox_amd as D
    from densebox_amd import decode as DC, synth
    net = D.DenseBox(synth.vgg19_standin(seed=0)).eval()
    with pytest.raises(RuntimeError, match='empty'):
        net.detect_batch([])
    with pytest.raises(RuntimeError, match='empty'):
        DC.detect_batch(net, torch.zeros(0, 3, 64, 64))
    with pytest.raises(RuntimeError, match='mixes'):
        net.detect_batch([torch.zeros(3, 64, 64), torch.zeros(64, 64, 3, dtype=torch.uint8)])
    with pytest.raises(RuntimeError, match='uint8'):
        net.detect_batch(torch.zeros(2, 3, 64, 64, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match=r'\[B,3,H,W\]'):
        net.detect_batch(torch.zeros(2, 64, 64, 3))
    with pytest.raises(RuntimeError, match='single images'):
        net.detect_batch([torch.zeros(2, 3, 64, 64)])
    with pytest.raises(RuntimeError, match='tensor'):
        net.detect_batch([torch.zeros(3, 64, 64), 'image.jpg'])
    with pytest.raises(RuntimeError, match='max_batch'):
        net.detect_batch(torch.zeros(2, 3, 64, 64), max_batch=0)
