"""CPU-side checks of the score-threshold decode: dbx_detect_thresh_batch and dbx_nms_large refuse every bad argument on the host, with
an error code and a message that names the function, before anything is launched; their scratch contracts; the Python entry points'
argument checks (no device work); the NumPy restatement the GPU tests use == the rows and keep list captured from the reference."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from densebox_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thresh_ref  # noqa: E402

NAN = float('nan')


def _call(L, score=0x1000, loc=0x2000, lm_heat=None, lm_loc=None, batch=2, rows=60, cols=60, t=0.5, max_dets=1024, nms=0.4,
          dets=0x3000, det_cols=5, topk=0x4000, keep=0x5000, counts=0x7000, scratch=0x6000):
    vp = lambda a: None if a is None else C.c_void_p(a)       # noqa: E731
    return L.dbx_detect_thresh_batch(vp(score), vp(loc), vp(lm_heat), vp(lm_loc), batch, rows, cols, t, max_dets, nms, vp(dets),
                                     det_cols, vp(topk), vp(keep), vp(counts), vp(scratch), None)


@pytest.mark.parametrize('bad', [
    dict(score=None), dict(loc=None), dict(dets=None), dict(topk=None), dict(keep=None), dict(counts=None), dict(scratch=None),
    dict(batch=0), dict(batch=-3),
    dict(rows=0), dict(cols=-1), dict(rows=65536, cols=65536),
    dict(max_dets=0), dict(max_dets=-1), dict(max_dets=4097),
    dict(t=NAN), dict(nms=NAN), dict(nms=-0.1),
    dict(det_cols=4), dict(det_cols=6), dict(det_cols=13), dict(det_cols=12, lm_heat=0x8000),
])
def test_detect_thresh_batch_rejects_bad_arguments_without_touching_the_gpu(bad):
    L = _lib.lib()
    rc = _call(L, **bad)
    assert rc == -1, bad
    msg = L.dbx_last_error()
    assert b'detect_thresh_batch' in msg, msg
    with pytest.raises(RuntimeError, match='detect_thresh_batch'):
        _lib.check(rc)


@pytest.mark.parametrize('bad', [
    dict(dets=None), dict(keep=None), dict(scratch=None), dict(n=0), dict(n=-5), dict(n=4097), dict(det_cols=4), dict(nms=NAN),
    dict(nms=-1.0),
])
def test_nms_large_rejects_bad_arguments_without_touching_the_gpu(bad):
    L = _lib.lib()
    a = dict(dets=0x1000, n=100, det_cols=5, nms=0.4, keep=0x2000, scratch=0x3000)
    a.update(bad)
    vp = lambda v: None if v is None else C.c_void_p(v)       # noqa: E731
    rc = L.dbx_nms_large(vp(a['dets']), a['n'], a['det_cols'], a['nms'], vp(a['keep']), vp(a['scratch']), None)
    assert rc == -1, bad
    assert b'nms_large' in L.dbx_last_error()


def test_scratch_contracts():
    L = _lib.lib()
    prev = 0
    for cap in (1, 10, 64, 65, 1000, 1024, 1025, 4096):
        one = L.dbx_detect_thresh_batch_scratch_bytes(1, 270, 480, cap)
        assert one > 0 and one % 256 == 0, (cap, one)
        assert one >= prev, cap                                   # monotone in max_dets
        prev = one
        for B in (2, 3, 32, 256):
            assert L.dbx_detect_thresh_batch_scratch_bytes(B, 270, 480, cap) == B * one
        # rows (13 columns), indices, order and the cap x ceil(cap / 64)-word matrix fit
        assert one >= cap * 13 * 8 + cap * 8 + cap * 4 + cap * ((cap + 63) // 64) * 8
    assert L.dbx_detect_thresh_batch_scratch_bytes(1, 60, 60, 4096) <= 3 * 2 ** 20
    for bad in ((0, 60, 60, 10), (1, 0, 60, 10), (1, 60, 60, 0), (1, 60, 60, 4097)):
        assert L.dbx_detect_thresh_batch_scratch_bytes(*bad) == -1
    prev = 0
    for n in (1, 64, 65, 1024, 1025, 4096):
        s = L.dbx_nms_large_scratch_bytes(n)
        assert s >= n * 4 + n * ((n + 63) // 64) * 8 and s >= prev
        prev = s
    assert L.dbx_nms_large_scratch_bytes(0) == -1 and L.dbx_nms_large_scratch_bytes(4097) == -1


def test_python_argument_checks_fail_before_any_device_work():
    import densebox_amd as D
    from densebox_amd import decode as DC, synth
    net = D.DenseBoxLM(synth.vgg19_standin(seed=0)).eval()
    x = torch.zeros(2, 3, 64, 64)
    u8 = torch.zeros(2, 64, 64, 3, dtype=torch.uint8)
    for bad in (NAN, float('inf'), -float('inf'), '0.5', None, True, np.bool_(False), [0.5]):
        with pytest.raises(RuntimeError, match='detect_batch_thresh: score_thresh'):
            net.detect_batch_thresh(x, bad)
    for bad in (0, -1, 4097, 10.0, '10', True, None):
        with pytest.raises(RuntimeError, match='detect_batch_thresh: max_dets'):
            DC.detect_batch_thresh(net, x, 0.5, max_dets=bad)
    with pytest.raises(RuntimeError, match='detect_batch_thresh: empty'):
        net.detect_batch_thresh([], 0.5)
    with pytest.raises(RuntimeError, match='detect_batch_thresh: max_batch'):
        net.detect_batch_thresh(x, 0.5, max_batch=0)
    with pytest.raises(RuntimeError, match='detect_batch_thresh.*mixes'):
        net.detect_batch_thresh([torch.zeros(3, 64, 64), torch.zeros(64, 64, 3, dtype=torch.uint8)], 0.5)
    with pytest.raises(RuntimeError, match='detect_batch_resized: score_thresh'):
        net.detect_batch_resized(u8, score_thresh=NAN)
    with pytest.raises(RuntimeError, match='detect_batch_resized: max_dets'):
        net.detect_batch_resized(u8, score_thresh=0.5, max_dets=5000)
    with pytest.raises(RuntimeError, match='detect_batch_resized: K=7 and score_thresh'):
        net.detect_batch_resized(u8, K=7, score_thresh=0.5)
    with pytest.raises(RuntimeError, match='detect_plates: score_thresh'):
        net.detect_plates(u8, region='plate', score_thresh=True)
    with pytest.raises(RuntimeError, match='detect_plates: max_dets'):
        DC.detect_plates(net, u8, region='plate', score_thresh=0.5, max_dets=0)
    with pytest.raises(RuntimeError, match='detect_plates: K=3 and score_thresh'):
        net.detect_plates(u8, K=3, region='canvas', score_thresh=0.5)


def test_thresh_ref_is_the_reference_on_the_captured_fixture(golden):
    """> 1024 candidates: rows and keep list as the reference's own parse_DetLMLOC(K = n) + NMS produced them"""
    g = golden('decode_thresh')
    rows, cols = g['score'].shape[2:]
    t, nms_t = float(g['t']), float(g['nms_thresh'])
    n = int((g['score'] > g['t']).sum())
    assert n == g['rows'].shape[0] and n > 1024
    assert len(np.unique(g['rows'][:, 4])) == n                               # distinct scores: NumPy's sort order is defined
    dets, keep, total = thresh_ref.thresh_detect(g['score'], g['loc'], g['lm_heat'], g['lm_loc'], rows * 4, cols * 4, t, 4096, nms_t)
    assert total == n and dets.dtype == np.float64
    assert dets.tobytes() == g['rows'].tobytes()
    assert keep == [int(v) for v in g['keep']]
    # the cap: max_dets below the count is the reference's top-max_dets
    dets2, keep2, total2 = thresh_ref.thresh_detect(g['score'], g['loc'], g['lm_heat'], g['lm_loc'], rows * 4, cols * 4, t, 1000, nms_t)
    assert total2 == n and dets2.tobytes() == g['rows'][:1000].tobytes()
    e, k, tot = thresh_ref.thresh_detect(g['score'], g['loc'], g['lm_heat'], g['lm_loc'], rows * 4, cols * 4, 2.0, 4096, nms_t)
    assert e.shape == (0, 13) and k == [] and tot == 0
