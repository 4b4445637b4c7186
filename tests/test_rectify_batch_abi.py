"""CPU-side checks of the batched plate rectification (dbx_warp_perspective_batch_u8, dbx_warp_batch_workspace_bytes,
rectify.perspective_transform_batch, decode.detect_plates): every bad argument is refused on the host, with an error code and a
message naming the entry point, before anything is launched; the plate window arithmetic; the Python argument checks."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from densebox_amd import _lib, rectify


def _job(**kw):
    j = _lib.WarpJob()
    j.src, j.sh, j.sw = 0x1000, 120, 200
    j.m9[:] = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    j.dh, j.dw, j.x0, j.y0, j.oh, j.ow, j.dst_off = 180, 300, 0, 0, 180, 300, 0
    for k, v in kw.items():
        if k == 'm9':
            j.m9[:] = v
        else:
            setattr(j, k, v)
    return j


def _call(L, jobs, njobs=None, c=3, dst=0x2000, ws=0x3000):
    arr = (_lib.WarpJob * max(1, len(jobs)))(*jobs)
    vp = lambda a: None if a is None else C.c_void_p(a)       # noqa: E731
    return L.dbx_warp_perspective_batch_u8(arr, len(jobs) if njobs is None else njobs, c, vp(dst), vp(ws), None)


@pytest.mark.parametrize('bad', [
    dict(njobs=-1), dict(c=0), dict(c=5), dict(dst=None), dict(ws=None),
    dict(job=dict(src=None)),
    dict(job=dict(sh=0)), dict(job=dict(sw=-2)), dict(job=dict(dh=0)), dict(job=dict(dw=0)), dict(job=dict(oh=0)), dict(job=dict(ow=-1)),
    dict(job=dict(x0=-1, ow=10)), dict(job=dict(y0=-1, oh=10)), dict(job=dict(x0=1)), dict(job=dict(y0=171, oh=10)),
    dict(job=dict(x0=290, ow=11)), dict(job=dict(dst_off=-16)),
    dict(job=dict(m9=[0.0] * 9)), dict(job=dict(m9=[1.0, 2.0, 0.0, 2.0, 4.0, 0.0, 0.0, 0.0, 1.0])),
    dict(job=dict(m9=[1.0, 0.0, float('nan'), 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])),
    dict(job=dict(m9=[1.0, 0.0, 0.0, 0.0, float('inf'), 0.0, 0.0, 0.0, 1.0])),
])
def test_warp_batch_rejects_bad_arguments_without_touching_the_gpu(bad):
    L = _lib.lib()
    bad = dict(bad)
    jobs = [_job(), _job(**bad.pop('job', {}))]
    rc = _call(L, jobs, **bad)
    assert rc == -1, bad
    msg = L.dbx_last_error()
    assert b'warp_perspective_batch' in msg, msg
    with pytest.raises(RuntimeError, match='warp_perspective_batch'):
        _lib.check(rc)


def test_warp_batch_null_job_list_and_empty_call():
    L = _lib.lib()
    assert L.dbx_warp_perspective_batch_u8(None, 1, 3, C.c_void_p(0x2000), C.c_void_p(0x3000), None) == -1
    assert b'warp_perspective_batch' in L.dbx_last_error()
    assert _call(L, [_job()], njobs=0) == 0                              # njobs == 0: a no-op that launches nothing
    assert L.dbx_warp_perspective_batch_u8(None, 0, 3, None, None, None) == 0


def test_warp_batch_workspace_grows_with_the_job_count():
    L = _lib.lib()
    sizes = [L.dbx_warp_batch_workspace_bytes(n) for n in (0, 1, 2, 10, 100, 320, 10000)]
    assert all(s > 0 and s % 256 == 0 for s in sizes), sizes
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] < sizes[3] < sizes[4] < sizes[5] < sizes[6], sizes
    assert sizes[-1] >= 10000 * (C.sizeof(_lib.WarpJob))                # at least a record per job
    assert L.dbx_warp_batch_workspace_bytes(-1) < 0


def test_warp_job_struct_layout_matches_the_header():
    assert C.sizeof(_lib.WarpJob) == 120
    assert _lib.WarpJob.m9.offset == 16 and _lib.WarpJob.dh.offset == 88 and _lib.WarpJob.dst_off.offset == 112


def test_plate_window_arithmetic():
    dh, dw = rectify.canvas_size(120, 200)
    assert (dh, dw) == (180, 300)
    # fractional corners: floor of the minimum, ceil of the maximum, inclusive
    dst = rectify.dst_rectangle([[60.3, 50.7], [180.2, 52.0], [176.5, 110.1], [56.9, 100.0]])
    assert rectify.plate_window(dst, dh, dw) == (56, 50, 111 - 50 + 1, 181 - 56 + 1)
    # integer corners stay put
    assert rectify.plate_window([[10, 20], [30, 20], [30, 40], [10, 40]], dh, dw) == (10, 20, 21, 21)
    # corners outside the canvas are clipped to it
    assert rectify.plate_window([[-5.5, -3.2], [400.0, -3.2], [400.0, 500.0], [-5.5, 500.0]], dh, dw) == (0, 0, dh, dw)
    assert rectify.plate_window([[290.5, 170.5], [310, 170.5], [310, 190], [290.5, 190]], dh, dw) == (290, 170, 10, 10)
    # empty: entirely left of / below the canvas
    assert rectify.plate_window([[-20, 10], [-10, 10], [-10, 30], [-20, 30]], dh, dw) is None
    assert rectify.plate_window([[10, 181], [30, 181], [30, 200], [10, 200]], dh, dw) is None
    # the float32 corner values decide: 0.99999999 rounds to 1.0 in float32
    assert rectify.plate_window([[0.99999999, 1], [2, 1], [2, 2], [0.99999999, 2]], dh, dw) == (1, 1, 2, 2)
    assert math.floor(np.float32(0.99999999)) == 1


def test_job_windows_from_quads():
    q = [[60.3, 50.7], [180.2, 52.0], [176.5, 110.1], [56.9, 100.0]]
    M, dh, dw, x0, y0, oh, ow = rectify._rect_job(q, 120, 200, 'canvas')
    assert (dh, dw, x0, y0, oh, ow) == (180, 300, 0, 0, 180, 300)                 # the whole canvas
    assert np.array_equal(M, rectify.get_perspective_matrix(q, rectify.dst_rectangle(q)))
    assert rectify._rect_job(q, 120, 200, 'plate')[3:] == (56, 50, 62, 126)
    assert rectify._rect_job([[0, 0], [1, 1], [2, 2], [3, 3]], 120, 200, 'canvas') is None            # degenerate
    assert rectify._rect_job([[0, 0], [float('nan'), 0], [10, 10], [0, 10]], 120, 200, 'plate') is None
    assert rectify._rect_job([[0, 0], [float('inf'), 0], [10, 10], [0, 10]], 120, 200, 'canvas') is None
    assert rectify._rect_job([[-40, -30], [-20, -30], [-18, -10], [-41, -12]], 120, 200, 'plate') is None   # empty window
    assert rectify._rect_job([[-40, -30], [-20, -30], [-18, -10], [-41, -12]], 120, 200, 'canvas') is not None


def test_perspective_transform_batch_argument_checks():
    img = np.zeros((20, 30, 3), np.uint8)
    q = [[1, 1], [10, 1], [10, 8], [1, 8]]
    with pytest.raises(TypeError, match='region'):                         # keyword-only, no default
        rectify.perspective_transform_batch([img], [[q]])
    with pytest.raises(RuntimeError, match='region'):
        rectify.perspective_transform_batch([img], [[q]], region='window')
    with pytest.raises(RuntimeError, match='2 lists of quads for 1 images'):
        rectify.perspective_transform_batch([img], [[q], [q]], region='plate')
    with pytest.raises(RuntimeError, match='lists of quads'):
        rectify.perspective_transform_batch(torch.zeros(3, 20, 30, 3, dtype=torch.uint8), [[q]], region='canvas')
    with pytest.raises(RuntimeError, match='uint8'):
        rectify.perspective_transform_batch([img.astype(np.float32)], [[q]], region='canvas')
    with pytest.raises(RuntimeError, match='channels'):
        rectify.perspective_transform_batch([img, np.zeros((20, 30, 1), np.uint8)], [[q], [q]], region='canvas')
    with pytest.raises(RuntimeError, match='channels'):
        rectify.perspective_transform_batch([np.zeros((20, 30, 5), np.uint8)], [[q]], region='canvas')


def test_detect_plates_python_argument_checks():
    """Float frames, a missing or unknown region, a DenseBox net (no landmarks) are refused before any device work."""
    import densebox_amd as D
    from densebox_amd import decode as DC, synth
    lm = D.DenseBoxLM(synth.vgg19_standin(seed=0)).eval()
    frames = torch.zeros(2, 64, 64, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='uint8'):
        lm.detect_plates(torch.zeros(2, 3, 64, 64), region='plate')
    with pytest.raises(RuntimeError, match='uint8'):
        lm.detect_plates([torch.zeros(64, 64, 3)], region='plate')
    with pytest.raises(RuntimeError, match='channels'):
        lm.detect_plates(torch.zeros(2, 64, 64, 4, dtype=torch.uint8), region='plate')
    with pytest.raises(TypeError, match='region'):                         # keyword-only, no default
        lm.detect_plates(frames)
    with pytest.raises(TypeError, match='region'):
        DC.detect_plates(lm, frames)
    with pytest.raises(RuntimeError, match='region'):
        DC.detect_plates(lm, frames, region='full')
    box = D.DenseBox(synth.vgg19_standin(seed=0)).eval()
    with pytest.raises(RuntimeError, match='DenseBox rows have no landmarks'):
        box.detect_plates(frames, region='canvas')
