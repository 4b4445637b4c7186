"""CPU-side checks of the fixed-size plate crops (dbx_plate_crops_batch, rectify.plate_crops_batch, decode.detect_plate_crops): the new
symbols are declared, bound and exported without an ABI bump; every bad argument is refused on the host, with an error code and a
message naming the entry point, before anything is launched; the Python argument checks run before the device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from densebox_amd import _lib, rectify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['dbx_plate_crops_batch']


def test_new_entry_point_is_exported_declared_and_bound_without_a_bump():
    L = _lib.lib()
    src = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, code), name + ' is not declared'
        assert name in _lib.SIGNATURES and name not in _lib.MISSING, name
        assert callable(getattr(L, name))
    assert re.search(r'\bdbx_crop_frame\b', code)
    assert int(re.search(r'#define\s+DBX_ABI_VERSION\s+(\d+)', src).group(1)) == L.dbx_version() == _lib.ABI_VERSION == 13
    assert re.search(r'without a bump: dbx_crop_frame, dbx_plate_crops_batch', src)
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert all(name in doc for name in NEW + ['dbx_crop_frame'])


def test_crop_frame_struct_layout_matches_the_header():
    assert C.sizeof(_lib.CropFrame) == 16
    assert _lib.CropFrame.src.offset == 0 and _lib.CropFrame.sh.offset == 8 and _lib.CropFrame.sw.offset == 12


def _call(L, frames=0x1000, nframes=2, c=3, quads=0x2000, row_stride=13, frame_stride=130, sel=0x3000, slots=10, ow=94, oh=24,
          dst=0x4000, ok=0x5000, m9=None):
    vp = lambda a: None if a is None else C.c_void_p(a)       # noqa: E731
    return L.dbx_plate_crops_batch(vp(frames), nframes, c, vp(quads), row_stride, frame_stride, vp(sel), slots, ow, oh, vp(dst), vp(ok),
                                   vp(m9), None)


@pytest.mark.parametrize('bad', [
    dict(frames=None), dict(quads=None), dict(dst=None), dict(ok=None),
    dict(c=0), dict(c=5), dict(c=-1),
    dict(slots=0), dict(slots=-2),
    dict(ow=0), dict(oh=0), dict(ow=-94), dict(oh=-1),
    dict(nframes=-1),
    dict(row_stride=7), dict(row_stride=0), dict(row_stride=-13),
    dict(sel=None, frame_stride=129), dict(sel=None, frame_stride=0), dict(sel=None, row_stride=8, slots=4, frame_stride=31),
    dict(nframes=1 << 20, slots=1 << 10, ow=2048, oh=1),                  # 2^30 tiles: beyond one grid
    dict(nframes=1, slots=1, ow=1 << 30, oh=1 << 6),                      # 2^25 tiles in one slot
])
def test_plate_crops_batch_rejects_bad_arguments_without_touching_the_gpu(bad):
    L = _lib.lib()
    rc = _call(L, **bad)
    assert rc == -1, bad
    msg = L.dbx_last_error()
    assert b'plate_crops_batch' in msg, msg
    with pytest.raises(RuntimeError, match='plate_crops_batch'):
        _lib.check(rc)


def test_plate_crops_batch_empty_call_is_a_no_op():
    L = _lib.lib()
    assert _call(L, frames=None, nframes=0, quads=None, sel=None, dst=None, ok=None) == 0       # all pointers null: nothing is touched
    assert _call(L, nframes=0) == 0


def test_plate_rectangle():
    assert rectify.plate_rectangle((94, 24)) == [[0, 0], [93, 0], [93, 23], [0, 23]]
    assert rectify.plate_rectangle(5) == [[0, 0], [4, 0], [4, 4], [0, 4]]
    assert rectify.plate_rectangle((1, 1)) == [[0, 0]] * 4
    for bad in ((0, 24), (94, -1), (94, 24, 3), (94,), 'wide', None, 0):
        with pytest.raises(RuntimeError, match='size'):
            rectify.plate_rectangle(bad)


def test_plate_crops_batch_python_argument_checks():
    img = np.zeros((20, 30, 3), np.uint8)
    q = [[1, 1], [10, 1], [10, 8], [1, 8]]
    with pytest.raises(TypeError, match='size'):                           # keyword-only, no default
        rectify.plate_crops_batch([img], [[q]])
    for bad in ((0, 24), (94, -3), (94, 24, 3), None):
        with pytest.raises(RuntimeError, match='size'):
            rectify.plate_crops_batch([img], [[q]], size=bad)
    with pytest.raises(RuntimeError, match='2 lists of quads for 1 images'):
        rectify.plate_crops_batch([img], [[q], [q]], size=(94, 24))
    with pytest.raises(RuntimeError, match='lists of quads'):
        rectify.plate_crops_batch(torch.zeros(3, 20, 30, 3, dtype=torch.uint8), [[q]], size=(94, 24))
    with pytest.raises(RuntimeError, match='uint8'):
        rectify.plate_crops_batch([img.astype(np.float32)], [[q]], size=(94, 24))
    with pytest.raises(RuntimeError, match='channels'):
        rectify.plate_crops_batch([np.zeros((20, 30, 5), np.uint8)], [[q]], size=(94, 24))
    for bad in ([[[1, 1], [10, 1], [10, 8]]], [[1, 2, 3, 4, 5, 6, 7]], np.zeros((2, 9)), np.zeros((2, 2, 4)), torch.zeros(3, 7),
                [q, [[1, 1], [2, 2]]], [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]):
        with pytest.raises(RuntimeError, match='8 numbers'):
            rectify.plate_crops_batch([img], [bad], size=(94, 24))


def test_quad_rows_accepts_lists_arrays_and_tensors():
    q = [[1, 1], [10, 1], [10, 8], [1, 8]]
    want = np.array([[1, 1, 10, 1, 10, 8, 1, 8]], dtype=np.float64)
    for qs in ([q], np.array([q], dtype=np.float32), want, torch.tensor([q], dtype=torch.float32), torch.from_numpy(want)):
        got = rectify._quad_rows('t', 0, qs)
        assert got.dtype == np.float64 and np.array_equal(got, want)
    for empty in ([], np.zeros((0, 8)), np.zeros((0, 4, 2)), torch.zeros(0, 8)):
        assert rectify._quad_rows('t', 0, empty).shape == (0, 8)


def test_detect_plate_crops_python_argument_checks():
    """Float frames, a missing or invalid size, a DenseBox net (no landmarks) are refused before any device work."""
    import densebox_amd as D
    from densebox_amd import decode as DC, synth
    lm = D.DenseBoxLM(synth.vgg19_standin(seed=0)).eval()
    frames = torch.zeros(2, 64, 64, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='uint8'):
        lm.detect_plate_crops(torch.zeros(2, 3, 64, 64), size=(94, 24))
    with pytest.raises(RuntimeError, match='uint8'):
        lm.detect_plate_crops([torch.zeros(64, 64, 3)], size=(94, 24))
    with pytest.raises(RuntimeError, match='channels'):
        lm.detect_plate_crops(torch.zeros(2, 64, 64, 4, dtype=torch.uint8), size=(94, 24))
    with pytest.raises(TypeError, match='size'):                           # keyword-only, no default
        lm.detect_plate_crops(frames)
    with pytest.raises(TypeError, match='size'):
        DC.detect_plate_crops(lm, frames)
    for bad in ((0, 24), (94, 0), (-94, 24), (94, 24, 3), None):
        with pytest.raises(RuntimeError, match='size'):
            DC.detect_plate_crops(lm, frames, size=bad)
    with pytest.raises(TypeError):                                         # the threshold decode is not part of this entry point
        lm.detect_plate_crops(frames, size=(94, 24), score_thresh=0.5)
    box = D.DenseBox(synth.vgg19_standin(seed=0)).eval()
    with pytest.raises(RuntimeError, match='DenseBox rows have no landmarks'):
        box.detect_plate_crops(frames, size=(94, 24))
