"""dbx_nv12_host on the CPU (no GPU): the pixel functions the kernels run, compiled for the host, are bit for bit the NumPy restatement
(tests/nv12_ref.py) in both directions -- frames from one block to several tiles, pitches w, w + 1 and w + 13, both byte orders, the four
variants, nothing written in a pitch gap; the struct sizes and offsets the header states; every refusal."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from densebox_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nv12_ref as N  # noqa: E402

SIZES = [(2, 2), (2, 4), (4, 2), (16, 64), (18, 66), (34, 130)]
FILL = 0xEE


def _params(standard=601, rng='limited', order='rgb'):
    return _lib.Nv12Params(standard, {'limited': 0, 'full': 1}[rng], {'rgb': 0, 'bgr': 1}[order], 0)


class Planes:
    """the three planes of one h x w frame as pitched host arrays filled with FILL; extra: bytes added to each row's pitch"""

    def __init__(self, h, w, extra):
        self.h, self.w = h, w
        self.y = np.full((h, w + extra), FILL, np.uint8)
        self.uv = np.full((h // 2, w + extra), FILL, np.uint8)
        self.rgb = np.full((h, 3 * w + extra), FILL, np.uint8)

    def record(self):
        return _lib.Nv12Frame(self.y.ctypes.data, self.uv.ctypes.data, self.rgb.ctypes.data, self.h, self.w, self.y.shape[1],
                              self.uv.shape[1], self.rgb.shape[1], 0)

    def set_nv12(self, frame):
        self.y[:, :self.w], self.uv[:, :self.w] = frame[:self.h], frame[self.h:]

    def nv12(self):
        return np.concatenate([self.y[:, :self.w], self.uv[:, :self.w]])

    def image(self):
        return self.rgb[:, :3 * self.w].reshape(self.h, self.w, 3)

    def gaps_untouched(self):
        return bool((self.y[:, self.w:] == FILL).all() and (self.uv[:, self.w:] == FILL).all() and (self.rgb[:, 3 * self.w:] == FILL).all())


def _host(rec, par, direction):
    return _lib.lib().dbx_nv12_host(C.byref(rec), C.byref(par), direction)


def test_struct_sizes_and_offsets():
    F, P, J = _lib.Nv12Frame, _lib.Nv12Params, _lib.ResizeJobNv12
    assert C.sizeof(F) == 48 and [getattr(F, n).offset for n, _ in F._fields_] == [0, 8, 16, 24, 28, 32, 36, 40, 44]
    assert C.sizeof(P) == 16 and [getattr(P, n).offset for n, _ in P._fields_] == [0, 4, 8, 12]
    assert C.sizeof(J) == 88 and [getattr(J, n).offset for n, _ in J._fields_] == [0, 8, 16, 20] + list(range(24, 76, 4)) + [80]
    assert _lib.lib().dbx_resize_batch_nv12_workspace_bytes(-1) == -1
    assert _lib.lib().dbx_resize_batch_nv12_workspace_bytes(3) >= 3 * 112 + 16


@pytest.mark.parametrize('h,w', SIZES)
def test_host_equals_restatement_both_directions(h, w):
    rs = np.random.RandomState(h * 1000 + w)
    for extra in (0, 1, 13):
        for std, rng in N.VARIANTS:
            for order in ('rgb', 'bgr'):
                par = _params(std, rng, order)
                frame = rs.randint(0, 256, size=(h * 3 // 2, w)).astype(np.uint8)
                p = Planes(h, w, extra)
                p.set_nv12(frame)
                assert _host(p.record(), par, 0) == 0, _lib.lib().dbx_last_error()
                assert np.array_equal(p.image(), N.nv12_to_rgb(frame, None, std, rng, order)), (extra, std, rng, order)
                assert np.array_equal(p.nv12(), frame) and p.gaps_untouched()
                img = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
                q = Planes(h, w, extra)
                q.rgb[:, :3 * w] = img.reshape(h, 3 * w)
                assert _host(q.record(), par, 1) == 0, _lib.lib().dbx_last_error()
                assert np.array_equal(q.nv12(), N.rgb_to_nv12(img, std, rng, order)), (extra, std, rng, order)
                assert np.array_equal(q.image(), img) and q.gaps_untouched()


def test_every_refusal():
    L = _lib.lib()
    good = Planes(4, 6, 2)

    def refused(word, direction=0, par=None, **fields):
        rec = good.record()
        for k, v in fields.items():
            setattr(rec, k, v)
        rc = _host(rec, par or _params(), direction)
        assert rc == -1 and word in L.dbx_last_error(), (fields, rc, L.dbx_last_error())
    for d in (0, 1):
        refused(b'odd', d, h=3)
        refused(b'odd', d, w=5)
        refused(b'odd', d, h=0)
        refused(b'odd', d, w=-2)
        refused(b'pitch', d, pitch_y=5)
        refused(b'pitch', d, pitch_uv=5)
        refused(b'pitch', d, pitch_rgb=17)
        refused(b'null', d, y=None)
        refused(b'null', d, uv=None)
        refused(b'null', d, rgb=None)
        refused(b'standard', d, par=_lib.Nv12Params(602, 0, 0, 0))
        refused(b'range', d, par=_lib.Nv12Params(601, 2, 0, 0))
        refused(b'order', d, par=_lib.Nv12Params(709, 1, -1, 0))
    refused(b'direction', 2)
    assert L.dbx_nv12_host(None, C.byref(_params()), 0) == -1 and b'null' in L.dbx_last_error()
    assert L.dbx_nv12_host(C.byref(good.record()), None, 0) == -1 and b'null' in L.dbx_last_error()
    assert (good.y == FILL).all() and (good.uv == FILL).all() and (good.rgb == FILL).all()
    # the launches refuse bad arguments on the host, before anything is queued
    assert L.dbx_nv12_to_rgb_batch(C.c_void_p(0x1000), 1, 4, 4, C.byref(_lib.Nv12Params(600, 0, 0, 0)), None) == -1
    assert L.dbx_rgb_to_nv12_batch(C.c_void_p(0x1000), -1, 4, 4, C.byref(_params()), None) == -1
    assert L.dbx_rgb_to_nv12_batch(None, 1, 4, 4, C.byref(_params()), None) == -1
    assert L.dbx_nv12_to_rgb_batch(C.c_void_p(0x1000), 1, 0, 4, C.byref(_params()), None) == -1
    assert L.dbx_nv12_to_rgb_batch(C.c_void_p(0x1000), 0, 4, 4, C.byref(_params()), None) == 0
    job = _lib.ResizeJobNv12(0x1000, 0x2000, 8, 8, 4, 8, 1, 1, 3, 3, 0, 0, 0, 0, 128, 5, 5, 0)

    def job_refused(word, **fields):
        j = _lib.ResizeJobNv12.from_buffer_copy(job)
        for k, v in fields.items():
            setattr(j, k, v)
        rc = L.dbx_resize_cubic_batch_nv12(C.byref(j), 1, C.byref(_params()), C.c_void_p(0x3000), C.c_void_p(0x4000), None)
        assert rc == -1 and word in L.dbx_last_error(), (fields, rc, L.dbx_last_error())
    job_refused(b'odd', sh=5)
    job_refused(b'odd', sw=7)
    job_refused(b'pitch', pitch_y=7)
    job_refused(b'pitch', pitch_uv=6)
    job_refused(b'null', y=None)
    job_refused(b'null', uv=None)
    job_refused(b'crop', cx0=6)
    job_refused(b'pad_value', pad_value=256)
    job_refused(b'negative', pad_l=-1)
    job_refused(b'dst_off', dst_off=-1)
    job_refused(b'non-positive', dw=0)
    assert L.dbx_resize_cubic_batch_nv12(C.byref(job), 1, None, C.c_void_p(0x3000), C.c_void_p(0x4000), None) == -1
    assert L.dbx_resize_cubic_batch_nv12(C.byref(job), 0, C.byref(_params()), None, None, None) == 0
