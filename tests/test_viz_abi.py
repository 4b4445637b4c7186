"""CPU-side checks of the overlay's entry points (dbx_draw_overlay_batch, dbx_overlay_font, dbx_overlay_label, densebox_amd.viz): the new
symbols are declared, bound and exported; dbx_overlay_frame and dbx_overlay_style have the documented layout; every bad argument is
refused on the host, with an error code and a message naming the entry point, before anything is launched; the Python argument checks
run before the device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from densebox_amd import _lib, track as T, viz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['dbx_draw_overlay_batch', 'dbx_overlay_font', 'dbx_overlay_label']


def test_new_entry_points_are_exported_declared_and_bound():
    L = _lib.lib()
    src = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, code), name + ' is not declared'
        assert name in _lib.SIGNATURES and name not in _lib.MISSING, name
        assert callable(getattr(L, name))
    assert int(re.search(r'#define\s+DBX_ABI_VERSION\s+(\d+)', src).group(1)) == L.dbx_version() == _lib.ABI_VERSION
    assert re.search(r'without a bump: dbx_overlay_frame, dbx_overlay_style, dbx_draw_overlay_batch, dbx_overlay_font, dbx_overlay_label', src)
    assert re.search(r'parity with cv2\.rectangle / putText / circle is[\s*]+unpinned', src)
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert all(name in doc for name in NEW + ['OverlayFrame', 'OverlayStyle'])
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert 'dbx_draw_overlay_batch' in design and 'annotate_batch' in open(os.path.join(ROOT, 'README.md')).read()


def test_overlay_layouts_match_the_header():
    F, S = _lib.OverlayFrame, _lib.OverlayStyle
    assert C.sizeof(F) == 24 and [getattr(F, n).offset for n, _ in F._fields_] == [0, 8, 16, 20]
    assert C.sizeof(S) == 28 and [getattr(S, n).offset for n, _ in S._fields_] == [0, 4, 8, 12, 16, 20, 24]
    src = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct dbx_overlay_style \{(.*?)\} dbx_overlay_style;', src, re.S).group(1), flags=re.S)
    assert re.findall(r'int32_t\s+(\w+);', body) == ['thickness', 'radius', 'font_scale', 'inset_scale']
    assert re.search(r'uint8_t box_color\[4\], text_color\[4\], mark_color\[4\];', body)
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct dbx_overlay_frame \{(.*?)\} dbx_overlay_frame;', src, re.S).group(1), flags=re.S)
    assert re.findall(r'(\w+\*?)\s+(\w+(?:, \w+)?);', body) == [('uint8_t*', 'src'), ('uint8_t*', 'dst'), ('int32_t', 'h, w')]
    r = viz.Style().record()
    assert (list(r.box_color), list(r.text_color), list(r.mark_color)) == ([0, 215, 255, 0], [225, 255, 255, 0], [0, 0, 255, 0])
    assert (r.thickness, r.radius, r.font_scale, r.inset_scale) == (2, 5, 2, 1)                 # viz_result's values


def _vp(a):
    return None if a is None else C.c_void_p(a)


_STYLE = dict(thickness=2, radius=5, font_scale=2, inset_scale=1)


def _draw(L, frames=0x1000, batch=2, c=3, max_h=64, max_w=64, dets=0x2000, det_cols=13, det_rows=20, keep=0x3000, prefix=None, slots=10,
          track_id=0x4000, crops=0x5000, ok=0x6000, ow=94, oh=24, style=True, **st):
    s = viz.Style().record()
    for k, v in st.items():
        assert k in _STYLE
        setattr(s, k, v)
    return L.dbx_draw_overlay_batch(_vp(frames), batch, c, max_h, max_w, _vp(dets), det_cols, det_rows, _vp(keep), _vp(prefix), slots,
                                    _vp(track_id), _vp(crops), _vp(ok), ow, oh, C.byref(s) if style else None, None)


@pytest.mark.parametrize('bad', [
    dict(batch=-1), dict(c=0), dict(c=5), dict(c=-1), dict(max_h=0), dict(max_w=0), dict(max_h=-4), dict(det_cols=4), dict(det_cols=12),
    dict(slots=0), dict(slots=1025), dict(slots=-1), dict(det_rows=-1), dict(det_rows=19), dict(det_rows=-1, prefix=0x7000),
    dict(thickness=0), dict(thickness=17), dict(radius=-2), dict(radius=33), dict(font_scale=-1), dict(font_scale=9),
    dict(inset_scale=0), dict(inset_scale=9), dict(crops=None), dict(ok=None), dict(ow=0), dict(oh=0), dict(ow=-3),
    dict(frames=None), dict(dets=None), dict(keep=None), dict(style=False),
    dict(max_h=(1 << 31) - 1, max_w=(1 << 31) - 1), dict(max_h=1 << 20, max_w=1 << 16), dict(batch=65536, det_rows=655360),
])
def test_draw_overlay_rejects_bad_arguments_without_touching_the_gpu(bad):
    L = _lib.lib()
    rc = _draw(L, **bad)
    assert rc == -1, bad
    assert b'draw_overlay_batch' in L.dbx_last_error()
    with pytest.raises(RuntimeError, match='draw_overlay_batch'):
        _lib.check(rc)


def test_empty_call_is_a_no_op_and_the_optional_pointers_are_optional():
    L = _lib.lib()
    assert _draw(L, batch=0) == 0
    assert _draw(L, batch=0, det_rows=0, track_id=None, crops=None, ok=None, ow=0, oh=0) == 0
    assert _draw(L, batch=0, det_rows=0, prefix=0x7000) == 0
    assert _draw(L, batch=0, thickness=16, radius=32, font_scale=8, inset_scale=8, slots=1024) == 0
    assert _draw(L, batch=0, thickness=1, radius=-1, font_scale=0, inset_scale=1, slots=1, c=1, det_cols=5) == 0


def test_style_argument_checks():
    for bad in (dict(thickness=0), dict(thickness=17), dict(thickness=2.0), dict(thickness=True), dict(radius=-2), dict(radius=33),
                dict(font_scale=-1), dict(font_scale=9), dict(inset_scale=0), dict(inset_scale=9), dict(box_color=()),
                dict(box_color=(1, 2, 3, 4, 5)), dict(text_color=(256, 0, 0)), dict(mark_color=(-1,)), dict(mark_color=7),
                dict(box_color=(0.5, 0, 0))):
        with pytest.raises(RuntimeError, match='Style'):
            viz.Style(**bad)
    s = viz.Style(box_color=(1, 2), thickness=16, radius=-1, font_scale=0, inset_scale=8)
    assert s.key() == ((1, 2, 0, 0), (225, 255, 255, 0), (0, 0, 255, 0), 16, -1, 0, 8)
    assert s.key() != viz.Style().key() and viz.Style().key() == viz.Style().key()


def test_draw_batch_python_argument_checks():
    """Everything is refused before the device is touched: this machine has none."""
    im, d13 = np.zeros((32, 32, 3), np.uint8), np.zeros((2, 13))
    with pytest.raises(RuntimeError, match='uint8'):
        viz.draw_batch([im.astype(np.float32)], [d13], [[0]])
    with pytest.raises(RuntimeError, match='one entry per image'):
        viz.draw_batch([im], [d13], [[0], [1]])
    with pytest.raises(RuntimeError, match=r'\[n, 5\] or \[n, 13\]'):
        viz.draw_batch([im], [np.zeros((2, 6))], [[0]])
    with pytest.raises(RuntimeError, match='all alike'):
        viz.draw_batch([im, im], [d13, np.zeros((2, 5))], [[0], [0]])
    with pytest.raises(RuntimeError, match='outside'):
        viz.draw_batch([im], [d13], [[2]])
    with pytest.raises(RuntimeError, match='exceed'):
        viz.draw_batch([im], [np.zeros((1025, 13))], [[0]])
    with pytest.raises(RuntimeError, match='one id per kept row'):
        viz.draw_batch([im], [d13], [[0, 1]], track_ids=[[4]])
    with pytest.raises(RuntimeError, match='together'):
        viz.draw_batch([im], [d13], [[0]], crops=[np.zeros((1, 4, 8, 3), np.uint8)])
    with pytest.raises(RuntimeError, match='one size'):
        viz.draw_batch([im, im], [d13, d13], [[0], [0]], crops=[np.zeros((1, 4, 8, 3), np.uint8), np.zeros((1, 5, 8, 3), np.uint8)],
                       ok=[[1], [1]])
    with pytest.raises(RuntimeError, match='one size'):                                       # the frames' channel count
        viz.draw_batch([im], [d13], [[0]], crops=[np.zeros((1, 4, 8, 1), np.uint8)], ok=[[1]])
    with pytest.raises(RuntimeError, match='one entry per kept row'):
        viz.draw_batch([im], [d13], [[0, 1]], crops=[np.zeros((1, 4, 8, 3), np.uint8)], ok=[[1]])
    with pytest.raises(RuntimeError, match='viz.Style'):
        viz.draw_batch([im], [d13], [[0]], style=dict(thickness=2))


def test_annotate_batch_python_argument_checks():
    import densebox_amd as D
    from densebox_amd import synth
    net = D.DenseBoxLMLOC(synth.vgg19_standin(seed=0)).eval()
    frames = torch.zeros(2, 64, 64, 3, dtype=torch.uint8)
    tr = T.Tracker(2)
    with pytest.raises(TypeError, match='score_thresh'):                                      # top-K only, as detect_plate_crops
        net.annotate_batch(frames, score_thresh=0.5)
    with pytest.raises(RuntimeError, match='landmarks'):
        D.DenseBox(synth.vgg19_standin(seed=0)).eval().annotate_batch(frames, inset=(94, 24))
    with pytest.raises(RuntimeError, match='uint8'):
        net.annotate_batch(torch.zeros(2, 3, 64, 64))
    with pytest.raises(RuntimeError, match='one shape'):
        net.annotate_batch([np.zeros((64, 64, 3), np.uint8), np.zeros((32, 64, 3), np.uint8)])
    with pytest.raises(RuntimeError, match='stream0'):
        net.annotate_batch(frames, tracker=tr, stream0=1)
    with pytest.raises(RuntimeError, match='track.Tracker'):
        net.annotate_batch(frames, tracker='yes')
    for bad in (0, 1025, 2.5, True):
        with pytest.raises(RuntimeError, match='K='):
            net.annotate_batch(frames, K=bad)
    with pytest.raises(RuntimeError, match='max_batch'):
        net.annotate_batch(frames, max_batch=0)
    for bad in ((0, 24), (94,), 'big'):
        with pytest.raises(RuntimeError, match='size'):
            net.annotate_batch(frames, inset=bad)
    with pytest.raises(RuntimeError, match='viz.Style'):
        net.annotate_batch(frames, style='red')
    assert tr._state is None                                                                  # no check above reached the device
