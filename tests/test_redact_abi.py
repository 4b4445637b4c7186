"""CPU-side checks of the redaction's entry points (dbx_redact_batch, dbx_redact_host, densebox_amd.redact): the new symbols are declared,
bound and exported; dbx_redact_style has the documented layout; every bad argument is refused on the host, with an error code and a
message naming the entry point, before anything is launched; dbx_redact_host -- the kernel's region build, coverage test and value rules
compiled for the host -- equals the NumPy restatement (tests/redact_ref.py) bit for bit on the crafted rows; the Python argument checks run
before the device is touched."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

from densebox_amd import _lib, redact, track as T

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import redact_cases as RC  # noqa: E402
import redact_ref as V  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['dbx_redact_batch', 'dbx_redact_host']


def test_new_entry_points_are_exported_declared_and_bound():
    L = _lib.lib()
    src = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, code), name + ' is not declared'
        assert name in _lib.SIGNATURES and name not in _lib.MISSING, name
        assert callable(getattr(L, name))
    assert int(re.search(r'#define\s+DBX_ABI_VERSION\s+(\d+)', src).group(1)) == L.dbx_version() == _lib.ABI_VERSION
    assert re.search(r'without a bump: dbx_redact_style, dbx_redact_batch, dbx_redact_host', src)
    assert 'dbx_redact_batch' in open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert 'redact_batch' in open(os.path.join(ROOT, 'README.md')).read()
    assert all(name in open(os.path.join(ROOT, 'INTEGRATION.md')).read() for name in NEW)


def test_style_layout_matches_the_header():
    S = _lib.RedactStyle
    assert C.sizeof(S) == 40 and [getattr(S, n).offset for n, _ in S._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32]
    src = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct dbx_redact_style \{(.*?)\} dbx_redact_style;', src, re.S).group(1), flags=re.S)
    assert re.findall(r'(\w+)\s+(\w+)(?:\[4\])?;', body) == [
        ('uint8_t', 'color'), ('int32_t', 'method'), ('int32_t', 'shape'), ('int32_t', 'cell'), ('int32_t', 'radius'), ('int32_t', 'grow'),
        ('int32_t', 'grow_pct'), ('int32_t', 'coast'), ('double', 'min_score')]
    assert [n for n, _ in S._fields_] == ['color', 'method', 'shape', 'cell', 'radius', 'grow', 'grow_pct', 'coast', 'min_score']
    r = redact.Redaction().record(13, 5)
    assert (list(r.color), r.method, r.shape, r.cell, r.radius, r.grow, r.grow_pct, r.coast, r.min_score) == (
        [0, 0, 0, 0], 1, 1, 12, 8, 2, 10, 5, -float('inf'))
    r = redact.Redaction(method='blur', shape='box', coast=0, color=(1, 2, 3)).record(13, 5)
    assert (list(r.color), r.method, r.shape, r.coast) == ([1, 2, 3, 0], 2, 0, 0)
    assert redact.Redaction().record(5, 2).shape == 0 and redact.Redaction(shape='quad').record(5, 2).shape == 1


def _vp(a):
    return None if a is None else C.c_void_p(a)


_FIELDS = ('method', 'shape', 'cell', 'radius', 'grow', 'grow_pct', 'coast', 'min_score')


def _record(st):
    s = redact.Redaction().record(13, 5)
    for k, v in st.items():
        assert k in _FIELDS
        setattr(s, k, v)
    return s


def _redact(L, frames=0x1000, batch=2, c=3, max_h=64, max_w=64, dets=0x2000, det_cols=13, det_rows=20, keep=0x3000, prefix=None, slots=10,
            tracks=0x4000, streams=4, stream0=1, max_tracks=64, style=True, **st):
    s = _record(st)
    return L.dbx_redact_batch(_vp(frames), batch, c, max_h, max_w, _vp(dets), det_cols, det_rows, _vp(keep), _vp(prefix), slots, _vp(tracks),
                              streams, stream0, max_tracks, C.byref(s) if style else None, None)


_BAD_STYLE = [dict(method=-1), dict(method=3), dict(shape=-1), dict(shape=2), dict(cell=1), dict(cell=33), dict(radius=0), dict(radius=17),
              dict(grow=-1), dict(grow=65), dict(grow_pct=-1), dict(grow_pct=101), dict(coast=-1), dict(min_score=float('nan'))]


@pytest.mark.parametrize('bad', [
    dict(batch=-1), dict(c=0), dict(c=5), dict(c=-1), dict(max_h=0), dict(max_w=0), dict(max_h=-4), dict(det_cols=4), dict(det_cols=12),
    dict(slots=0), dict(slots=1025), dict(slots=-1), dict(det_rows=-1), dict(det_rows=19), dict(det_rows=-1, prefix=0x7000),
    dict(stream0=-1), dict(stream0=3), dict(streams=2), dict(max_tracks=0), dict(max_tracks=257), dict(max_tracks=-1),
    dict(frames=None), dict(dets=None), dict(keep=None), dict(style=False),
    dict(max_h=(1 << 31) - 1, max_w=(1 << 31) - 1), dict(max_h=1 << 20, max_w=1 << 16), dict(batch=65536, det_rows=655360, streams=1 << 17),
] + _BAD_STYLE)
def test_redact_batch_rejects_bad_arguments_without_touching_the_gpu(bad):
    L = _lib.lib()
    rc = _redact(L, **bad)
    assert rc == -1, bad
    assert b'redact_batch' in L.dbx_last_error()
    with pytest.raises(RuntimeError, match='redact_batch'):
        _lib.check(rc)


def test_empty_call_is_a_no_op_and_the_optional_pointers_are_optional():
    L = _lib.lib()
    assert _redact(L, batch=0) == 0
    assert _redact(L, batch=0, det_rows=0, tracks=None, streams=0, stream0=-1, max_tracks=0) == 0        # without tracks they are not read
    assert _redact(L, batch=0, det_rows=0, prefix=0x7000) == 0
    assert _redact(L, batch=0, method=2, shape=1, cell=32, radius=16, grow=64, grow_pct=100, coast=(1 << 31) - 1, slots=1024, max_tracks=256) == 0
    assert _redact(L, batch=0, method=0, shape=0, cell=2, radius=1, grow=0, grow_pct=0, coast=0, slots=1, c=1, det_cols=5, max_tracks=1,
                   min_score=float('inf')) == 0


# ------------------------------------------------------------------------------------------------------------ dbx_redact_host
def _host(img, rows, keep, tracks, style, into=None, rc_only=False, over=None):
    """dbx_redact_host on one frame; keep: the list of row numbers"""
    img = np.ascontiguousarray(img)
    h, w, c = img.shape
    rows = np.ascontiguousarray(rows, np.float64)
    kl = np.asarray(keep, np.int32)
    out = np.full(img.shape, 0xEE, np.uint8) if into is None else into
    rec = redact.Redaction(**style).record(rows.shape[1], 0)
    a = dict(src=img.ctypes.data, dst=out.ctypes.data, h=h, w=w, c=c, rows=rows.ctypes.data, det_cols=rows.shape[1], n=rows.shape[0],
             keep=kl.ctypes.data if kl.size else None, k=kl.size, tracks=None if tracks is None else tracks.ctypes.data,
             ntracks=0 if tracks is None else tracks.size, style=C.byref(rec))
    a.update(over or {})
    rc = _lib.lib().dbx_redact_host(_vp(a['src']), _vp(a['dst']), a['h'], a['w'], a['c'], _vp(a['rows']), a['det_cols'], a['n'], _vp(a['keep']),
                                    a['k'], _vp(a['tracks']), a['ntracks'], a['style'])
    if rc_only:
        return rc
    _lib.check(rc)
    return out


def test_redact_host_refusals():
    L = _lib.lib()
    img, rows, tr = np.zeros((4, 6, 3), np.uint8), np.zeros((2, 13)), RC.tracks(4, 6)
    fill = dict(method='fill')
    assert _host(img, rows, [0], tr, fill, rc_only=True) == 0
    for over in (dict(src=None), dict(dst=None), dict(h=0), dict(w=-1), dict(c=0), dict(c=5), dict(det_cols=6), dict(n=-1), dict(k=-1),
                 dict(rows=None), dict(keep=None, k=1), dict(ntracks=0), dict(ntracks=257), dict(style=None)):
        assert _host(img, rows, [0], tr, fill, rc_only=True, over=over) == -1, over
        assert b'redact_host' in L.dbx_last_error()
    for bad in _BAD_STYLE:
        rec = _record(bad)
        assert _host(img, rows, [0], tr, fill, rc_only=True, over=dict(style=C.byref(rec))) == -1, bad
    for method in ('pixelate', 'blur'):                                         # in place: fill only
        assert _host(img, rows, [0], None, dict(method=method), into=img, rc_only=True) == -1
    assert _host(img, rows, [], None, fill, rc_only=True, over=dict(rows=None, n=0)) == 0  # a frame without rows


@pytest.mark.parametrize('c', [1, 3, 4])
@pytest.mark.parametrize('h,w', RC.SIZES)
def test_redact_host_equals_the_restatement_on_crafted_rows(h, w, c):
    rs = np.random.RandomState(h * 100 + w + c)
    img = rs.randint(0, 256, size=(h, w, c)).astype(np.uint8)
    rows, n = RC.crafted(h, w), RC.crafted(h, w).shape[0]
    lists = [RC.effective(raw, n, n) for raw in RC.keep_lists(h, w)]
    for si, st in enumerate(RC.styles()):
        for tr in (None, RC.tracks(h, w)):
            for li, kl in enumerate(lists if si < 4 else lists[:1]):
                count = V.covered(h, w, rows, kl, tr, st)
                # no case passes by being all copy or all fill
                assert (count > 0).any() and ((count == 0).any() or (h, w) == (1, 1)), (st, tr is not None, li)
                if h >= 17:
                    assert (count >= 2).any()
                want = V.redact(img, rows, kl, tr, st)
                got = _host(img, rows, kl, tr, st)
                assert np.array_equal(got, want), (st, tr is not None, li, np.argwhere((got != want).any(axis=2))[:5])
                if st['method'] == 'fill' and h >= 17:
                    assert not np.array_equal(got, img)
    # five columns: a quad style falls back to boxes; in place under fill only the covered bytes change
    st = dict(RC.BASE, method='fill', shape='quad')
    five = _host(img, rows[:, :5], lists[0], None, st)
    assert np.array_equal(five, V.redact(img, rows[:, :5], lists[0], None, st))
    assert np.array_equal(five, V.redact(img, rows, lists[0], None, dict(st, shape='box')))
    buf = img.copy()
    assert _host(buf, rows, lists[0], None, st, into=buf) is buf and np.array_equal(buf, V.redact(img, rows, lists[0], None, st))
    # the keep count is clamped to the rows: entries past min(k, n) are not walked
    long = lists[0] + [0] * 5
    assert np.array_equal(_host(img, rows[:3], long, None, st), V.redact(img, rows[:3], long[:3], None, st))


def test_track_rules_through_the_host_build():
    h, w = 17, 33
    img = np.random.RandomState(5).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    tr, none = RC.tracks(h, w), np.zeros((0, 5))
    for coast in (0, 1, RC.COAST, RC.COAST + 1):
        st = dict(RC.BASE, method='fill', coast=coast)
        got = _host(img, none, [], tr, st)
        assert np.array_equal(got, V.redact(img, none, [], tr, st))
        assert (got != img).any() == (coast > 0)
    a, b = (_host(img, none, [], tr, dict(RC.BASE, method='fill', coast=k)) for k in (1, RC.COAST))
    assert (a != img).sum() < (b != img).sum()                                  # the slot of age COAST joins


# ------------------------------------------------------------------------------------------------------------ the Python layer
def test_redaction_argument_checks():
    for bad in (dict(method='smear'), dict(method=1), dict(shape='circle'), dict(shape=0), dict(cell=1), dict(cell=33), dict(cell=4.0),
                dict(cell=True), dict(radius=0), dict(radius=17), dict(grow=-1), dict(grow=65), dict(grow_pct=-1), dict(grow_pct=101),
                dict(coast=-1), dict(coast=1.5), dict(coast=1 << 31), dict(min_score=float('nan')), dict(min_score='high'), dict(color=()),
                dict(color=(1, 2, 3, 4, 5)), dict(color=(256, 0, 0)), dict(color=7)):
        with pytest.raises(RuntimeError, match='Redaction'):
            redact.Redaction(**bad)
    s = redact.Redaction(method='fill', shape='box', cell=32, radius=16, color=(1, 2), grow=64, grow_pct=100, coast=0, min_score=0.5)
    assert s.key() == ('fill', 'box', 32, 16, (1, 2, 0, 0), 64, 100, 0, 0.5)
    assert s.key() != redact.Redaction().key() and redact.Redaction().key() == redact.Redaction().key()


def test_redact_batch_python_argument_checks():
    """Everything is refused before the device is touched: this machine has none."""
    im, d13 = np.zeros((32, 32, 3), np.uint8), np.zeros((2, 13))
    with pytest.raises(RuntimeError, match='uint8'):
        redact.redact_batch([im.astype(np.float32)], [d13], [[0]])
    with pytest.raises(RuntimeError, match='one entry per image'):
        redact.redact_batch([im], [d13], [[0], [1]])
    with pytest.raises(RuntimeError, match=r'\[n, 5\] or \[n, 13\]'):
        redact.redact_batch([im], [np.zeros((2, 6))], [[0]])
    with pytest.raises(RuntimeError, match='outside'):
        redact.redact_batch([im], [d13], [[2]])
    with pytest.raises(RuntimeError, match='exceed'):
        redact.redact_batch([im], [np.zeros((1025, 13))], [[0]])
    with pytest.raises(RuntimeError, match='one entry per image'):
        redact.redact_batch([im], [d13], [[0]], tracks=[np.zeros(1, T.TRACK)] * 2)
    with pytest.raises(RuntimeError, match='track.TRACK'):
        redact.redact_batch([im], [d13], [[0]], tracks=[np.zeros((1, 13))])
    with pytest.raises(RuntimeError, match='exceed 256'):
        redact.redact_batch([im], [d13], [[0]], tracks=[np.zeros(257, T.TRACK)])
    with pytest.raises(RuntimeError, match='redact.Redaction'):
        redact.redact_batch([im], [d13], [[0]], style=dict(method='fill'))


def test_net_redact_batch_python_argument_checks():
    import densebox_amd as D
    from densebox_amd import synth
    net = D.DenseBoxLMLOC(synth.vgg19_standin(seed=0)).eval()
    frames = torch.zeros(2, 64, 64, 3, dtype=torch.uint8)
    tr = T.Tracker(2)
    with pytest.raises(TypeError, match='score_thresh'):                                      # top-K only, as annotate_batch
        net.redact_batch(frames, score_thresh=0.5)
    with pytest.raises(RuntimeError, match='uint8'):
        net.redact_batch(torch.zeros(2, 3, 64, 64))
    with pytest.raises(RuntimeError, match='one shape'):
        net.redact_batch([np.zeros((64, 64, 3), np.uint8), np.zeros((32, 64, 3), np.uint8)])
    with pytest.raises(RuntimeError, match='stream0'):
        net.redact_batch(frames, tracker=tr, stream0=1)
    with pytest.raises(RuntimeError, match='track.Tracker'):
        net.redact_batch(frames, tracker='yes')
    for bad in (0, 1025, 2.5, True):
        with pytest.raises(RuntimeError, match='K='):
            net.redact_batch(frames, K=bad)
    with pytest.raises(RuntimeError, match='max_batch'):
        net.redact_batch(frames, max_batch=0)
    with pytest.raises(RuntimeError, match='redact.Redaction'):
        net.redact_batch(frames, style='black')
    assert tr._state is None                                                                  # no check above reached the device
