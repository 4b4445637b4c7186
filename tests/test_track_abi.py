"""CPU-side checks of the tracking entry points (dbx_track_update_batch, dbx_track_append, densebox_amd.track): the new symbols are
declared, bound and exported without an ABI bump; dbx_track and dbx_track_record have the documented layout; every bad argument is
refused on the host, with an error code and a message naming the entry point, before anything is launched; the Python argument checks
run before the device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from densebox_amd import _lib, track as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['dbx_track_update_batch', 'dbx_track_append']
NAN = float('nan')


def test_new_entry_points_are_exported_declared_and_bound_without_a_bump():
    L = _lib.lib()
    src = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, code), name + ' is not declared'
        assert name in _lib.SIGNATURES and name not in _lib.MISSING, name
        assert callable(getattr(L, name))
    assert int(re.search(r'#define\s+DBX_ABI_VERSION\s+(\d+)', src).group(1)) == L.dbx_version() == _lib.ABI_VERSION == 13
    assert re.search(r'without a bump: dbx_track, dbx_track_record, dbx_track_update_batch, dbx_track_append', src)
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert all(name in doc for name in NEW + ['dbx_track_record'])


def test_track_layouts_match_the_header():
    assert C.sizeof(_lib.Track) == 104 and C.sizeof(_lib.TrackRecord) == 112
    K = _lib.Track
    assert (K.box.offset, K.vel.offset, K.score.offset, K.best_score.offset) == (0, 32, 64, 72)
    assert [getattr(K, n).offset for n in ('id', 'hits', 'age', 'first_frame', 'last_frame', 'best_frame')] == [80, 84, 88, 92, 96, 100]
    assert (_lib.TrackRecord.stream.offset, _lib.TrackRecord.reserved.offset, _lib.TrackRecord.t.offset) == (0, 4, 8)
    assert T.TRACK.itemsize == 104 and T.RECORD.itemsize == 112
    assert [T.TRACK.fields[n][1] for n, _ in K._fields_] == [getattr(K, n).offset for n, _ in K._fields_]
    src = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    m = re.search(r'typedef struct dbx_track \{(.*?)\} dbx_track;', src, re.S)
    body = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
    assert re.findall(r'(\w+)\s+(\w+)(?:\[4\])?;', body) == [('double', 'box'), ('double', 'vel'), ('double', 'score'), ('double', 'best_score')] + [
        ('int32_t', n) for n in ('id', 'hits', 'age', 'first_frame', 'last_frame', 'best_frame')]


def _vp(a):
    return None if a is None else C.c_void_p(a)


def _update(L, dets=0x1000, det_cols=13, det_rows=80, keep=0x2000, prefix=None, batch=2, slots=8, headers=0x3000, tracks=0x4000, streams=4,
            stream0=1, max_tracks=16, iou_thresh=0.3, max_age=5, alpha=0.5, beta=0.1, birth_score=0.0, track_id=0x5000, track_slot=0x6000,
            track_hits=0x7000, retired=0x8000, tally=0x9000):
    return L.dbx_track_update_batch(_vp(dets), det_cols, det_rows, _vp(keep), _vp(prefix), batch, slots, _vp(headers), _vp(tracks), streams,
                                    stream0, max_tracks, iou_thresh, max_age, alpha, beta, birth_score, _vp(track_id), _vp(track_slot),
                                    _vp(track_hits), _vp(retired), _vp(tally), None)


def _append(L, retired=0x8000, tally=0x9000, batch=2, max_tracks=16, stream0=1, records=0xa000, capacity=100, state=0xb000):
    return L.dbx_track_append(_vp(retired), _vp(tally), batch, max_tracks, stream0, _vp(records), capacity, _vp(state), None)


@pytest.mark.parametrize('bad', [
    dict(batch=-1), dict(stream0=-1), dict(stream0=3), dict(stream0=2, batch=3, det_rows=800), dict(streams=2), dict(streams=-1),
    dict(det_cols=4), dict(det_cols=12), dict(det_cols=0),
    dict(slots=0), dict(slots=1025), dict(slots=-1), dict(slots=4096, det_rows=1 << 20),
    dict(max_tracks=0), dict(max_tracks=257), dict(max_tracks=-2),
    dict(max_age=-1),
    dict(iou_thresh=NAN), dict(alpha=NAN), dict(beta=NAN), dict(birth_score=NAN),
    dict(det_rows=15), dict(det_rows=-1), dict(det_rows=-1, prefix=0xd000),
    dict(dets=None), dict(keep=None), dict(headers=None), dict(tracks=None), dict(track_id=None), dict(track_slot=None),
    dict(track_hits=None), dict(retired=None), dict(tally=None),
])
def test_track_update_batch_rejects_bad_arguments_without_touching_the_gpu(bad):
    L = _lib.lib()
    rc = _update(L, **bad)
    assert rc == -1, bad
    msg = L.dbx_last_error()
    assert b'track_update_batch' in msg, msg
    with pytest.raises(RuntimeError, match='track_update_batch'):
        _lib.check(rc)


@pytest.mark.parametrize('bad', [
    dict(retired=None), dict(tally=None), dict(records=None), dict(state=None),
    dict(batch=-1), dict(stream0=-1), dict(max_tracks=0), dict(max_tracks=257), dict(capacity=-1),
])
def test_track_append_rejects_bad_arguments_without_touching_the_gpu(bad):
    L = _lib.lib()
    rc = _append(L, **bad)
    assert rc == -1, bad
    msg = L.dbx_last_error()
    assert b'track_append' in msg, msg
    with pytest.raises(RuntimeError, match='track_append'):
        _lib.check(rc)


def test_empty_calls_are_no_ops():
    L = _lib.lib()
    none = dict(dets=None, keep=None, headers=None, tracks=None, track_id=None, track_slot=None, track_hits=None, retired=None, tally=None)
    assert _update(L, batch=0, det_rows=0, **none) == 0
    assert _update(L, batch=0) == 0
    assert _update(L, batch=0, stream0=4) == 0                       # stream0 + 0 <= streams
    assert _append(L, batch=0, retired=None, tally=None, records=None, state=None) == 0
    assert _append(L, batch=0) == 0


def test_tracker_argument_checks():
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(RuntimeError, match='streams'):
            T.Tracker(bad)
    for bad in (0, 257, 2.0, True):
        with pytest.raises(RuntimeError, match='max_tracks'):
            T.Tracker(2, max_tracks=bad)
    for bad in (-1, 1.0, True, 1 << 31):
        with pytest.raises(RuntimeError, match='max_age'):
            T.Tracker(2, max_age=bad)
    for bad in (0, -5, 1.5, True):
        with pytest.raises(RuntimeError, match='capacity'):
            T.Tracker(2, capacity=bad)
    for name in ('iou_thresh', 'alpha', 'beta', 'birth_score'):
        for bad in (NAN, 'half', None, True):
            with pytest.raises(RuntimeError, match=name):
                T.Tracker(2, **{name: bad})
    tr = T.Tracker(3, max_tracks=256, iou_thresh=0.25, max_age=0, alpha=1, beta=0, birth_score=0.5, capacity=7)
    assert tr.params() == (256, 0.25, 0, 1.0, 0.0, 0.5, 7) and tr.streams == 3 and tr._state is None          # nothing allocated yet
    tr.reset()
    assert tr.finished().shape == (0,) and tr.finished().dtype == T.RECORD
    live = tr.live()                                                                                          # an unused tracker
    assert len(live) == 3 and all(l.shape == (0,) and l.dtype == T.TRACK for l in live) and not tr.headers().any()
    assert T.Tracker(1).birth_score == -np.inf and T.Tracker(1).serial != T.Tracker(1).serial
    assert tr._state is None


def test_update_batch_python_argument_checks():
    d5, d13 = np.zeros((2, 5)), np.zeros((2, 13))
    tr = T.Tracker(2)
    with pytest.raises(TypeError, match='tracker'):                        # keyword-only, no default
        T.update_batch([d5], [[0]])
    with pytest.raises(RuntimeError, match='one entry per image'):
        T.update_batch([d5], [[0], [1]], tracker=tr)
    with pytest.raises(RuntimeError, match='one entry per image'):
        T.update_batch([], [], tracker=tr)
    with pytest.raises(RuntimeError, match='track.Tracker'):
        T.update_batch([d5], [[0]], tracker=None)
    with pytest.raises(RuntimeError, match='stream0'):
        T.update_batch([d5, d5, d5], [[0]] * 3, tracker=tr)
    with pytest.raises(RuntimeError, match='stream0'):
        T.update_batch([d5, d5], [[0]] * 2, tracker=tr, stream0=1)
    for bad in (-1, 0.0, True):
        with pytest.raises(RuntimeError, match='stream0'):
            T.update_batch([d5], [[0]], tracker=tr, stream0=bad)
    with pytest.raises(RuntimeError, match='all alike'):
        T.update_batch([d5, d13], [[0], [0]], tracker=tr)
    with pytest.raises(RuntimeError, match='all alike'):
        T.update_batch([np.zeros((2, 6))], [[0]], tracker=tr)
    with pytest.raises(RuntimeError, match='outside'):
        T.update_batch([d5], [[2]], tracker=tr)
    with pytest.raises(RuntimeError, match='outside'):
        T.update_batch([d5], [[-1]], tracker=tr)
    with pytest.raises(RuntimeError, match='exceed'):
        T.update_batch([np.zeros((1025, 5))], [[0]], tracker=tr)
    assert tr._state is None


def test_track_batch_python_argument_checks():
    """Everything is refused before the device is touched: this machine has none."""
    import densebox_amd as D
    from densebox_amd import synth
    box = D.DenseBox(synth.vgg19_standin(seed=0)).eval()
    frames = torch.zeros(2, 64, 64, 3, dtype=torch.uint8)
    tr = T.Tracker(2)
    with pytest.raises(TypeError, match='tracker'):
        box.track_batch(frames)
    with pytest.raises(RuntimeError, match='track.Tracker'):
        box.track_batch(frames, tracker=None)
    with pytest.raises(RuntimeError, match='stream0'):
        box.track_batch(frames, tracker=tr, stream0=1)
    with pytest.raises(RuntimeError, match='stream0'):
        box.track_batch(frames, tracker=T.Tracker(1))
    with pytest.raises(RuntimeError, match='both given'):
        box.track_batch(frames, tracker=tr, K=20, score_thresh=0.5)
    with pytest.raises(RuntimeError, match='score_thresh'):
        box.track_batch(frames, tracker=tr, score_thresh=NAN)
    for bad in (0, 1025, 4096):
        with pytest.raises(RuntimeError, match='max_dets'):
            box.track_batch(frames, tracker=tr, score_thresh=0.5, max_dets=bad)
    for bad in (0, 1025, 2.5, True):
        with pytest.raises(RuntimeError, match='K='):
            box.track_batch(frames, tracker=tr, K=bad)
    with pytest.raises(RuntimeError, match='one shape'):
        box.track_batch([torch.zeros(64, 64, 3, dtype=torch.uint8), torch.zeros(32, 64, 3, dtype=torch.uint8)], tracker=tr)
    with pytest.raises(RuntimeError, match='uint8'):
        box.track_batch(torch.zeros(2, 64, 64, 4, dtype=torch.uint8), tracker=tr)
    with pytest.raises(RuntimeError, match='max_batch'):
        box.track_batch(frames, tracker=tr, max_batch=0)
    assert tr._state is None                                               # no check above reached the device
