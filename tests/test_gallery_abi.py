"""CPU-side checks of the best-shot gallery's entry points (dbx_crop_sharpness, dbx_track_gallery_update, densebox_amd.gallery): the
new symbols are declared, bound and exported without an ABI bump; dbx_shot and dbx_shot_record have the documented layout; every bad
argument is refused on the host, with an error code and a message naming the entry point, before anything is launched; the Python
argument checks run before the device is touched."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

from densebox_amd import _lib, gallery as G, track as T

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gallery_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['dbx_crop_sharpness', 'dbx_track_gallery_update']
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
    assert re.search(r'without a bump: dbx_shot, dbx_shot_record, dbx_crop_sharpness, dbx_track_gallery_update', src)
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert all(name in doc for name in NEW + ['dbx_shot', 'dbx_shot_record'])


def test_shot_layouts_match_the_header():
    S, R = _lib.Shot, _lib.ShotRecord
    assert C.sizeof(S) == 40 and C.sizeof(R) == 48
    assert [getattr(S, n).offset for n, _ in S._fields_] == [0, 8, 16, 24, 28, 32, 36]
    assert (R.stream.offset, R.slot.offset, R.shot.offset) == (0, 4, 8)
    for dt in (G.SHOT, gallery_ref.SHOT):
        assert dt.itemsize == 40 and [dt.fields[n][1] for n, _ in S._fields_] == [getattr(S, n).offset for n, _ in S._fields_]
        assert list(dt.names) == [n for n, _ in S._fields_]
    for dt in (G.SHOT_RECORD, gallery_ref.SHOT_RECORD):
        assert dt.itemsize == 48 and [dt.fields[n][1] for n in ('stream', 'slot', 'shot')] == [0, 4, 8]
    src = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct dbx_shot \{(.*?)\} dbx_shot;', src, re.S).group(1), flags=re.S)
    assert re.findall(r'(\w+)\s+(\w+);', body) == [('double', 'key'), ('double', 'score'), ('int64_t', 'sharpness')] + [
        ('int32_t', n) for n in ('id', 'frame', 'shots', 'reserved')]
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct dbx_shot_record \{(.*?)\} dbx_shot_record;', src, re.S).group(1), flags=re.S)
    assert re.findall(r'(\w+)\s+(\w+);', body) == [('int32_t', 'stream'), ('int32_t', 'slot'), ('dbx_shot', 'shot')]
    fresh = gallery_ref.fresh(7)
    assert fresh['key'] == -np.inf and np.isnan(fresh['score']) and [int(fresh[n]) for n in ('sharpness', 'id', 'frame', 'shots', 'reserved')] == [
        0, 7, -1, 0, 0]


def _vp(a):
    return None if a is None else C.c_void_p(a)


def _sharp(L, crops=0x1000, n=4, oh=24, ow=94, c=3, out=0x2000):
    return L.dbx_crop_sharpness(_vp(crops), n, oh, ow, c, _vp(out), None)


_PTRS = ('tracks', 'headers', 'track_slot', 'crops', 'ok', 'retired', 'tally', 'append_state', 'shots', 'shot_crops', 'arena',
         'arena_crops', 'gstate')


def _update(L, batch=2, slots=8, streams=4, stream0=1, max_tracks=16, oh=24, ow=94, c=3, capacity=100, policy=0, min_score=0.5, commit=1,
            **ptrs):
    p = [_vp(ptrs.get(name, 0x1000 * (i + 1))) for i, name in enumerate(_PTRS)]
    return L.dbx_track_gallery_update(*p, batch, slots, streams, stream0, max_tracks, oh, ow, c, capacity, policy, min_score, commit, None)


@pytest.mark.parametrize('bad', [
    dict(n=-1), dict(c=0), dict(c=2), dict(c=4), dict(oh=0), dict(ow=0), dict(oh=-3), dict(oh=129, ow=128), dict(oh=16385, ow=1),
    dict(oh=1 << 20, ow=1 << 20), dict(crops=None), dict(out=None),
])
def test_crop_sharpness_rejects_bad_arguments_without_touching_the_gpu(bad):
    L = _lib.lib()
    rc = _sharp(L, **bad)
    assert rc == -1, bad
    assert b'crop_sharpness' in L.dbx_last_error()
    with pytest.raises(RuntimeError, match='crop_sharpness'):
        _lib.check(rc)


@pytest.mark.parametrize('bad', [
    dict(batch=-1), dict(stream0=-1), dict(stream0=3), dict(streams=2), dict(streams=-1),
    dict(slots=0), dict(slots=1025), dict(slots=-1), dict(max_tracks=0), dict(max_tracks=257), dict(max_tracks=-2),
    dict(c=0), dict(c=2), dict(c=4), dict(oh=0), dict(ow=0), dict(ow=-1), dict(oh=129, ow=128), dict(oh=1 << 20, ow=1 << 20),
    dict(capacity=-1), dict(policy=-1), dict(policy=2), dict(min_score=NAN),
] + [{name: None} for name in _PTRS])
def test_gallery_update_rejects_bad_arguments_without_touching_the_gpu(bad):
    L = _lib.lib()
    rc = _update(L, **bad)
    assert rc == -1, bad
    assert b'track_gallery_update' in L.dbx_last_error()
    with pytest.raises(RuntimeError, match='track_gallery_update'):
        _lib.check(rc)


def test_empty_calls_are_no_ops():
    L = _lib.lib()
    assert _sharp(L, n=0) == 0
    assert _update(L, batch=0) == 0
    assert _update(L, batch=0, stream0=4) == 0
    assert _update(L, batch=0, **{name: None for name in _PTRS}) == 0


def test_plate_gallery_argument_checks():
    tr = T.Tracker(2, max_tracks=4)
    with pytest.raises(RuntimeError, match='track.Tracker'):
        G.PlateGallery(None)
    for bad in ((0, 24), (94,), (94, 24, 3), 'big', (129, 128), (16385, 1), 2.5):
        with pytest.raises(RuntimeError, match='size'):
            G.PlateGallery(tr, size=bad)
    for bad in ('sharp', 0, None):
        with pytest.raises(RuntimeError, match='policy'):
            G.PlateGallery(tr, policy=bad)
    for bad in (NAN, 'half', None, True):
        with pytest.raises(RuntimeError, match='min_score'):
            G.PlateGallery(tr, min_score=bad)
    for bad in (0, -5, 1.5, True):
        with pytest.raises(RuntimeError, match='capacity'):
            G.PlateGallery(tr, capacity=bad)
    for bad in (0, 2, 4, 3.0, True):
        with pytest.raises(RuntimeError, match='channels'):
            G.PlateGallery(tr, channels=bad)
    g = G.PlateGallery(tr, size=(128, 128), policy='score', min_score=0.5, capacity=7, channels=1)
    assert g.params() == (128, 128, 1, 1, 0.5, 7) and g.crop_bytes == 16384
    g = G.PlateGallery(tr)
    assert g.params() == (94, 24, 3, 0, -np.inf, 4096) and '(streams * max_tracks + capacity) * (oh * ow * c + 48)' in G.PlateGallery.__doc__
    g.reset()                                                              # an unused gallery: nothing to read, nothing allocated
    assert g.counters() == (0, 0, 0, 0)
    rec, crops, valid = g.finished()
    assert rec.shape == (0,) and rec.dtype == G.SHOT_RECORD and crops.shape == (0, 24, 94, 3) and valid.shape == (0,) and valid.dtype == bool
    live = g.live()
    assert len(live) == 2 and all(s.shape == (0,) and s.dtype == G.SHOT and c.shape == (0, 24, 94, 3) for s, c in live)
    assert g._live is None and tr._state is None


def test_sharpness_python_argument_checks():
    for bad in (np.zeros((2, 5, 5, 3), np.float32), np.zeros((5, 5, 3), np.uint8), np.zeros((1, 5, 5, 2), np.uint8),
                torch.zeros(1, 5, 5, 4, dtype=torch.uint8), [[1, 2]], np.zeros((1, 129, 128, 1), np.uint8), np.zeros((1, 0, 5, 1), np.uint8)):
        with pytest.raises(RuntimeError, match='sharpness'):
            G.sharpness(bad)


def test_update_batch_python_argument_checks():
    d13, im = np.zeros((2, 13)), np.zeros((32, 32, 3), np.uint8)
    tr = T.Tracker(2)
    g = G.PlateGallery(tr)
    with pytest.raises(TypeError, match='gallery'):                        # keyword-only, no default
        G.update_batch([im], [d13], [[0]], tracker=tr)
    with pytest.raises(RuntimeError, match='one entry per image'):
        G.update_batch([im], [d13], [[0], [1]], tracker=tr, gallery=g)
    with pytest.raises(RuntimeError, match='track.Tracker'):
        G.update_batch([im], [d13], [[0]], tracker=None, gallery=g)
    with pytest.raises(RuntimeError, match='PlateGallery'):
        G.update_batch([im], [d13], [[0]], tracker=tr, gallery=None)
    with pytest.raises(RuntimeError, match='another tracker'):
        G.update_batch([im], [d13], [[0]], tracker=T.Tracker(2), gallery=g)
    with pytest.raises(RuntimeError, match='stream0'):
        G.update_batch([im] * 3, [d13] * 3, [[0]] * 3, tracker=tr, gallery=g)
    with pytest.raises(RuntimeError, match='2 images for 1 entries'):
        G.update_batch([im, im], [d13], [[0]], tracker=tr, gallery=g)
    with pytest.raises(RuntimeError, match='landmarks'):                   # 5-column rows
        G.update_batch([im], [np.zeros((2, 5))], [[0]], tracker=tr, gallery=g)
    with pytest.raises(RuntimeError, match='channels'):
        G.update_batch([np.zeros((32, 32, 1), np.uint8)], [d13], [[0]], tracker=tr, gallery=g)
    with pytest.raises(RuntimeError, match='outside'):
        G.update_batch([im], [d13], [[2]], tracker=tr, gallery=g)
    with pytest.raises(RuntimeError, match='exceed'):
        G.update_batch([im], [np.zeros((1025, 13))], [[0]], tracker=tr, gallery=g)
    assert tr._state is None and g._live is None


def test_track_plate_crops_python_argument_checks():
    """Everything is refused before the device is touched: this machine has none."""
    import densebox_amd as D
    from densebox_amd import synth
    net = D.DenseBoxLMLOC(synth.vgg19_standin(seed=0)).eval()
    frames = torch.zeros(2, 64, 64, 3, dtype=torch.uint8)
    tr = T.Tracker(2)
    g = G.PlateGallery(tr)
    with pytest.raises(TypeError, match='gallery'):
        net.track_plate_crops(frames, tracker=tr)
    with pytest.raises(TypeError, match='score_thresh'):                   # top-K only, as detect_plate_crops
        net.track_plate_crops(frames, tracker=tr, gallery=g, score_thresh=0.5)
    with pytest.raises(RuntimeError, match='landmarks'):
        D.DenseBox(synth.vgg19_standin(seed=0)).eval().track_plate_crops(frames, tracker=tr, gallery=g)
    with pytest.raises(RuntimeError, match='uint8'):
        net.track_plate_crops(torch.zeros(2, 3, 64, 64), tracker=tr, gallery=g)
    with pytest.raises(RuntimeError, match='uint8'):
        net.track_plate_crops([torch.zeros(3, 64, 64)], tracker=tr, gallery=g)
    with pytest.raises(RuntimeError, match='one shape'):
        net.track_plate_crops([torch.zeros(64, 64, 3, dtype=torch.uint8), torch.zeros(32, 64, 3, dtype=torch.uint8)], tracker=tr, gallery=g)
    with pytest.raises(RuntimeError, match='stream0'):
        net.track_plate_crops(frames, tracker=tr, gallery=g, stream0=1)
    with pytest.raises(RuntimeError, match='PlateGallery'):
        net.track_plate_crops(frames, tracker=tr, gallery=None)
    with pytest.raises(RuntimeError, match='another tracker'):
        net.track_plate_crops(frames, tracker=T.Tracker(2), gallery=g)
    with pytest.raises(RuntimeError, match='channels'):
        net.track_plate_crops(frames, tracker=tr, gallery=G.PlateGallery(tr, channels=1))
    for bad in (0, 1025, 2.5, True):
        with pytest.raises(RuntimeError, match='K='):
            net.track_plate_crops(frames, tracker=tr, gallery=g, K=bad)
    with pytest.raises(RuntimeError, match='max_batch'):
        net.track_plate_crops(frames, tracker=tr, gallery=g, max_batch=0)
    assert tr._state is None and g._live is None                           # no check above reached the device
