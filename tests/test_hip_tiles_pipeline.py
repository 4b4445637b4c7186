"""detect_tiled on the GPU against the composition a user could write before it existed: the tile pixels from tests/cubic_ref.py on the
padded crops, net.detect_batch / net.detect_batch_thresh on that tile tensor with the same max_batch and order, and the restatement
(tests/tiles_ref.py) on the host -- bit for bit.  The totals of owned and dropped rows are printed, not asserted: they depend on the
stand-in weights (tests/test_hip_tiles.py carries the coverage conditions on crafted rows)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cubic_ref                                        # noqa: E402
import tiles_ref as R                                   # noqa: E402

import densebox_amd as D                                # noqa: E402
from densebox_amd import _lib, decode as DC, synth, tiles as T, track     # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = ((96, 160), (64, 64), (40, 50), (130, 70))     # 40 x 50 is one padded tile at src 64
TILE, OVERLAP = 64, 16


def _img(rs, h, w):
    img = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    img[::7] = 0
    img[:, ::11] = 255
    return img


def _net(kind, dtype='f32'):
    net = getattr(D, kind)(synth.vgg19_standin(seed=0))
    synth.fill_params_(net, 11)
    net = net.cuda().eval()
    net.compute_dtype = dtype
    return net


_FRAMES = {}


def _frames():
    if not _FRAMES:
        rs = np.random.RandomState(41)
        _FRAMES['f'] = [_img(rs, h, w) for h, w in SHAPES]
    return _FRAMES['f']


_PIXELS = {}


def _table_and_pixels(src):
    """the call's table and its tile tensor from cubic_ref, computed once per src and left unchanged"""
    if src not in _PIXELS:
        frames = _frames()
        table = np.concatenate([R.plan(f.shape[0], f.shape[1], src, OVERLAP, b, src / TILE) for b, f in enumerate(frames)])
        px = np.stack([R.tile_pixels(frames[int(t['frame'])], t, TILE, cubic_ref) for t in table])
        _PIXELS[src] = (table, px)
    return _PIXELS[src]


def _composition(net, src, max_batch, K=10, thresh=None, rule=R.CORE, nms=0.4, only=None):
    """(per frame (rows, keep, tile index), stage) from the public calls and the restatement; only: the table indices of the tiles that run"""
    table, px = _table_and_pixels(src)
    if only is not None:
        table, px = table[only], px[only]
    x = torch.from_numpy(px)
    if thresh is None:
        per = net.detect_batch(x, K=K, nms_thresh=nms, max_batch=max_batch)
        rows, counts, rpt = np.stack([d for d, _ in per]), None, K
    else:
        per = net.detect_batch_thresh(x, thresh[0], max_dets=thresh[1], nms_thresh=nms, max_batch=max_batch)
        rpt = thresh[1]
        rows = np.zeros((len(per), rpt, per[0][0].shape[1]))
        counts = [d.shape[0] for d, _ in per]
        for t, (d, _) in enumerate(per):
            rows[t, :d.shape[0]] = d
    stage, want = R.stitch(rows, counts, table, len(SHAPES), rpt, rule, nms)
    return want, stage, table


def _totals(what, stage):
    delivered, owned = sum(m.shape[0] for m, _ in stage), sum(int(k.sum()) for _, k in stage)
    print('%s: %d tiles, %d rows delivered, %d owned, %d dropped' % (what, len(stage), delivered, owned, delivered - owned))


def _assert_same(got, want, table, what):
    first = np.concatenate([[0], np.cumsum(np.bincount(table['frame'], minlength=len(SHAPES)))])
    assert len(got) == len(want)
    for b, (g, (wd, wk, wt)) in enumerate(zip(got, want)):
        assert g[0].dtype == np.float64 and g[0].shape == wd.shape and g[0].tobytes() == wd.tobytes(), (what, b, 'rows')
        assert g[1] == wk, (what, b, 'keep')
        if len(g) > 2:
            assert (g[2] + first[b]).tolist() == wt.tolist(), (what, b, 'tile index')
            assert g[3].tobytes() == table[first[b]:first[b + 1]].astype(T.TILE_DTYPE).tobytes(), (what, b, 'plan')


@pytest.mark.parametrize('dtype', ['f32', 'f16'])
@pytest.mark.parametrize('kind', ['DenseBox', 'DenseBoxLMLOC'])
def test_detect_tiled_is_the_composition_bit_for_bit(kind, dtype):
    net = _net(kind, dtype)
    frames = _frames()
    dc = 5 if kind == 'DenseBox' else 13
    for src in (64, 32):
        by_batch = {}
        for max_batch in (4, 32):
            want, stage, table = _composition(net, src, max_batch)
            _totals('%s %s src %d max_batch %d top-K' % (kind, dtype, src, max_batch), stage)
            got = net.detect_tiled(frames, tile=TILE, src=src, overlap=OVERLAP, K=10, max_batch=max_batch, with_tiles=True)
            _assert_same(got, want, table, (src, max_batch, 'top-K'))
            assert all(g[0].shape[1] == dc for g in got)
            by_batch[max_batch] = got
        if dtype == 'f32':                      # only the fp32 forward is bit for bit independent of its batch
            for a, b in zip(by_batch[4], by_batch[32]):
                assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[2].tolist() == b[2].tolist()
        # the threshold decode: a threshold between the scores of the stand-in weights' maps, few rows per tile
        t = _score_threshold(net, src)
        want, stage, table = _composition(net, src, 4, thresh=(t, 24))
        _totals('%s %s src %d threshold %.4g' % (kind, dtype, src, t), stage)
        got = net.detect_tiled(frames, tile=TILE, src=src, overlap=OVERLAP, score_thresh=t, max_dets=24, max_batch=4, with_tiles=True)
        _assert_same(got, want, table, (src, 'threshold'))
        assert len({m.shape[0] for m, _ in stage}) > 1, 'every tile delivered the same number of rows: pick another threshold'
    # the same frames as CPU tensors, CUDA tensors and without the tile index
    want, _, table = _composition(net, 64, 32)
    _assert_same(net.detect_tiled([torch.from_numpy(f) for f in frames], tile=TILE, overlap=OVERLAP), want, table, 'CPU tensors')
    _assert_same(net.detect_tiled([torch.from_numpy(f).cuda() for f in frames], tile=TILE, overlap=OVERLAP), want, table, 'CUDA tensors')


def _score_threshold(net, src):
    """a threshold that cuts the tiles' score maps unevenly: the 150th largest top-10 score over all tiles (or the last)"""
    _, px = _table_and_pixels(src)
    per = net.detect_batch(torch.from_numpy(px), K=10)
    s = np.sort(np.concatenate([d[:, 4] for d, _ in per]))[::-1]
    return float(np.float32(s[min(150, s.size - 1)]))


def test_graph_replay_equals_eager(monkeypatch):
    frames = _frames()
    for kind, dtype in (('DenseBoxLMLOC', 'f16'), ('DenseBox', 'f32')):
        net = _net(kind, dtype)
        with monkeypatch.context() as m:
            m.setenv('DBX_GRAPH', '0')
            eager = [net.detect_tiled(frames, tile=TILE, src=32, overlap=OVERLAP, max_batch=8, with_tiles=True) for _ in range(3)]
            assert not net.__dict__.get('_detect_graphs')
        want, _, table = _composition(net, 32, 8)
        for rep in range(3):
            _assert_same(eager[rep], want, table, (kind, 'eager', rep))
            _assert_same(net.detect_tiled(frames, tile=TILE, src=32, overlap=OVERLAP, max_batch=8, with_tiles=True), want, table,
                         (kind, 'graph', rep))
        shapes = {k[1] for k in net.__dict__['_detect_graphs'] if k[0] == 'level'}
        assert shapes == {(8, TILE, TILE, 3), (table.shape[0] % 8 or 8, TILE, TILE, 3)}, 'one graph shape plus a tail'
    net = _net('DenseBoxLMLOC', 'f16')
    net.train()                                          # train mode: the same launches eagerly (dropout: only the structure is checked)
    res = net.detect_tiled(frames, tile=TILE, overlap=OVERLAP)
    assert not net.__dict__.get('_detect_graphs') and all(d.shape[1] == 13 and keep == (DC.NMS(d, 0.4) if len(d) else []) for d, keep in res)


def test_one_cut_launch_one_rows_launch_per_chunk_one_nms_call(monkeypatch):
    net = _net('DenseBoxLMLOC', 'f16')
    frames = _frames()
    L = _lib.lib()
    calls = {'dbx_resize_cubic_batch_u8': [], 'dbx_tile_rows_batch': [], 'dbx_tile_nms_batch': [], 'dbx_nms': [], 'dbx_nms_large': []}
    for name in calls:
        real = getattr(L, name)
        monkeypatch.setattr(L, name, (lambda real, name: lambda *a: (calls[name].append(a), real(*a))[1])(real, name))
    n = _table_and_pixels(64)[0].shape[0]
    for max_batch in (4, 32):
        for v in calls.values():
            del v[:]
        net.detect_tiled(frames, tile=TILE, overlap=OVERLAP, max_batch=max_batch)
        assert len(calls['dbx_resize_cubic_batch_u8']) == 1 and calls['dbx_resize_cubic_batch_u8'][0][1] == n
        assert [(c[5], c[6]) for c in calls['dbx_tile_rows_batch']] == [(t0, min(max_batch, n - t0)) for t0 in range(0, n, max_batch)]
        assert len(calls['dbx_tile_nms_batch']) == 1 and not calls['dbx_nms'] and not calls['dbx_nms_large']


def test_roi_runs_only_the_tiles_whose_core_it_meets(monkeypatch):
    net = _net('DenseBoxLMLOC', 'f32')
    frames = _frames()
    roi = [[(100, 10, 150, 40)], None, [], [(0, 0, 5, 5), (60, 120, 70, 130)]]
    full, _ = _table_and_pixels(32)
    run = np.zeros(full.shape[0], bool)
    for b, rects in enumerate(roi):
        sel = full['frame'] == b
        run[sel] = True if rects is None else R.core_hits(full[sel], rects)
    assert 0 < run.sum() < full.shape[0] and not run[full['frame'] == 2].any()
    L = _lib.lib()
    jobs = []
    real = L.dbx_resize_cubic_batch_u8
    monkeypatch.setattr(L, 'dbx_resize_cubic_batch_u8', lambda *a: (jobs.append(a[1]), real(*a))[1])
    got = net.detect_tiled(frames, tile=TILE, src=32, overlap=OVERLAP, max_batch=32, roi=roi, with_tiles=True)
    assert jobs == [int(run.sum())]
    # the composition over the tiles that ran, cores from the full grid
    want, stage, table = _composition(net, 32, 32, only=np.flatnonzero(run))
    _totals('roi: %d of %d tiles' % (run.sum(), full.shape[0]), stage)
    _assert_same(got, want, table, 'roi')
    assert got[2][0].shape == (0, 13) and got[2][1] == [] and got[2][3].shape == (0,)
    # ... which is the full run restricted to the rows owned by the tiles that ran (f32: the forward does not depend on the batch)
    whole = net.detect_tiled(frames, tile=TILE, src=32, overlap=OVERLAP, max_batch=32, with_tiles=True)
    first = np.concatenate([[0], np.cumsum(np.bincount(full['frame'], minlength=4))])
    for b, ((d, keep, tl, pl), (wd, _, wt, _)) in enumerate(zip(got, whole)):
        ran = run[first[b] + wt]
        assert d.tobytes() == wd[ran].tobytes(), b
        assert keep == (DC.NMS(d, 0.4) if len(d) else [])


def test_rule_none_on_a_single_tile_frame_is_detect_batch_resized():
    """a square frame is one window: src = its side, no padding; the tile is then detect_batch_resized's resized frame, and its rows
    mapped back are the same numbers (side / size = src / tile, no offset)"""
    net = _net('DenseBoxLMLOC', 'f16')
    rs = np.random.RandomState(43)
    frames = [_img(rs, 96, 96), _img(rs, 96, 96)]
    got = net.detect_tiled(frames, tile=TILE, src=96, overlap=OVERLAP, K=10, rule='none')
    want = net.detect_batch_resized(frames, size=TILE, K=10)
    for (d, keep), (wd, _) in zip(got, want):
        assert d.tobytes() == wd.tobytes() and keep == DC.NMS(wd, 0.4)


def test_the_other_entry_points_are_unchanged_by_detect_tiled_calls():
    """the graph cache is one LRU over all tags: detect_tiled's shapes may evict the others' entries, which are then re-captured"""
    net = _net('DenseBoxLMLOC', 'f32')
    frames = _frames()
    x4 = synth.synth_images(4, 240, 240, seed=4).cuda()
    rs = np.random.RandomState(44)
    mixed = [_img(rs, 120, 200), _img(rs, 97, 240)]

    def snapshot():
        tr = track.Tracker(streams=4)
        return (net.detect_batch(x4, K=10), net.detect_pyramid(mixed, sizes=(96, 160), K=10), net.track_batch(x4, tracker=tr, K=10))

    def same(a, b):
        return all(len(p) == len(q) and all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(p, q))
                   for ra, rb in zip(a, b) for p, q in zip(ra, rb))
    before = snapshot()
    for src, mb in ((64, 4), (32, 8), (32, 5), (64, 32)):
        net.detect_tiled(frames, tile=TILE, src=src, overlap=OVERLAP, max_batch=mb)
        net.detect_tiled(frames, tile=TILE, src=src, overlap=OVERLAP, max_batch=mb, score_thresh=0.0, max_dets=16)
    assert len(net.__dict__['_detect_graphs']) <= DC._MAX_GRAPHS
    assert same(before, snapshot())
    want, _, table = _composition(net, 32, 8)
    _assert_same(net.detect_tiled(frames, tile=TILE, src=32, overlap=OVERLAP, max_batch=8), want, table, 'after the others')
