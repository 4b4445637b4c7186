"""CPU-side checks of tiled detection: the new entry points are exported, declared and bound at ABI version 13; dbx_tile's layout;
dbx_tile_grid equals the restated plan; dbx_tile_host (the kernels' own mapping and ownership functions) equals the restatement
bitwise on hand cases and on 100 000 seeded rows; every refusal of the entry points and of the front end, before any device work; the
size functions; tiles.plan's region-of-interest pruning."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from densebox_amd import _lib, tiles as T

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiles_ref as R       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float('inf'), float('nan')
NEW = ['dbx_tile_grid', 'dbx_tile_stage_bytes', 'dbx_tile_rows_batch', 'dbx_tile_nms_batch_workspace_bytes', 'dbx_tile_nms_batch',
       'dbx_tile_host']


def test_new_entry_points_are_exported_declared_and_bound_at_version_13():
    L = _lib.lib()
    src = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, code), name + ' is not declared'
        assert name in _lib.SIGNATURES and name not in _lib.MISSING, name
        assert callable(getattr(L, name))
    assert int(re.search(r'#define\s+DBX_ABI_VERSION\s+(\d+)', src).group(1)) == L.dbx_version() == _lib.ABI_VERSION == 13
    assert re.search(r'#define\s+DBX_TILE_RULE_NONE\s+0\b', code) and re.search(r'#define\s+DBX_TILE_RULE_CORE\s+1\b', code)
    assert (_lib.TILE_RULE_NONE, _lib.TILE_RULE_CORE) == (R.NONE, R.CORE) == (0, 1)
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert all(name in doc for name in NEW)


def test_dbx_tile_layout_matches_the_header_the_binding_and_the_doc():
    src = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    m = re.search(r'typedef struct dbx_tile \{(.*?)\} dbx_tile;', src, re.S)
    fields = []
    for ctype, names in re.findall(r'(int32_t|double)\s+([^;]+);', m.group(1)):
        fields += [(n.strip(), C.c_int32 if ctype == 'int32_t' else C.c_double) for n in names.split(',')]
    assert fields == list(_lib.Tile._fields_)
    assert C.sizeof(_lib.Tile) == 64 == T.TILE_DTYPE.itemsize == R.TILE.itemsize
    offs = {n: getattr(_lib.Tile, n).offset for n, _ in _lib.Tile._fields_}
    assert offs == dict(frame=0, x0=4, y0=8, side=12, cw=16, ch=20, scale=24, lo2x=32, hi2x=40, lo2y=48, hi2y=56)
    for dt in (T.TILE_DTYPE, R.TILE):
        assert {n: dt.fields[n][1] for n in dt.names} == offs and list(dt.names) == [n for n, _ in fields]
    assert '"dbx_tile is 64 bytes"' in open(os.path.join(ROOT, 'densebox_amd', 'csrc', 'tile_ops.hip')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    m = re.search(r'class Tile\(C\.Structure\):.*?_fields_ = \[(.*?)\]\n', doc, re.S)
    assert m, 'INTEGRATION.md does not show Tile'
    names = re.findall(r"\('(\w+)', C\.(\w+)\)", m.group(1))
    assert [(n, getattr(C, t)) for n, t in names] == list(_lib.Tile._fields_)


def _grid(h, w, src, overlap, cap=None, out='ok'):
    L = _lib.lib()
    n = L.dbx_tile_grid(h, w, src, overlap, None, 0)
    if n < 0 or out is None:
        return n, None
    table = np.zeros(max(n, 1), T.TILE_DTYPE)
    got = L.dbx_tile_grid(h, w, src, overlap, table.ctypes.data, n if cap is None else cap)
    return got, table[:n]


def test_tile_grid_is_the_restated_plan():
    for L_ in range(1, 201):
        for S in (8, 32, 64):
            for ov in (0, 8, S // 2):
                if 2 * ov > S:
                    continue
                for h, w in ((L_, 3 * S + 1), (S, L_)):
                    n, table = _grid(h, w, S, ov)
                    want = R.plan(h, w, S, ov)
                    assert n == want.shape[0] and table.tobytes() == want.tobytes(), (h, w, S, ov)
    n, table = _grid(2160, 3840, 512, 128)
    assert n == 60 and table.tobytes() == R.plan(2160, 3840, 512, 128).tobytes()
    assert T.plan(2160, 3840, 512, 128).tobytes() == table.tobytes()
    assert _grid(2160, 3840, 512, 128, cap=100)[0] == 60           # a larger cap is fine; only the plan's records are written


@pytest.mark.parametrize('bad', [
    dict(src=0), dict(src=-4), dict(overlap=-1), dict(src=64, overlap=33), dict(src=1, overlap=1), dict(h=0), dict(w=0), dict(h=-5),
    dict(cap=5), dict(cap=0), dict(cap=-1), dict(h=70000, w=70000, src=8, overlap=0),
])
def test_tile_grid_refusals(bad):
    L = _lib.lib()
    a = dict(h=96, w=160, src=64, overlap=16, cap=6)
    a.update(bad)
    table = np.zeros(64, T.TILE_DTYPE)
    assert L.dbx_tile_grid(a['h'], a['w'], a['src'], a['overlap'], table.ctypes.data, a['cap']) == -1, bad
    assert b'tile_grid' in L.dbx_last_error()
    assert table.tobytes() == np.zeros(64, T.TILE_DTYPE).tobytes(), 'a refused call wrote records'
    with pytest.raises(RuntimeError, match='tile_grid'):
        _lib.check(-1)


def _host(table, tile_of, rows, rule, op=1):
    L = _lib.lib()
    table = np.ascontiguousarray(table.astype(T.TILE_DTYPE))
    rows = np.ascontiguousarray(rows, np.float64)
    tile_of = np.ascontiguousarray(tile_of, np.int32)
    out, marks = np.full_like(rows, -7.0), np.full(rows.shape[0], -7, np.int32)
    _lib.check(L.dbx_tile_host(op, rows.shape[0], table.ctypes.data, table.shape[0], tile_of.ctypes.data, rows.ctypes.data, rows.shape[1],
                               rule, out.ctypes.data, marks.ctypes.data))
    return out, marks


def _want(table, tile_of, rows, rule):
    out, marks = np.empty_like(rows), np.empty(rows.shape[0], np.int32)
    for t in np.unique(tile_of):
        sel = tile_of == t
        out[sel] = R.map_rows(rows[sel], table[t])
        marks[sel] = R.marks(out[sel], table[t], rule)
    return out, marks


def test_tile_host_hand_cases():
    table = np.concatenate([R.plan(64, 160, 64, 16), R.plan(64, 160, 32, 8, 1, 0.5)])
    assert table.shape[0] == 3 + 3 * 7 and (table[5]['x0'], table[5]['y0'], table[5]['scale']) == (48, 0, 0.5)
    rows = np.array([[50.0, 0.0, 62.0, 10.0, 0.5],            # window at 0: centre sum 112, the boundary: the higher tile's
                     [2.0, 0.0, 14.0, 10.0, 0.5],             # the same box seen from the window at 48: owned
                     [50.0, 0.0, 61.75, 10.0, 0.5],           # a quarter pixel less: tile 0's
                     [NAN, 0.0, 60.0, 10.0, 0.5], [50.0, NAN, 60.0, 10.0, 0.5], [50.0, 0.0, NAN, 10.0, 0.5], [50.0, 0.0, 60.0, NAN, 0.5],
                     [10.0, 5.0, 30.0, 15.0, NAN],            # a NaN score: copied, owned
                     [-0.0, -0.0, -0.0, -0.0, -0.0],          # -0 * scale - (-0) = +0
                     [1e308, 0.0, 1e308, 10.0, INF],          # the sum overflows to +inf: below no upper bound, not even the last core's +inf
                     [10.0, 5.0, 30.0, 15.0, 0.9]])           # the half-pixel tile at (48, 0): 53, 2.5, 63, 7.5
    tile_of = np.array([0, 1, 0, 1, 1, 1, 1, 0, 0, 2, 3 + 2], np.int32)
    for rule in (R.CORE, R.NONE):
        got, marks = _host(table, tile_of, rows, rule)
        want, wm = _want(table, tile_of, rows, rule)
        assert got.tobytes() == want.tobytes() and marks.tolist() == wm.tolist()
    got, marks = _host(table, tile_of, rows, R.CORE)
    assert marks.tolist() == [0, 1, 1, 0, 0, 0, 0, 1, 1, 0, 1]
    assert got[1].tolist() == [50.0, 0.0, 62.0, 10.0, 0.5] and got[10].tolist() == [53.0, 2.5, 63.0, 7.5, 0.9]
    assert np.signbit(got[8, :4]).tolist() == [False] * 4 and np.signbit(got[8, 4])
    lm = np.arange(13, dtype=np.float64)[None]
    assert _host(table, [1], lm, R.CORE)[0][0].tolist() == [48, 1, 50, 3, 4, 53, 6, 55, 8, 57, 10, 59, 12]
    out, marks = _host(table, tile_of, rows, R.CORE, op=0)     # the map alone: the marks are not written
    assert out.tobytes() == got.tobytes() and (marks == -7).all()


def seeded_rows(dc, n=100000, seed=2023):
    """(table, tile_of [n], rows [n, dc]): rows of two frames' tiles (scale 1 and 0.5) in tile coordinates on a QUARTER-PIXEL lattice,
    the box centres up to 8 tile pixels outside the window; one row in 16 is moved so that the centre sum of its mapped box is exactly a
    finite core bound of its tile (its width is then a multiple of half a pixel, so x1 stays on the lattice)."""
    rs = np.random.RandomState(seed)
    table = np.concatenate([R.plan(96, 160, 64, 16, 0, 1.0), R.plan(130, 70, 32, 8, 1, 0.5)])
    tile_of = rs.randint(0, table.shape[0], n).astype(np.int32)
    t = table[tile_of]
    w, h = rs.randint(4, 49, n) * 2 / 4.0, rs.randint(2, 25, n) * 2 / 4.0
    x1 = rs.randint(-32, 4 * 72, n) / 4.0 - w / 2
    y1 = rs.randint(-32, 4 * 72, n) / 4.0 - h / 2
    snap = rs.randint(0, 16, n) == 0
    for lo, hi, org, p1, ext in (('lo2x', 'hi2x', 'x0', x1, w), ('lo2y', 'hi2y', 'y0', y1, h)):
        bound = np.where(rs.randint(0, 2, n) == 0, t[lo], t[hi])
        sel = snap & np.isfinite(bound) & (rs.randint(0, 2, n) == 0)
        p1[sel] = ((bound[sel] - 2.0 * t[org][sel]) / t['scale'][sel] - ext[sel]) / 2
    rows = np.zeros((n, dc))
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = x1, y1, x1 + w, y1 + h
    rows[:, 4] = rs.uniform(0, 1, n)
    if dc == 13:
        rows[:, 5:] = rs.randint(-64, 4 * 80, (n, 8)) / 4.0
    assert (rows[:, :4] * 4 == np.round(rows[:, :4] * 4)).all(), 'off the quarter-pixel lattice'
    return table, tile_of, rows


@pytest.mark.parametrize('dc', [5, 13])
def test_tile_host_is_the_restatement_on_100000_seeded_rows(dc):
    table, tile_of, rows = seeded_rows(dc)
    want, wm = _want(table, tile_of, rows, R.CORE)
    got, marks = _host(table, tile_of, rows, R.CORE)
    assert got.tobytes() == want.tobytes()
    assert marks.tolist() == wm.tolist()
    t = table[tile_of]
    sx, sy = want[:, 0] + want[:, 2], want[:, 1] + want[:, 3]
    on_bound = (sx == t['lo2x']) | (sx == t['hi2x']) | (sy == t['lo2y']) | (sy == t['hi2y'])
    shares = on_bound.mean(), (wm == 1).mean(), (wm == 0).mean()
    print('dc %d: %.2f %% of the centres on a core boundary, %.1f %% owned, %.1f %% not' % ((dc,) + tuple(100 * s for s in shares)))
    assert shares[0] >= 0.01 and shares[1] >= 0.20 and shares[2] >= 0.20, shares
    # both sides of the half-open rule are met on the boundary rows: a lower bound owns, an upper bound does not
    assert wm[on_bound].min() == 0 and wm[on_bound].max() == 1
    got_n, marks_n = _host(table, tile_of, rows, R.NONE)
    assert got_n.tobytes() == want.tobytes() and (marks_n == 1).all()


def test_tile_host_refusals():
    L = _lib.lib()
    table = R.plan(64, 160, 64, 16).astype(T.TILE_DTYPE)
    rows, tile_of = np.zeros((2, 5)), np.zeros(2, np.int32)
    out, marks = np.zeros((2, 5)), np.zeros(2, np.int32)
    ok = dict(op=1, n=2, tiles=table.ctypes.data, n_tiles=3, tile_of=tile_of.ctypes.data, rows=rows.ctypes.data, dc=5, rule=1,
              out=out.ctypes.data, marks=marks.ctypes.data)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return L.dbx_tile_host(a['op'], a['n'], a['tiles'], a['n_tiles'], a['tile_of'], a['rows'], a['dc'], a['rule'], a['out'], a['marks'])
    assert call() == 0 and call(n=0, tiles=None, rows=None) == 0 and call(op=0, marks=None) == 0
    for bad in (dict(op=2), dict(op=-1), dict(n=-1), dict(dc=4), dict(dc=12), dict(rule=2), dict(rule=-1), dict(n_tiles=0), dict(tiles=None),
                dict(tile_of=None), dict(rows=None), dict(out=None), dict(marks=None)):
        assert call(**bad) == -1, bad
        assert b'tile_host' in L.dbx_last_error()
    for v in (3, -1):
        tile_of[1] = v
        assert call() == -1 and b'names tile' in L.dbx_last_error()


def _table(n_frames_tiles=(1, 6, 2)):
    return R.case_table(n_frames_tiles).astype(T.TILE_DTYPE)


def _rows_call(L, table='ok', rows=0x1000, counts=None, tdev=0x2000, n_tiles=None, t0=0, n=4, rpt=10, dc=5, rule=1, stage=0x3000, edit=None):
    vp = lambda a: None if a is None else C.c_void_p(a)       # noqa: E731
    if isinstance(table, str):
        table = _table()
        if edit:
            edit(table)
    nt = (table.shape[0] if table is not None else 9) if n_tiles is None else n_tiles
    return L.dbx_tile_rows_batch(vp(rows), vp(counts), vp(table.ctypes.data) if table is not None else None, vp(tdev), nt, t0, n, rpt, dc,
                                 rule, vp(stage), None)


def _nms_call(L, table='ok', tdev=0x2000, n_tiles=None, frames=3, rpt=10, dc=5, nms=0.4, stage=0x3000, od=0x4000, ok=0x5000, ot=0x6000,
              oc=0x7000, ws=0x8000, edit=None):
    vp = lambda a: None if a is None else C.c_void_p(a)       # noqa: E731
    if isinstance(table, str):
        table = _table()
        if edit:
            edit(table)
    nt = (table.shape[0] if table is not None else 9) if n_tiles is None else n_tiles
    return L.dbx_tile_nms_batch(vp(table.ctypes.data) if table is not None else None, vp(tdev), nt, frames, rpt, dc, nms, vp(stage), vp(od),
                                vp(ok), vp(ot), vp(oc), vp(ws), None)


def _set(field, t, v):
    def edit(table):
        table[field][t] = v
    return edit


TABLE_FAULTS = [
    dict(edit=_set('scale', 4, 0.0)), dict(edit=_set('scale', 0, -1.0)), dict(edit=_set('scale', 8, INF)), dict(edit=_set('scale', 3, NAN)),
    dict(edit=_set('frame', 3, 0)), dict(edit=_set('frame', 8, 1)), dict(edit=_set('frame', 0, -1)),
    dict(edit=_set('x0', 2, -1)), dict(edit=_set('y0', 5, -48)), dict(edit=_set('lo2x', 1, NAN)), dict(edit=_set('hi2y', 7, NAN)),
    dict(table=None), dict(n_tiles=0), dict(n_tiles=-1), dict(n_tiles=2 ** 20 + 1),
    dict(dc=4), dict(dc=6), dict(dc=0), dict(rpt=0), dict(rpt=-1), dict(rpt=4097),
    dict(rpt=683),                                      # 6 tiles x 683 rows = 4098 > 4096
]


@pytest.mark.parametrize('bad', TABLE_FAULTS + [
    dict(rows=None), dict(tdev=None), dict(stage=None), dict(n=0), dict(n=-2), dict(t0=-1), dict(t0=6, n=4), dict(t0=9, n=1),
    dict(rule=2), dict(rule=-1),
])
def test_tile_rows_batch_rejects_bad_arguments_without_touching_the_gpu(bad):
    L = _lib.lib()
    rc = _rows_call(L, **bad)
    assert rc == -1, bad
    assert b'tile_rows_batch' in L.dbx_last_error()
    with pytest.raises(RuntimeError, match='tile_rows_batch'):
        _lib.check(rc)


@pytest.mark.parametrize('bad', TABLE_FAULTS + [
    dict(tdev=None), dict(stage=None), dict(od=None), dict(ok=None), dict(ot=None), dict(oc=None), dict(ws=None),
    dict(frames=0), dict(frames=-1), dict(frames=2),    # frame index 2 is outside 0..1
    dict(nms=NAN), dict(nms=-0.1),
])
def test_tile_nms_batch_rejects_bad_arguments_without_touching_the_gpu(bad):
    L = _lib.lib()
    rc = _nms_call(L, **bad)
    assert rc == -1, bad
    assert b'tile_nms_batch' in L.dbx_last_error()
    with pytest.raises(RuntimeError, match='tile_nms_batch'):
        _lib.check(rc)


def test_a_frame_with_too_many_rows_is_refused_by_both():
    """tile 0 moved to frame 1 keeps the frame indices non-decreasing (frame 0 is then empty, frame 1 has 7 tiles): accepted as a table,
    and refused only when 7 tiles x rows_per_tile exceeds the NMS's bound"""
    L = _lib.lib()
    for call in (_rows_call, _nms_call):
        assert call(L, rpt=586, edit=_set('frame', 0, 1)) == -1 and b'the NMS' in L.dbx_last_error()      # 7 x 586 = 4102
        assert call(L, rpt=683) == -1 and b'the NMS' in L.dbx_last_error()                                  # 6 x 683 = 4098


def test_size_functions():
    L = _lib.lib()
    up = lambda v: (v + 255) // 256 * 256                      # noqa: E731
    f = L.dbx_tile_stage_bytes
    for n, rpt, dc in ((1, 1, 5), (9, 10, 13), (64, 64, 13), (480, 68, 13), (60, 68, 5)):
        assert f(n, rpt, dc) == up(n * 8) + up(n * rpt * 4) + up(n * rpt * dc * 8)
    for bad in ((0, 10, 5), (-1, 10, 5), (9, 0, 5), (9, 4097, 5), (9, 10, 4), (9, 10, 12), (2 ** 20 + 1, 1, 5), (2 ** 20, 4096, 5)):
        assert f(*bad) == -1, bad
    g = L.dbx_tile_nms_batch_workspace_bytes
    for frames, mt, rpt in ((1, 1, 1), (3, 6, 10), (1, 64, 64), (8, 60, 68), (2, 1, 4096)):
        nmax = mt * rpt
        assert g(frames, mt, rpt) == frames * (up(nmax * 4) + up(nmax * ((nmax + 63) // 64) * 8))
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 61, 68), (1, 2, 2049), (1, 1, 4097), (-1, 1, 1)):
        assert g(*bad) == -1, bad


def test_plan_prunes_by_core_and_keeps_the_full_grids_cores():
    full = T.plan(96, 160, 64, 16)
    assert full.tobytes() == R.plan(96, 160, 64, 16).tobytes()
    for rects in ([(0, 0, 56, 10)], [(0, 0, 57, 10)], [(60, 40, 61, 50), (150, 0, 160, 5)], [], [(-50, -50, -40, -40)], [(0, 0, 160, 96)]):
        got = T.plan(96, 160, 64, 16, roi=rects)
        assert got.tobytes() == full[R.core_hits(full, rects)].tobytes(), rects
    assert len(T.plan(96, 160, 64, 16, roi=[(-50, -50, -40, -40)])) == 1        # the unbounded corner core
    table = T.call_table('t', [(96, 160), (64, 64), (40, 50), (130, 70)], 64, 32, 8, roi=[None, [], [(0, 0, 1, 1)], None])
    assert np.bincount(table['frame'], minlength=4).tolist() == [len(R.plan(96, 160, 32, 8)), 0, 1, len(R.plan(130, 70, 32, 8))]
    assert (table['scale'] == 0.5).all()


def test_front_end_argument_checks_fail_before_any_device_work():
    import densebox_amd as D
    from densebox_amd import synth
    net = D.DenseBoxLMLOC(synth.vgg19_standin(seed=0)).eval()
    frames = [np.zeros((96, 160, 3), np.uint8), np.zeros((40, 50, 3), np.uint8)]
    kw = dict(tile=64, overlap=16)
    for bad in (0, -4, 66, 62, 64.0, '64', True, None):
        with pytest.raises(RuntimeError, match='detect_tiled: tile'):
            net.detect_tiled(frames, tile=bad, overlap=16)
    for bad in (0, -1, 32.0, '32', True):
        with pytest.raises(RuntimeError, match='detect_tiled: src'):
            net.detect_tiled(frames, src=bad, **kw)
    for bad in (-1, 33, 16.0, None, True):
        with pytest.raises(RuntimeError, match='detect_tiled: overlap'):
            net.detect_tiled(frames, tile=64, overlap=bad)
    with pytest.raises(RuntimeError, match='detect_tiled: overlap'):
        net.detect_tiled(frames, tile=64, src=32, overlap=17)
    for bad in (0, -1, 4097, 10.0, True):
        with pytest.raises(RuntimeError, match='detect_tiled: K'):
            net.detect_tiled(frames, K=bad, **kw)
    for bad in (0, -1, 2.0, None):
        with pytest.raises(RuntimeError, match='detect_tiled: max_batch'):
            net.detect_tiled(frames, max_batch=bad, **kw)
    for bad in ('centre', None, 1):
        with pytest.raises(RuntimeError, match='detect_tiled: rule'):
            net.detect_tiled(frames, rule=bad, **kw)
    for bad in (NAN, INF, '0.5', True):
        with pytest.raises(RuntimeError, match='detect_tiled: score_thresh'):
            net.detect_tiled(frames, score_thresh=bad, **kw)
    for bad in (0, 4097, 10.0, None):
        with pytest.raises(RuntimeError, match='detect_tiled: max_dets'):
            net.detect_tiled(frames, score_thresh=0.5, max_dets=bad, **kw)
    with pytest.raises(RuntimeError, match='detect_tiled: K=7 and score_thresh'):
        net.detect_tiled(frames, K=7, score_thresh=0.5, **kw)
    for bad in (NAN, -0.1):
        with pytest.raises(RuntimeError, match='detect_tiled: nms_thresh'):
            net.detect_tiled(frames, nms_thresh=bad, **kw)
    # 6 tiles x 683 rows exceed the NMS's 4096; 6 x 682 would pass this check
    with pytest.raises(RuntimeError, match=r'detect_tiled: frame 0 has 6 tiles x 683 rows per tile = 4098 rows'):
        net.detect_tiled(frames, K=683, **kw)
    with pytest.raises(RuntimeError, match=r'detect_tiled: frame 0 has 6 tiles x 700 rows'):
        net.detect_tiled(frames, score_thresh=0.5, max_dets=700, **kw)
    for bad in ([[(0, 0, 10, 10)]], 'all', [[(0, 0, 10, 10)], [(0, 0, 10)]], [[(0, 0, 10, 10)], [(5, 5, 5, 9)]], [[(0, 0, 10.5, 10)], []],
                [[(0, 0, 10, 10)], (0, 0, 10, 10)]):
        with pytest.raises(RuntimeError, match='detect_tiled: (roi|a rectangle)'):
            net.detect_tiled(frames, roi=bad, **kw)
    with pytest.raises(RuntimeError, match='detect_tiled: no tile to run'):
        net.detect_tiled(frames, roi=[[], []], **kw)
    with pytest.raises(RuntimeError, match='detect_tiled.*uint8'):
        net.detect_tiled([frames[0].astype(np.float32)], **kw)
    with pytest.raises(RuntimeError, match='tiles.plan'):
        T.plan(0, 10, 64, 16)
    for bad in (dict(results=[np.zeros((1, 5))]), dict(table=np.zeros(2)), dict(frames=0), dict(rule='x'),
                dict(results=[np.zeros((1, 5)), np.zeros((1, 13))]), dict(results=[np.zeros((1, 6))] * 2), dict(results=[np.zeros((4097, 5))] * 2)):
        a = dict(results=[np.zeros((1, 5))] * 2, table=T.plan(64, 100, 64, 16), frames=1, rule='core')
        a.update(bad)
        with pytest.raises(RuntimeError, match='tiles.merge_host_results'):
            T.merge_host_results(a['results'], a['table'], a['frames'], rule=a['rule'])
