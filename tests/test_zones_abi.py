"""CPU-side checks of the zones' C ABI and Python front end: struct layouts against the header, every refusal of the entry points, of
dbx_zone_check_config and of densebox_amd.zones, and dbx_zone_host -- the kernels' own geometry compiled for the host -- bitwise equal
to the restatement (tests/zones_ref.py) on the hand cases and on 100 000 random cases each from a small lattice, where ties are
frequent.  No GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from densebox_amd import _lib, track as T, zones as ZN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zones_ref as Z  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
P = C.c_void_p(0x1000)          # a non-null pointer that is never followed: every call below is refused before anything is queued


def test_struct_layouts_match_the_header():
    src = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    text = ' '.join(l.strip().lstrip('*').strip() for l in src[src.index('Layouts: dbx_zone_line'):].split('*/')[0].splitlines())
    seen = 0
    for name, cls in (('dbx_zone_line', _lib.ZoneLine), ('dbx_zone_poly', _lib.ZonePoly), ('dbx_zone_config', _lib.ZoneConfig),
                      ('dbx_zone_state', _lib.ZoneState), ('dbx_zone_event', _lib.ZoneEvent)):
        m = re.search(r'%s (\d+) bytes \(([^)]*)\)' % name, text)
        assert m, name
        assert C.sizeof(cls) == int(m.group(1)), name
        stated = [(f.split()[0], int(f.split()[1].rstrip(':'))) for f in m.group(2).replace(': x, y interleaved', '').split(', ')]
        assert stated == [(f[0], getattr(cls, f[0]).offset) for f in cls._fields_], (name, stated)
        seen += len(stated)
    assert seen == 4 + 3 + 7 + 6 + 8
    for dt, cls in ((ZN.POLY, _lib.ZonePoly), (ZN.CONFIG, _lib.ZoneConfig), (ZN.STATE, _lib.ZoneState), (ZN.EVENT, _lib.ZoneEvent),
                    (Z.STATE, _lib.ZoneState), (Z.EVENT, _lib.ZoneEvent)):
        assert dt.itemsize == C.sizeof(cls)
        assert [dt.fields[n][1] for n in dt.names] == [getattr(cls, f[0]).offset for f in cls._fields_]
    for s in ('dbx_zone_filter_keep', 'dbx_zone_update_batch', 'dbx_zone_append', 'dbx_zone_check_config', 'dbx_zone_host'):
        assert re.search(r'\bint %s\(' % s, src) and s in _lib.SIGNATURES


def _refused(rc, word):
    L = _lib.lib()
    assert rc == ERR_ARG and word.encode() in L.dbx_last_error(), (rc, L.dbx_last_error())


def test_filter_refusals():
    L = _lib.lib()

    def call(dets=P, dc=5, det_rows=8, keep=P, prefix=None, batch=2, slots=4, cfg=P, streams=3, stream0=1, anchor=0, out=C.c_void_p(0x2000),
             stats=P):
        return L.dbx_zone_filter_keep(dets, dc, det_rows, keep, prefix, batch, slots, cfg, streams, stream0, anchor, out, stats, None)
    _refused(call(batch=-1), 'batch')
    _refused(call(dc=6), 'det_cols')
    _refused(call(slots=0), 'slots')
    _refused(call(slots=1025, det_rows=4096), 'slots')
    _refused(call(det_rows=-1), 'det_rows')
    _refused(call(det_rows=7), 'det_rows')
    _refused(call(stream0=-1), 'streams')
    _refused(call(stream0=2), 'streams')
    _refused(call(streams=-1, stream0=0, batch=0), 'streams')
    _refused(call(anchor=2), 'anchor')
    _refused(call(anchor=-1), 'anchor')
    for name in ('dets', 'keep', 'cfg', 'out', 'stats'):
        _refused(call(**{name: None}), 'null')
    _refused(call(out=P), 'keep_out')
    assert call(batch=0, dets=None, keep=None, cfg=None, out=None, stats=None) == 0             # a no-op


def test_update_refusals():
    L = _lib.lib()

    def call(tracks=P, headers=P, cfg=P, state=P, lines=P, regions=P, batch=2, streams=3, stream0=1, T_=4, min_hits=1, anchor=0, staged=P,
             count=P, commit=1):
        return L.dbx_zone_update_batch(tracks, headers, cfg, state, lines, regions, batch, streams, stream0, T_, min_hits, anchor, staged,
                                       count, commit, None)
    _refused(call(batch=-1), 'batch')
    _refused(call(stream0=-1), 'streams')
    _refused(call(stream0=2), 'streams')
    _refused(call(T_=0), 'max_tracks')
    _refused(call(T_=257), 'max_tracks')
    _refused(call(min_hits=0), 'min_hits')
    _refused(call(anchor=2), 'anchor')
    for name in ('tracks', 'headers', 'cfg', 'state', 'lines', 'regions', 'staged', 'count'):
        _refused(call(**{name: None}), 'null')
    assert call(batch=0, tracks=None, state=None) == 0


def test_append_refusals():
    L = _lib.lib()

    def call(staged=P, count=P, batch=2, T_=4, events=P, capacity=8, state=P):
        return L.dbx_zone_append(staged, count, batch, T_, events, capacity, state, None)
    _refused(call(batch=-1), 'batch')
    _refused(call(T_=0), 'max_tracks')
    _refused(call(T_=257), 'max_tracks')
    _refused(call(capacity=-1), 'capacity')
    for name in ('staged', 'count', 'state', 'events'):
        _refused(call(**{name: None}), 'null')
    assert call(batch=0, staged=None, count=None, state=None, events=None) == 0


def _config(lines=1, regions=1, masks=1):
    c = _lib.ZoneConfig()
    c.n_lines, c.n_regions, c.n_masks = lines, regions, masks
    for i in range(8):
        c.lines[i].ax, c.lines[i].ay, c.lines[i].bx, c.lines[i].by = 0, 0, 4 + i, 8
        for p in (c.regions[i], c.masks[i]):
            p.n = 3
            p.xy[0:6] = [0, 0, 40, 0, 0, 40]
    return c


def test_check_config_refusals():
    L = _lib.lib()
    assert L.dbx_zone_check_config(C.byref(_config())) == 0 and L.dbx_zone_check_config(C.byref(_config(8, 8, 8))) == 0
    assert L.dbx_zone_check_config(C.byref(_lib.ZoneConfig())) == 0                                # an empty table
    _refused(L.dbx_zone_check_config(None), 'null')
    for field in ('n_lines', 'n_regions', 'n_masks'):
        for v in (-1, 9):
            c = _config()
            setattr(c, field, v)
            _refused(L.dbx_zone_check_config(C.byref(c)), field)
    for v in (2, 17, 0, -3):
        for which in ('regions', 'masks'):
            c = _config()
            getattr(c, which)[0].n = v
            _refused(L.dbx_zone_check_config(C.byref(c)), 'vertices')
    c = _config()
    c.regions[1].n = 99                                                                          # beyond n_regions: not looked at
    assert L.dbx_zone_check_config(C.byref(c)) == 0
    for v in ((1 << 20) + 1, -(1 << 20) - 1):
        c = _config()
        c.lines[0].by = v
        _refused(L.dbx_zone_check_config(C.byref(c)), 'coordinate')
        c = _config()
        c.masks[0].xy[5] = v
        _refused(L.dbx_zone_check_config(C.byref(c)), 'coordinate')
        c = _config()
        c.regions[0].xy[0] = v
        _refused(L.dbx_zone_check_config(C.byref(c)), 'coordinate')
    c = _config()
    c.lines[0].by = 1 << 20                                                                      # the bound itself is allowed
    c.regions[0].xy[6] = 1 << 30                                                                 # beyond n: not looked at
    assert L.dbx_zone_check_config(C.byref(c)) == 0
    c = _config()
    c.lines[0].bx, c.lines[0].by = 0, 0
    _refused(L.dbx_zone_check_config(C.byref(c)), 'A == B')
    c = _config()
    c.regions[0].role = 1
    _refused(L.dbx_zone_check_config(C.byref(c)), 'role')
    c = _config()
    c.masks[0].role = 1
    assert L.dbx_zone_check_config(C.byref(c)) == 0
    c.masks[0].role = 2
    _refused(L.dbx_zone_check_config(C.byref(c)), 'role')


def test_front_end_refusals():
    tr = T.Tracker(3, max_tracks=4)
    for kw in (dict(anchor='top'), dict(min_hits=0), dict(min_hits=1.5), dict(capacity=0), dict(min_hits=True)):
        with pytest.raises(RuntimeError, match='Zones'):
            ZN.Zones(tr, **kw)
    with pytest.raises(RuntimeError, match='Tracker'):
        ZN.Zones(object())
    zn = ZN.Zones(tr, anchor='bottom', min_hits=2)
    tri = [(0, 0), (10, 0), (0, 10)]
    bad = [
        dict(s=3), dict(s=-1), dict(s=0.5),
        dict(lines=[((0, 0), (1, 1))] * 9), dict(regions=[tri] * 9), dict(include=[tri] * 5, exclude=[tri] * 4),
        dict(lines=[((0, 0), (0, 0))]), dict(lines=[((0, 0), (0.1, 0.1))]),                     # A == B after rounding to quarter pixels
        dict(lines=[((0, 0), (1, float('nan')))]), dict(lines=[((0, 0), (float('inf'), 1))]), dict(lines=[((0, 0), (262144.25, 1))]),
        dict(lines=[((0, 0),)]), dict(lines=[((0, 0), (1, 1), (2, 2))]), dict(lines=[((0, 0), (1, 1, 1))]), dict(lines=[5]),
        dict(regions=[tri[:2]]), dict(regions=[[(i, i * i) for i in range(17)]]), dict(include=[[(0, 0), (1, 'a'), (2, 2)]]),
        dict(exclude=[[(0, 0), (1, 1), (-262145, 2)]]), dict(regions=[[(0, 0), (1, True), (2, 2)]]),
    ]
    for kw in bad:
        kw = dict(kw)
        with pytest.raises(RuntimeError, match='set_stream'):
            zn.set_stream(kw.pop('s', 0), **kw)
    assert not zn.table(0)['n_lines'] and not zn.table(0)['n_masks']                             # a refused table changes nothing
    zn.set_stream(2, lines=[((0, 0), (262144, -262144))], regions=[tri], include=[tri], exclude=[[(i, i * i) for i in range(16)]])
    t = zn.table(2)
    assert (t['n_lines'], t['n_regions'], t['n_masks']) == (1, 1, 2) and t['lines'][0].tolist() == [0, 0, 1 << 20, -(1 << 20)]
    assert t['masks'][0]['role'] == 0 and t['masks'][1]['role'] == 1 and t['masks'][1]['n'] == 16 and t['masks'][1]['xy'][31] == 900
    assert zn.table(2)['regions'][0]['xy'][:6].tolist() == [0, 0, 40, 0, 0, 40]
    other = ZN.Zones(T.Tracker(3, max_tracks=4))
    for fn, kw in ((ZN.update_batch, dict(tracker=tr, zones=other)), (ZN.update_batch, dict(tracker=tr, zones=None)),
                   (ZN.filter_keep, dict(zones=tr))):
        with pytest.raises(RuntimeError, match='zones'):
            fn([np.zeros((1, 5))], [[0]], **kw)
    with pytest.raises(RuntimeError, match='does not fit'):
        ZN.filter_keep([np.zeros((1, 5))] * 2, [[0]] * 2, zones=zn, stream0=2)
    assert zn.events().shape == (0,) and not zn.counts()[0].any() and zn.counts()[1].shape == (3, 8, 3)


# ------------------------------------------------------------------------------------------------------------ dbx_zone_host
def _host(op, boxes=None, ints=None):
    n = len(boxes) if boxes is not None else len(ints)
    out = np.full((n, 3) if op <= 1 else (n,), -99, np.int32)
    b = None if boxes is None else np.ascontiguousarray(boxes, np.float64)
    i = None if ints is None else np.ascontiguousarray(ints, np.int32)
    rc = _lib.lib().dbx_zone_host(op, n, None if b is None else b.ctypes.data, None if i is None else i.ctypes.data, out.ctypes.data)
    assert rc == 0, _lib.lib().dbx_last_error()
    return out


def _poly_row(p, poly):
    row = np.zeros(35, np.int32)
    row[0], row[1], row[2] = p[0], p[1], len(poly)
    row[3:3 + 2 * len(poly)] = np.asarray(poly, np.int32).reshape(-1)
    return row


def test_host_geometry_refusals():
    L = _lib.lib()
    out = np.zeros(4, np.int32)
    _refused(L.dbx_zone_host(5, 1, None, out.ctypes.data, out.ctypes.data), 'op')
    _refused(L.dbx_zone_host(-1, 1, None, out.ctypes.data, out.ctypes.data), 'op')
    _refused(L.dbx_zone_host(2, -1, None, out.ctypes.data, out.ctypes.data), 'n=')
    _refused(L.dbx_zone_host(2, 1, None, None, out.ctypes.data), 'null')
    _refused(L.dbx_zone_host(0, 1, None, out.ctypes.data, out.ctypes.data), 'null')
    _refused(L.dbx_zone_host(3, 1, None, out.ctypes.data, None), 'null')
    assert L.dbx_zone_host(4, 0, None, None, None) == 0


def test_host_geometry_equals_the_restatement_on_the_hand_cases():
    line = (0, 0, 0, 40)
    moves = [((10, 20), (-10, 20)), ((-10, 20), (10, 20)), ((10, 20), (0, 20)), ((0, 20), (-10, 20)), ((-10, 20), (0, 20)), ((0, 20), (10, 20)),
             ((0, 10), (0, 30)), ((10, 50), (-10, 50)), ((10, 0), (-10, 0)), ((10, 40), (-10, 40)), ((-10, 0), (10, 0)), ((-10, 40), (10, 40)),
             ((3, 3), (3, 3))]
    got = _host(3, ints=[line + a + b for a, b in moves])
    want = [Z.crossing(line, a, b) for a, b in moves]
    assert got.tolist() == [-1 if w is None else w for w in want]
    assert got.tolist() == [0, 1, 0, -1, -1, 1, -1, -1, 0, -1, -1, 1, -1]
    pts = [(10, 20), (-10, 20), (0, 20), (0, -5), (1 << 22, -(1 << 22))]
    assert _host(2, ints=[line + p for p in pts]).tolist() == [int(Z.side(line, p)) for p in pts] == [0, 1, 1, 1, 0]
    square = [(0, 0), (40, 0), (40, 40), (0, 40)]
    diamond = [(20, 0), (40, 20), (20, 40), (0, 20)]
    ell = [(0, 0), (40, 0), (40, 20), (20, 20), (20, 40), (0, 40)]
    tie = [(0, 0), (40, 40), (40, 0), (0, 40)]
    cases = [(p, square) for p in square + [(20, 0), (20, 40), (0, 20), (40, 20), (20, 20)]]
    cases += [(p, diamond) for p in ((10, 20), (-10, 20), (50, 20), (20, 20))]
    cases += [(p, poly) for poly in (ell, ell[::-1]) for p in ((10, 30), (30, 10), (30, 30), (20, 30), (19, 30))]
    cases += [(p, tie) for p in ((5, 20), (35, 20), (20, 5), (20, 35), (20, 20))]
    got = _host(4, ints=[_poly_row(p, poly) for p, poly in cases])
    assert got.tolist() == [int(Z.inside(poly, p)) for p, poly in cases]
    assert got[:9].tolist() == [1, 0, 0, 0, 1, 0, 1, 0, 1]
    boxes = [[0.0, 0.0, 20.25, 0.0], [0.0, 0.0, 20.75, 0.0], [0.0, 0.0, 20.24, 0.0], [0.0, 0.0, -20.25, 0.0], [0.0, 0.0, -20.26, 0.0],
             [0.0, 3.0, 0.0, 7.125], [0.0, 3.0, 0.0, 7.375], [1048575.75] * 4, [-1048575.75] * 4]
    for bad in (np.nan, np.inf, -np.inf, 1048576.0, -1048576.0):
        for c in range(4):
            boxes.append([1.0, 2.0, 3.0, 4.0])
            boxes[-1][c] = bad
    for op, kind in ((0, 'centre'), (1, 'bottom')):
        want = [Z.anchor(b, kind) for b in boxes]
        assert _host(op, boxes=boxes).tolist() == [[0, 0, 0] if w is None else [1, w[0], w[1]] for w in want]
    assert _host(1, boxes=boxes)[5:7].tolist() == [[1, 0, 29], [1, 0, 30]] and _host(0, boxes=boxes)[:2, 1].tolist() == [41, 42]


def _on_segment(a, b, p):
    return Z.cross(b[0] - a[0], b[1] - a[1], p[0] - a[0], p[1] - a[1]) == 0 and min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and \
        min(a[1], b[1]) <= p[1] <= max(a[1], b[1])


def test_host_geometry_equals_the_restatement_on_random_lattice_cases():
    rs = np.random.RandomState(5)
    n = 100000
    # (move, line): eight coordinates from a 7 x 7 lattice scaled by up to 2^17 (so that products need more than 32 bits); a tie is a
    # zero among the four cross products that decide
    q = rs.randint(0, 7, size=(n, 8)) * rs.choice([1, 3, 1 << 17], size=(n, 1))
    same = (q[:, 0] == q[:, 2]) & (q[:, 1] == q[:, 3])
    q[same, 2] += 1                                                            # A != B
    rows = q.tolist()
    want, ties = [], 0
    for r in rows:
        line, p0, p1 = tuple(r[:4]), (r[4], r[5]), (r[6], r[7])
        c = Z.crossing(line, p0, p1)
        want.append(-1 if c is None else c)
        m = (p1[0] - p0[0], p1[1] - p0[1])
        ties += 0 in (Z.cross(line[2] - line[0], line[3] - line[1], p0[0] - line[0], p0[1] - line[1]),
                      Z.cross(line[2] - line[0], line[3] - line[1], p1[0] - line[0], p1[1] - line[1]),
                      Z.cross(m[0], m[1], line[0] - p0[0], line[1] - p0[1]), Z.cross(m[0], m[1], line[2] - p0[0], line[3] - p0[1]))
    assert _host(3, ints=q).tolist() == want
    assert ties >= n // 100 and min(want.count(v) for v in (-1, 0, 1)) > n // 100, (ties, [want.count(v) for v in (-1, 0, 1)])
    assert _host(2, ints=q[:, :6]).tolist() == [int(Z.side(tuple(r[:4]), (r[4], r[5]))) for r in rows]
    # (point, polygon): 3..16 vertices and the point from a 6 x 6 lattice; a tie is a point on the polygon's boundary
    ints = np.zeros((n, 35), np.int32)
    nv = rs.randint(3, 17, size=n)
    scale = rs.choice([1, 5, 1 << 17], size=n)
    want, ties = [], 0
    for i in range(n):
        k = int(nv[i])
        pts = rs.randint(0, 6, size=(k + 1, 2)) * int(scale[i])
        ints[i, 0:2], ints[i, 2], ints[i, 3:3 + 2 * k] = pts[0], k, pts[1:].reshape(-1)
        poly, p = [tuple(v) for v in pts[1:].tolist()], tuple(pts[0].tolist())
        want.append(int(Z.inside(poly, p)))
        ties += any(_on_segment(poly[j], poly[(j + 1) % k], p) for j in range(k))
    assert _host(4, ints=ints).tolist() == want
    assert ties >= n // 100 and n // 10 < sum(want) < n - n // 10, (ties, sum(want))
