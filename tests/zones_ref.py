"""Restatement of the zone semantics (dbx_zone_filter_keep, dbx_zone_update_batch, dbx_zone_append, densebox_amd.zones) for the tests, in
plain Python integers and NumPy, written from the contract in include/densebox_hip.h as its sequential walk.  Geometry is in quarter
pixels; Python integers do not overflow, so every product is exact.  The anchor is float64, one IEEE operation per written operation.
tests/test_zones_ref.py pins it on hand-computed cases.  Also the seeded sequences the GPU tests replay.  Not collected."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_ref as TR  # noqa: E402

STATE = np.dtype([('owner_id', '<i4'), ('has_prev', '<i4'), ('px', '<i4'), ('py', '<i4'), ('inside', '<i4'), ('reserved', '<i4', (3,))])
EVENT = np.dtype([('stream', '<i4'), ('track_id', '<i4'), ('kind', '<i4'), ('index', '<i4'), ('frame', '<i4'), ('hits', '<i4'),
                  ('ax', '<i4'), ('ay', '<i4')])
assert STATE.itemsize == 32 and EVENT.itemsize == 32
FORWARD, BACKWARD, ENTER, EXIT, ENDED = range(5)


def quarter(v):
    """a user's float in quarter pixels: int(floor(4 * v + 0.5))"""
    return int(math.floor(4 * float(v) + 0.5))


def anchor(box, kind='centre'):
    """(ax, ay) in quarter pixels of the float64 box (x1, y1, x2, y2), or None when a value is not finite or has |v| >= 2^20"""
    x1, y1, x2, y2 = (float(v) for v in box[:4])
    if not all(math.isfinite(v) and abs(v) < 1048576.0 for v in (x1, y1, x2, y2)):
        return None
    ax = int(math.floor((x1 + x2) * 2.0 + 0.5))
    ay = int(math.floor((y1 + y2) * 2.0 + 0.5)) if kind == 'centre' else int(math.floor(y2 * 4.0 + 0.5))
    return ax, ay


def cross(ux, uy, vx, vy):
    return ux * vy - uy * vx


def side(line, p):
    ax, ay, bx, by = line
    return cross(bx - ax, by - ay, p[0] - ax, p[1] - ay) >= 0


def crossing(line, p0, p1):
    """None, FORWARD or BACKWARD for the move p0 -> p1 against the directed line (ax, ay, bx, by)"""
    s0, s1 = side(line, p0), side(line, p1)
    if s0 == s1:
        return None
    mx, my = p1[0] - p0[0], p1[1] - p0[1]
    ta = cross(mx, my, line[0] - p0[0], line[1] - p0[1]) >= 0
    tb = cross(mx, my, line[2] - p0[0], line[3] - p0[1]) >= 0
    if ta == tb:
        return None
    return FORWARD if s1 else BACKWARD


def inside(poly, p):
    """even-odd, half-open: poly a sequence of (x, y) integer vertices"""
    px, py = p
    n, count = len(poly), 0
    for i in range(n):
        (xi, yi), (xj, yj) = poly[i], poly[(i + 1) % n]
        if (yi > py) == (yj > py):
            continue
        d = yj - yi
        l, r = (px - xi) * d, (xj - xi) * (py - yi)
        count += (l < r) if d > 0 else (l > r)
    return count % 2 == 1


class Config:
    """one stream's table, in quarter pixels: lines [(ax, ay, bx, by)], regions [polygon], masks [(role, polygon)] with role 0 include,
    1 exclude; a polygon is a list of (x, y)"""

    def __init__(self, lines=(), regions=(), masks=()):
        self.lines = [tuple(int(v) for v in l) for l in lines]
        self.regions = [[(int(x), int(y)) for x, y in p] for p in regions]
        self.masks = [(int(r), [(int(x), int(y)) for x, y in p]) for r, p in masks]


def from_pixels(lines=(), regions=(), include=(), exclude=()):
    """a Config from a front end's float pixel coordinates: lines ((ax, ay), (bx, by)), polygons [(x, y), ...]"""
    q = quarter
    return Config([(q(a[0]), q(a[1]), q(b[0]), q(b[1])) for a, b in lines], [[(q(x), q(y)) for x, y in p] for p in regions],
                  [(0, [(q(x), q(y)) for x, y in p]) for p in include] + [(1, [(q(x), q(y)) for x, y in p]) for p in exclude])


# ------------------------------------------------------------------------------------------------------------ filter
def filter_keep(cfg, dets, keep, kind='centre'):
    """The keep list of one frame behind the filter: `keep` is the list as det_frame reads it (the clamped count's entries).  Returns the
    surviving entries in order."""
    if not cfg.masks:
        return list(keep)
    dets = np.asarray(dets, np.float64)
    has_inc = any(r != 1 for r, _ in cfg.masks)
    out = []
    for r in keep:
        if not 0 <= r < dets.shape[0]:
            continue
        p = anchor(dets[r], kind)
        if p is None:
            continue
        inc = any(inside(poly, p) for role, poly in cfg.masks if role != 1)
        exc = any(inside(poly, p) for role, poly in cfg.masks if role == 1)
        if (inc or not has_inc) and not exc:
            out.append(int(r))
    return out


# ------------------------------------------------------------------------------------------------------------ update
def new_state(streams, max_tracks):
    """(state STATE [streams, max_tracks], line counts int64 [streams, 8, 2], region counts int64 [streams, 8, 3])"""
    st = np.zeros((streams, max_tracks), STATE)
    st['owner_id'] = -1
    return st, np.zeros((streams, 8, 2), np.int64), np.zeros((streams, 8, 3), np.int64)


def _event(stream, tid, kind, index, frame, hits, p):
    e = np.zeros((), EVENT)
    e['stream'], e['track_id'], e['kind'], e['index'], e['frame'], e['hits'], e['ax'], e['ay'] = stream, tid, kind, index, frame, hits, p[0], p[1]
    return e


def update_frame(cfg, zstate, lines, regions, header, table, stream, min_hits=1, kind='centre'):
    """One frame of one stream behind the tracking update, in place on zstate STATE [T], lines int64 [8, 2], regions int64 [8, 3];
    header and table are the tracker's, as the update left them.  Returns the frame's events in order."""
    f = int(header[0]) - 1
    ev = []
    for t in range(table.shape[0]):
        z, k = zstate[t], table[t]
        kid, hits = int(k['id']), int(k['hits'])
        if z['owner_id'] >= 0 and kid != z['owner_id']:                       # 1
            for r in range(8):
                if int(z['inside']) >> r & 1:
                    ev.append(_event(stream, z['owner_id'], ENDED, r, f, 0, (z['px'], z['py'])))
                    regions[r, 1] += 1
                    regions[r, 2] -= 1
            z['owner_id'], z['has_prev'], z['px'], z['py'], z['inside'] = -1, 0, 0, 0, 0
        if kid < 0 or hits < min_hits:
            continue
        if kid != z['owner_id']:                                              # 2
            z['owner_id'], z['has_prev'], z['inside'] = kid, 0, 0
        p = anchor(k['box'], kind)
        if p is None:
            z['has_prev'] = 0
            continue
        if z['has_prev']:
            p0 = (int(z['px']), int(z['py']))
            for l, line in enumerate(cfg.lines):
                c = crossing(line, p0, p)
                if c is not None:
                    ev.append(_event(stream, kid, c, l, f, hits, p))
                    lines[l, c] += 1
        for r, poly in enumerate(cfg.regions):                                # 3
            now = inside(poly, p)
            if now != bool(int(z['inside']) >> r & 1):
                ev.append(_event(stream, kid, ENTER if now else EXIT, r, f, hits, p))
                regions[r, 0 if now else 1] += 1
                regions[r, 2] += 1 if now else -1
                z['inside'] = int(z['inside']) ^ (1 << r)
        z['px'], z['py'], z['has_prev'] = p[0], p[1], 1
    return ev


def update_batch(cfgs, zs, tstate, batch, stream0=0, min_hits=1, kind='centre'):
    """frames b = 0..batch-1 update streams stream0 + b of zs = (state, lines, regions) from tstate = (headers, tracks); cfgs: one Config
    per stream.  Returns per frame the list of events."""
    return [update_frame(cfgs[stream0 + b], zs[0][stream0 + b], zs[1][stream0 + b], zs[2][stream0 + b], tstate[0][stream0 + b],
                         tstate[1][stream0 + b], stream0 + b, min_hits, kind) for b in range(batch)]


def append(astate, arena, capacity, staged):
    """dbx_zone_append: astate int64 [4] = (cursor, dropped, total, reserved) in place; arena a list that grows up to `capacity` events,
    frame order then staging order"""
    cur = start = int(astate[0])
    for ev in staged:
        for e in ev:
            if cur < capacity:
                arena.append(e)
            cur += 1
    kept = min(cur, capacity)
    astate[0] = kept
    astate[1] += cur - kept
    astate[2] += cur - start


def as_events(evs):
    return np.array(evs, EVENT) if len(evs) else np.zeros(0, EVENT)


# ------------------------------------------------------------------------------------------------------------ seeded sequences
def scene(variant=0):
    """The table the sequences are made for, on a 640 x 480 image (pixels): two lines, two regions and one include polygon -- or, with
    variant 1, all 8 lines and 8 regions with 16-vertex polygons and an exclude polygon as well."""
    if variant == 0:
        return from_pixels(lines=[((320, 40), (320, 440)), ((60, 240), (600, 200))],
                           regions=[[(100, 100), (300, 100), (300, 300), (100, 300)], [(350, 150), (560, 120), (420, 260), (580, 400), (340, 380)]],
                           include=[[(40, 40), (600, 40), (600, 440), (40, 440)]])
    lines = [((80 * i + 40, 30), (80 * i + 60, 450)) if i % 2 else ((30, 50 * i + 40), (610, 50 * i + 70)) for i in range(8)]
    regions = []
    for i in range(8):
        cx, cy = 120 + 130 * (i % 4), 140 + 200 * (i // 4)
        regions.append([(cx + (70 if v % 2 else 35) * math.cos(2 * math.pi * v / 16 * (1 if i % 2 else -1)),
                         cy + (70 if v % 2 else 35) * math.sin(2 * math.pi * v / 16 * (1 if i % 2 else -1))) for v in range(16)])
    return from_pixels(lines=lines, regions=regions, include=[[(40, 40), (600, 40), (600, 440), (40, 440)]],
                       exclude=[[(300, 200), (340, 200), (340, 240), (300, 240)]])


def sequence(seed, steps, slots, objects=6, dc=5):
    """`steps` frames of one camera: per frame (dets float64 [n, dc], keep list), n <= slots.  Objects of 30 x 20 pixels move back and forth on straight
    paths of up to 83 pixels on the 640 x 480 image, a quarter-pixel jitter on top, some of them from outside the include polygon; each lives for a
    span of frames and then vanishes (its track coasts and is retired, inside a region or not); every other object appears in the frame
    its predecessor's track is retired with TRACK_PARAMS, so that slots are freed and taken again in one frame.  Every fifth frame holds
    a row with a NaN coordinate (never born; filtered out where a mask is set).  A live track with an invalid anchor cannot come from
    finite rows, so replay() plants one in the table (plant_invalid)."""
    rs = np.random.RandomState(seed)
    n_obj = min(objects, max(1, slots - 1))
    start = rs.randint(0, max(1, steps // 2), size=n_obj)
    start[0] = 0
    life = rs.randint(max(3, steps // 4), steps, size=n_obj)
    for j in range(1, n_obj, 2):                       # with max_age = 1 the track of j - 1 is retired in exactly this frame
        if start[j - 1] + life[j - 1] + 1 < steps - 1:
            start[j] = start[j - 1] + life[j - 1] + 1
    # the middle of a path lies on the first line (x = 320), on an edge of the first region (x = 300) or anywhere (every third one:
    # also outside the include polygon); the path runs 20..36 pixels to either side of it in x and up to 20 in y
    mid = np.stack([rs.randint(0, 640 * 4, size=n_obj), rs.randint(60 * 4, 420 * 4, size=n_obj)], 1) / 4.0
    mid[0::3, 0] = 320.0 + rs.randint(-8, 9, size=mid[0::3].shape[0]) / 4.0
    mid[1::3, 0] = 300.0 + rs.randint(-8, 9, size=mid[1::3].shape[0]) / 4.0
    mid[1::3, 1] = rs.randint(120 * 4, 280 * 4, size=mid[1::3].shape[0]) / 4.0
    half = np.stack([rs.randint(20 * 4, 36 * 4 + 1, size=n_obj) * rs.choice([-1, 1], size=n_obj), rs.randint(-20 * 4, 20 * 4 + 1, size=n_obj)], 1) / 4.0
    p0, p1 = mid - half, mid + half
    out = []
    for f in range(steps):
        rows = []
        for j in range(n_obj):
            if start[j] <= f < start[j] + life[j]:
                u = abs(((f - start[j]) % 12) - 6) / 6.0                      # back and forth along the path, 6 frames each way
                c = p0[j] + (p1[j] - p0[j]) * u
                c = np.floor(c * 4) / 4.0 + rs.randint(-1, 2, size=2) / 4.0
                rows.append(([c[0] - 15, c[1] - 10, c[0] + 15, c[1] + 10], 0.5 + 0.5 * rs.rand()))
        if f % 5 == 4 and len(rows) < slots:
            rows.append(([50.0, np.nan, 90.0, 80.0], 0.95))
        rows = rows[:slots]
        d = np.zeros((len(rows), dc), np.float64)
        for i, (b, s) in enumerate(rows):
            d[i, :4], d[i, 4] = b, s
        if dc == 13:
            d[:, 5:] = rs.randint(0, 2400, size=(len(rows), 8)) / 4.0
        perm = rs.permutation(len(rows))
        store = np.zeros_like(d)
        store[perm] = d
        out.append((store, [int(v) for v in perm]))
    return out


TRACK_PARAMS = dict(iou_thresh=0.05, max_age=1, alpha=0.5, beta=0.1, birth_score=TR.BIRTH_SCORE)


def plant_invalid(tstate, stream, step):
    """Every thirteenth step the lowest live slot of `stream` gets a box whose x2 is 2^20 (not usable): returns True when it did"""
    if step % 13 != 5:
        return False
    live = np.nonzero(tstate[1][stream]['id'] >= 0)[0]
    if live.size == 0:
        return False
    tstate[1][stream][live[0]]['box'][2] = 1048576.0
    return True


def replay(cfgs, seqs, streams, stream0, max_tracks, steps, min_hits=1, kind='centre', capacity=1 << 16, plant=True, on_step=None):
    """The whole chain on the restatements: per step the filter, tests/track_ref.py, (planted invalid boxes,) the zone update and the
    append, for frames b = 0..len(seqs)-1 on streams stream0 + b.  on_step(step, frames, kept, tstate_before_plant..., ...) is called
    with everything a GPU test compares.  Returns a dict of totals."""
    B = len(seqs)
    tstate = TR.new_state(streams, max_tracks)
    zs = new_state(streams, max_tracks)
    astate, arena = np.zeros(4, np.int64), []
    tot = dict(fwd=0, bwd=0, enter=0, exit=0, ended=0, reuse=0, dropped_rows=0, kept_rows=0, invalid=0)
    for step in range(steps):
        frames = [seqs[b][step] for b in range(B)]
        kept = [filter_keep(cfgs[stream0 + b], d, k, kind) for b, (d, k) in enumerate(frames)]
        for (d, k), kk in zip(frames, kept):
            tot['kept_rows'] += len(kk)
            tot['dropped_rows'] += len(k) - len(kk)
        res = TR.update_batch(tstate, [(d, kk) for (d, _), kk in zip(frames, kept)], stream0, **TRACK_PARAMS)
        tot['reuse'] += sum(r[5]['reuse'] for r in res)
        planted = [plant and plant_invalid(tstate, stream0 + b, step) for b in range(B)]
        tot['invalid'] += sum(planted)
        evs = update_batch(cfgs, zs, tstate, B, stream0, min_hits, kind)
        append(astate, arena, capacity, evs)
        for ev in evs:
            for e in ev:
                tot[('fwd', 'bwd', 'enter', 'exit', 'ended')[int(e['kind'])]] += 1
        if on_step is not None:
            on_step(step, frames, kept, res, tstate, zs, evs, astate, arena)
    return tot


# (max_tracks, slots, objects, steps, batch, scene variant, anchor, min_hits, arena capacity): the sequence set the GPU tests replay, on
# streams 1.. of 3.  One track slot, a table that fills up, a whole workgroup of slots; 2 + 2 + 1 and 8 + 8 + 2 configured items with
# 16-vertex polygons; both anchors; min_hits 1 and 3; an arena that takes everything, nothing, and a few events.
CASES = [
    (4, 7, 6, 48, 2, 0, 'centre', 1, 1 << 12),
    (1, 1, 1, 96, 2, 0, 'bottom', 1, 0),
    (256, 16, 14, 48, 2, 1, 'centre', 3, 40),
    (4, 7, 6, 48, 2, 1, 'bottom', 3, 1 << 12),
]
STREAMS, STREAM0 = 3, 1
_cache = {}


def case_inputs(case):
    """(configs per stream, sequences per frame of the batch) of a case; the streams outside the launch have a table of their own"""
    T, slots, objects, steps, B, variant, kind, min_hits, capacity = case
    cfgs = [scene(1 - variant)] + [scene(variant)] * B + [scene(1 - variant)] * (STREAMS - 1 - B)
    return cfgs, [sequence(100 + 10 * b, steps, slots, objects) for b in range(B)]


def reference(case):
    """The restated chain of a case, computed once: (totals, per step a dict of copies: frames, kept lists, the tracker's state behind
    the update (planted boxes included), the zone state and counters, the events per frame, the append state and the arena's length;
    the arena itself)."""
    if case not in _cache:
        T, slots, objects, steps, B, variant, kind, min_hits, capacity = case
        cfgs, seqs = case_inputs(case)
        snaps = []

        def on_step(step, frames, kept, res, tstate, zs, evs, astate, arena):
            snaps.append(dict(frames=frames, kept=kept, ids=[(r[0].copy(), r[2].copy()) for r in res], headers=tstate[0].copy(),
                              tracks=tstate[1].copy(), zstate=zs[0].copy(), lines=zs[1].copy(), regions=zs[2].copy(),
                              events=[as_events(e) for e in evs], astate=astate.copy(), stored=len(arena)))
        arena_out = []

        def keep_arena(*a):
            on_step(*a)
            arena_out[:] = [a[8]]
        tot = replay(cfgs, seqs, STREAMS, STREAM0, T, steps, min_hits, kind, capacity, on_step=keep_arena)
        _cache[case] = (tot, snaps, as_events(arena_out[0]))
    return _cache[case]
