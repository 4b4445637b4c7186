"""Zones on the GPU behind the tracker: per camera stream a region-of-interest filter on the keep lists in front of the tracking update
(dbx_zone_filter_keep), counted crossings of directed lines and enter / exit events of count regions behind it (dbx_zone_update_batch),
and the events of every call collected in a device arena (dbx_zone_append).  Nothing of it copies the tracker's state to the host.

Semantics (include/densebox_hip.h has the contract): geometry is in quarter pixels; a box is judged by its anchor, the centre or the
middle of its bottom edge; a polygon is tested by the even-odd rule with half-open edges; a move crosses a line A -> B when its end
points lie on different sides of the line and A and B on different sides of the move, forward when the side cross(B - A, P - A) >= 0
goes from false to true.  A row is kept when its anchor is inside an include polygon (or there is none) and inside no exclude polygon;
a track counts from the frame it has min_hits rows, and a track that ends inside a region leaves it with an "ended inside" event."""
import ctypes as C
import itertools
import math

import numpy as np
import torch

from . import _lib, decode as DC, rows as R, track as T
from ._lib import check, ptr, stream_ptr
from .decode import _integer

MAX_ITEMS = 8                # lines, regions and mask polygons per stream
MAX_VERTS = 16
COORD_MAX = 1 << 20          # quarter pixels
EVENTS_PER_SLOT = 24         # dbx_zone_update_batch's staging per track slot
ANCHORS = {'centre': 0, 'bottom': 1}
KINDS = ('forward', 'backward', 'enter', 'exit', 'ended_inside')
POLY = np.dtype([('n', '<i4'), ('role', '<i4'), ('xy', '<i4', (32,))])                                            # dbx_zone_poly
CONFIG = np.dtype([('n_lines', '<i4'), ('n_regions', '<i4'), ('n_masks', '<i4'), ('reserved', '<i4'), ('lines', '<i4', (8, 4)),
                   ('regions', POLY, (8,)), ('masks', POLY, (8,))])                                               # dbx_zone_config
STATE = np.dtype([('owner_id', '<i4'), ('has_prev', '<i4'), ('px', '<i4'), ('py', '<i4'), ('inside', '<i4'),
                  ('reserved', '<i4', (3,))])                                                                     # dbx_zone_state
EVENT = np.dtype([('stream', '<i4'), ('track_id', '<i4'), ('kind', '<i4'), ('index', '<i4'), ('frame', '<i4'), ('hits', '<i4'),
                  ('ax', '<i4'), ('ay', '<i4')])                                                                  # dbx_zone_event
assert POLY.itemsize == C.sizeof(_lib.ZonePoly) == 136 and CONFIG.itemsize == C.sizeof(_lib.ZoneConfig) == 2320
assert STATE.itemsize == C.sizeof(_lib.ZoneState) == 32 and EVENT.itemsize == C.sizeof(_lib.ZoneEvent) == 32


def _quarter(what, v):
    """a pixel coordinate in quarter pixels, int(floor(4 * v + 0.5)), or RuntimeError"""
    if not isinstance(v, (int, float, np.integer, np.floating)) or isinstance(v, (bool, np.bool_)) or not math.isfinite(v):
        raise RuntimeError('set_stream: %s has a coordinate %r that is not a finite number' % (what, v))
    q = int(math.floor(4 * float(v) + 0.5))
    if abs(q) > COORD_MAX:
        raise RuntimeError('set_stream: %s has a coordinate %r beyond +-%d pixels' % (what, v, COORD_MAX // 4))
    return q


def _points(what, pts, lo, hi):
    try:
        pts = [tuple(p) for p in pts]
    except TypeError:
        raise RuntimeError('set_stream: %s must be a sequence of (x, y) points' % what)
    if not lo <= len(pts) <= hi or any(len(p) != 2 for p in pts):
        raise RuntimeError('set_stream: %s must have %d..%d points (x, y), got %d' % (what, lo, hi, len(pts)))
    return [(_quarter(what, x), _quarter(what, y)) for x, y in pts]


class Zones:
    """The device side of the zones of a track.Tracker's streams: per stream a table (dbx_zone_config, 2320 bytes) of up to 8 directed
    lines, 8 count regions and 8 mask polygons, per (stream, track slot) 32 bytes of zone state, the counters, and an arena of
    `capacity` events (32 bytes each).  net.watch_batch() and zones.update_batch() advance it; counts() and events() read it.

    anchor: 'centre' or 'bottom', the point of a box that is tested.  min_hits: a track counts once it has had that many rows.  The
    buffers are allocated at the first use, on the tracker's device."""
    _serials = itertools.count()

    def __init__(self, tracker, anchor='centre', min_hits=1, capacity=1 << 16):
        if not isinstance(tracker, T.Tracker):
            raise RuntimeError('Zones: tracker must be a track.Tracker, got %s' % type(tracker).__name__)
        if anchor not in ANCHORS:
            raise RuntimeError('Zones: anchor=%r must be one of %s' % (anchor, sorted(ANCHORS)))
        if not _integer(min_hits) or not 1 <= min_hits < 1 << 31:
            raise RuntimeError('Zones: min_hits=%r must be a positive integer' % (min_hits,))
        if not _integer(capacity) or capacity < 1:
            raise RuntimeError('Zones: capacity=%r must be a positive integer' % (capacity,))
        self.tracker, self.anchor, self.min_hits, self.capacity = tracker, anchor, int(min_hits), int(capacity)
        self.streams, self.max_tracks = tracker.streams, tracker.max_tracks
        self.serial = next(Zones._serials)          # part of the graph keys, with the buffers' addresses
        self._host = np.zeros(self.streams, CONFIG)
        self._cfg = self._state = self._dry = self._events = None

    # -------------------------------------------------------------------------------------------------------- the table
    def set_stream(self, s, lines=(), regions=(), include=(), exclude=()):
        """Replaces the table of stream `s`: lines ((ax, ay), (bx, by)) directed A -> B, regions / include / exclude polygons of 3..16
        points (x, y), all in pixels (floats; rounded to quarter pixels).  The kernels read the table from the device, so captured
        graphs see the change at their next replay; zone state and counters stay (reset() clears them)."""
        if not _integer(s) or not 0 <= s < self.streams:
            raise RuntimeError('set_stream: stream %r is not in 0..%d' % (s, self.streams - 1))
        lines, regions, masks = list(lines), list(regions), [(0, p) for p in include] + [(1, p) for p in exclude]
        for what, items in (('lines', lines), ('regions', regions), ('include + exclude', masks)):
            if len(items) > MAX_ITEMS:
                raise RuntimeError('set_stream: %d %s exceed %d' % (len(items), what, MAX_ITEMS))
        c = np.zeros((), CONFIG)
        c['n_lines'], c['n_regions'], c['n_masks'] = len(lines), len(regions), len(masks)
        for i, l in enumerate(lines):
            (ax, ay), (bx, by) = _points('line %d' % i, l, 2, 2)
            if (ax, ay) == (bx, by):
                raise RuntimeError('set_stream: line %d has A == B (in quarter pixels)' % i)
            c['lines'][i] = ax, ay, bx, by
        for name, polys in (('regions', [(0, p) for p in regions]), ('masks', masks)):
            for i, (role, p) in enumerate(polys):
                pts = _points('%s polygon %d' % (name, i), p, 3, MAX_VERTS)
                c[name][i]['n'], c[name][i]['role'] = len(pts), role
                c[name][i]['xy'][:2 * len(pts)] = np.asarray(pts, np.int32).reshape(-1)
        buf = np.ascontiguousarray(c).reshape(1).view(np.uint8).copy()
        check(_lib.lib().dbx_zone_check_config(C.cast(buf.ctypes.data, C.POINTER(_lib.ZoneConfig))))
        self._host[s] = c
        if self._cfg is not None:
            self._cfg[s * CONFIG.itemsize:(s + 1) * CONFIG.itemsize].copy_(torch.from_numpy(buf))

    def table(self, s):
        """the host copy of stream s's table (CONFIG)"""
        return self._host[s].copy()

    # -------------------------------------------------------------------------------------------------------- buffers
    def _layout(self):
        """byte offsets of (line counts, region counts, append state) behind the zone state in the state buffer, and its size"""
        o_lines = self.streams * self.max_tracks * STATE.itemsize
        o_regions = o_lines + self.streams * 8 * 2 * 8
        o_app = o_regions + self.streams * 8 * 3 * 8
        return o_lines, o_regions, o_app, o_app + 32

    def _initial(self):
        o_lines, _, _, size = self._layout()
        host = np.zeros(size, np.uint8)
        host[:o_lines].view(STATE)['owner_id'] = -1
        return host

    def _buffers(self, dev):
        """(table uint8, state uint8: dbx_zone_state [streams][max_tracks], line counts int64 [streams][8][2], region counts int64
        [streams][8][3], append state int64 [4]; events uint8 [capacity * 32]) on the device, allocated once"""
        if self._state is None:
            dev = self.tracker.device if self.tracker.device is not None else dev
            self._cfg = torch.from_numpy(self._host.view(np.uint8).reshape(-1).copy()).to(dev)
            self._state = torch.from_numpy(self._initial()).to(dev)
            self._dry = torch.empty_like(self._state)            # the copy of the state a graph's warm-up runs advance
            self._events = torch.empty(self.capacity * EVENT.itemsize, dtype=torch.uint8, device=dev)
        return self._cfg, self._state, self._events

    def _key(self, dev):
        cfg, state, events = self._buffers(dev)
        return (self.serial, cfg.data_ptr(), state.data_ptr(), events.data_ptr(), self.anchor, self.min_hits, self.capacity)

    def reset(self):
        """forget every slot's zone state, the counters and the events; the tables, the buffers and the graphs captured on them stay"""
        if self._state is not None:
            self._state.copy_(torch.from_numpy(self._initial()))

    def _host_state(self):
        host = self._initial() if self._state is None else self._state.cpu().numpy()
        o_lines, o_regions, o_app, size = self._layout()
        return (host[:o_lines].view(STATE).reshape(self.streams, self.max_tracks), host[o_lines:o_regions].view(np.int64).reshape(self.streams, 8, 2),
                host[o_regions:o_app].view(np.int64).reshape(self.streams, 8, 3), host[o_app:size].view(np.int64))

    def counts(self):
        """one copy: (lines int64 [streams, 8, 2] = (forward, backward), regions int64 [streams, 8, 3] = (enters, exits, occupancy))"""
        _, lines, regions, _ = self._host_state()
        return lines.copy(), regions.copy()

    def events(self):
        """One copy of the append state, then one copy of exactly the events written: the structured array (EVENT) in the order they
        happened (call by call, stream by stream, slot by slot).  Raises when events were dropped because the arena was full."""
        if self._state is None:
            return np.zeros(0, EVENT)
        o_app = self._layout()[2]
        cursor, dropped = (int(v) for v in self._state[o_app:o_app + 16].cpu().numpy().view(np.int64))
        if dropped > 0:
            raise RuntimeError('Zones: %d events did not fit the arena of capacity=%d; watch with a larger capacity'
                               % (dropped, self.capacity))
        return np.zeros(0, EVENT) if cursor == 0 else self._events[:cursor * EVENT.itemsize].cpu().numpy().view(EVENT)


# ------------------------------------------------------------------------------------------------------------ the launches
def _check_zones(fn, zones, tracker=None):
    if not isinstance(zones, Zones):
        raise RuntimeError('%s: zones must be a zones.Zones, got %s' % (fn, type(zones).__name__))
    if tracker is not None and zones.tracker is not tracker:
        raise RuntimeError('%s: zones was made for another tracker' % fn)


def _filter(zn, rows, stream0):
    """dbx_zone_filter_keep on the device rows: (the filtered keep buffer, of rows.keep's layout; stats int32 [B, 2])"""
    cfg = zn._buffers(rows.dets.device)[0]
    keep_out = torch.empty_like(rows.keep)
    stats = torch.empty((rows.B, 2), dtype=torch.int32, device=rows.dets.device)
    check(_lib.lib().dbx_zone_filter_keep(*rows.args(), ptr(cfg), zn.streams, stream0, ANCHORS[zn.anchor], ptr(keep_out), ptr(stats),
                                          stream_ptr()))
    return keep_out, stats


def _launch(zn, rows, stream0, dry=False):
    """filter -> dbx_track_update_batch -> dbx_zone_update_batch -> dbx_track_append -> dbx_zone_append on the device rows `rows`, for
    streams stream0 .. stream0 + B - 1.  dry: the tracker and the zones advance scratch copies of their state and append nothing.
    Returns (the filtered keep buffer, track._launch's tensors, every other tensor the launches wrote)."""
    tr, dev, B = zn.tracker, rows.dets.device, rows.B
    cfg, state, events = zn._buffers(dev)
    if dry:
        zn._dry.copy_(state)
        state = zn._dry
    keep_f, stats = _filter(zn, rows, stream0)
    o_lines, o_regions, o_app, _ = zn._layout()
    zb = state.data_ptr()
    staged = torch.empty(B * zn.max_tracks * EVENTS_PER_SLOT * EVENT.itemsize, dtype=torch.uint8, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    L = _lib.lib()

    def between(base, o_tab):
        check(L.dbx_zone_update_batch(C.c_void_p(base + o_tab), C.c_void_p(base), ptr(cfg), C.c_void_p(zb), C.c_void_p(zb + o_lines),
                                      C.c_void_p(zb + o_regions), B, zn.streams, stream0, zn.max_tracks, zn.min_hits, ANCHORS[zn.anchor],
                                      ptr(staged), ptr(count), 1, stream_ptr()))
    out = T._launch(tr, R.Rows(rows.dets, keep_f, rows.prefix, B, rows.slots), stream0, dry, between=between)
    check(L.dbx_zone_append(ptr(staged), ptr(count), B, zn.max_tracks, None if dry else ptr(events), 0 if dry else zn.capacity,
                            C.c_void_p(zb + o_app), stream_ptr()))
    return keep_f, out, (stats, staged, count)


def filter_keep(dets, keeps, *, zones, stream0=0):
    """The region-of-interest filter alone on the host results of any detect_* call, with ONE upload, the filter launch and one copy
    back: entry j belongs to stream stream0 + j.  Returns per image the filtered keep list."""
    fn = 'filter_keep'
    _check_zones(fn, zones)
    p = R.pack_host(fn, dets, keeps, max_slots=T.MAX_SLOTS)
    T._check_streams(fn, zones.tracker, stream0, p.B)
    rows = p.upload(zones.tracker.device if zones.tracker.device is not None else torch.device('cuda'))
    k = _filter(zones, rows, int(stream0))[0].cpu().numpy().reshape(p.B, p.slots + 1)
    return [DC._keep_list(k[b]) for b in range(p.B)]


def update_batch(dets, keeps, *, tracker, zones, stream0=0):
    """track.update_batch() with the filter in front and the two zone launches behind it, on the host results of any detect_* call.
    Returns per image (keep, track_id, track_hits): the filtered keep list and, for its entries in order, what track.update_batch
    returns."""
    fn = 'update_batch'
    _check_zones(fn, zones, tracker)
    p = R.pack_host(fn, dets, keeps, max_slots=T.MAX_SLOTS)
    T._check_streams(fn, tracker, stream0, p.B)
    rows = p.upload(tracker.device if tracker.device is not None else torch.device('cuda'))
    keep_f, out, _ = _launch(zones, rows, int(stream0))
    k, h = keep_f.cpu().numpy().reshape(p.B, p.slots + 1), out[0].cpu().numpy()
    lists = [DC._keep_list(k[b]) for b in range(p.B)]
    return [(l, h[0, b, :len(l)].copy(), h[1, b, :len(l)].copy()) for b, l in enumerate(lists)]


# ------------------------------------------------------------------------------------------------------------ net.watch_batch
def _watch_eager(zn, K, thresh, stream0, nms_thresh, dry_outside_capture):
    """track._track_eager with the filter and the zone launches: the tensors that go to the host first (the filtered keep lists in the
    place of the decode's), then every other tensor the launches wrote"""
    def eager(net, images):
        s, l, hm, ll = DC._forward_maps(net, images)
        B = int(images.size(0))
        dry = dry_outside_capture and not torch.cuda.is_current_stream_capturing()
        rows, extra = R.decode_rows(s, l, hm, ll, B, K, thresh, nms_thresh)
        keep_f, out, more = _launch(zn, rows, stream0, dry)
        return (rows.dets, keep_f) + extra + out + (rows.keep,) + more
    return eager


def watch_batch(net, images, *, tracker, zones, stream0=0, K=10, score_thresh=None, max_dets=1024, nms_thresh=0.4, max_batch=32):
    """track_batch() with zones: per chunk the forward, the decode, dbx_zone_filter_keep on the keep lists, dbx_track_update_batch on the
    filtered lists, dbx_zone_update_batch, dbx_track_append and dbx_zone_append; the arguments are track_batch's, plus `zones` (a Zones
    made for `tracker`).  Neither the tracker's nor the zones' state leaves the device; zones.counts() and zones.events() read it.

    Returns, per image in input order, (dets, keep, track_id, track_hits): dets bit for bit detect_batch's or detect_batch_thresh's,
    keep the FILTERED keep list, track_id and track_hits for its entries as track_batch gives them.

    Eval mode replays ONE hipGraph per chunk from the cache detect() uses, under the tag 'watch', keyed like track_batch's plus the
    zones, their buffers and parameters.  The tables are read from the device at every replay: set_stream() needs no recapture."""
    fn = 'watch_batch'
    _check_zones(fn, zones, tracker)
    T._check_streams(fn, tracker, stream0, DC._frame_count(fn, images))
    tc = DC._thresh_or_topk(fn, K, score_thresh, max_dets)
    if tc is None:
        R._check_K(fn, K, T.MAX_SLOTS)
    if tc is not None and tc[1] > T.MAX_SLOTS:
        raise RuntimeError('%s: max_dets=%r must be an integer in 1..%d' % (fn, max_dets, T.MAX_SLOTS))
    DC._one_shape(fn, images, with_dtype=True)
    mode = ('topk', int(K)) if tc is None else ('thresh', tc[1], tc[0])
    flags = (True, True, True) + (False,) * 7 if tc is None else (False, False, True, True) + (False,) * 7
    dry, dc = DC._use_graph(net), DC._det_cols(net)

    def chunk(x, idx):
        first = int(stream0) + idx[0]
        key = (mode + tracker._key(x.device, first) + zones._key(x.device), float(nms_thresh))
        res = DC._run_chunk(net, 'watch', x, key, _watch_eager(zones, int(K), tc, first, nms_thresh, dry), flags)
        return T._unpack(mode[0], res, dc)
    return DC._detect_many(fn, images, max_batch, chunk, with_index=True)
