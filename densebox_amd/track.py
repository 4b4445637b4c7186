"""Multi-stream tracking by detection on the GPU: one independent tracker per camera stream, its state on the device, updated by ONE
dbx_track_update_batch launch per batch behind decode + NMS; the tracks that ended are collected in a device arena (dbx_track_append).

Semantics, per stream and frame (include/densebox_hip.h has the contract): every live track predicts box + vel; the kept rows are walked
in keep-list order and each takes the unclaimed live track of the largest +1-pixel IoU (the NMS's formula; the lowest slot on ties) when
that IoU is > iou_thresh, strictly; a claimed track moves by an alpha-beta filter per coordinate (box = p + alpha * r, vel += beta * r
with r = row - p), an unclaimed one coasts on its prediction and is retired once it has gone more than max_age frames without a match;
an unmatched row with finite coordinates and score >= birth_score starts a track in the lowest free slot (ids count up per stream), or
is counted in the stream's `unborn` when the table is full."""
import ctypes as C
import itertools

import numpy as np
import torch

from . import _lib, decode as DC, rows as R
from ._lib import check, ptr, stream_ptr
from .decode import _integer, _keep_list

MAX_SLOTS = 1024             # dbx_track_update_batch's bound on the list positions of a frame (they live in LDS)
MAX_TRACKS = 256             # ... and on the track slots of a stream (one thread each)
TRACK = np.dtype([('box', '<f8', (4,)), ('vel', '<f8', (4,)), ('score', '<f8'), ('best_score', '<f8'), ('id', '<i4'), ('hits', '<i4'),
                  ('age', '<i4'), ('first_frame', '<i4'), ('last_frame', '<i4'), ('best_frame', '<i4')])           # dbx_track
RECORD = np.dtype([('stream', '<i4'), ('reserved', '<i4'), ('t', TRACK)])                                           # dbx_track_record
assert TRACK.itemsize == C.sizeof(_lib.Track) == 104 and RECORD.itemsize == C.sizeof(_lib.TrackRecord) == 112


def _number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_)) and not np.isnan(v)


class Tracker:
    """The device side of tracking `streams` cameras: per stream a header (frame, next_id, unborn) and a table of `max_tracks` slots of
    dbx_track (104 bytes), plus an arena of `capacity` dbx_track_record (112 bytes) for the tracks that ended.  net.track_batch() and
    track.update_batch() advance it without copying state to the host; live() and finished() read it.

    iou_thresh: a row continues a track when their IoU is strictly above it.  max_age: a track is retired once it has gone more than
    max_age frames without a match.  alpha, beta: the gains of the position and velocity corrections.  birth_score: an unmatched row
    starts a track when its score is >= this.  The defaults (0.3, 5, 0.5, 0.1, every row) are a convention, NOT tuned values: no trained
    weights exist in this tree to tune them with.  The buffers are allocated on `device` (the current CUDA device by default) at the
    first use."""
    _serials = itertools.count()

    def __init__(self, streams, max_tracks=64, iou_thresh=0.3, max_age=5, alpha=0.5, beta=0.1, birth_score=-float('inf'),
                 capacity=1 << 16, device=None):
        if not _integer(streams) or streams < 1:
            raise RuntimeError('Tracker: streams=%r must be a positive integer' % (streams,))
        if not _integer(max_tracks) or not 1 <= max_tracks <= MAX_TRACKS:
            raise RuntimeError('Tracker: max_tracks=%r must be an integer in 1..%d' % (max_tracks, MAX_TRACKS))
        if not _integer(max_age) or max_age < 0 or max_age >= 1 << 31:
            raise RuntimeError('Tracker: max_age=%r must be a non-negative integer' % (max_age,))
        if not _integer(capacity) or capacity < 1:
            raise RuntimeError('Tracker: capacity=%r must be a positive integer' % (capacity,))
        for name, v in (('iou_thresh', iou_thresh), ('alpha', alpha), ('beta', beta), ('birth_score', birth_score)):
            if not _number(v):
                raise RuntimeError('Tracker: %s=%r must be a number' % (name, v))
        self.streams, self.max_tracks, self.max_age, self.capacity = int(streams), int(max_tracks), int(max_age), int(capacity)
        self.iou_thresh, self.alpha, self.beta, self.birth_score = float(iou_thresh), float(alpha), float(beta), float(birth_score)
        self.device = None if device is None else torch.device(device)
        self.serial = next(Tracker._serials)        # part of the graph keys: a new tracker never replays another one's graphs
        self._state = self._dry = self._records = None

    def params(self):
        return (self.max_tracks, self.iou_thresh, self.max_age, self.alpha, self.beta, self.birth_score, self.capacity)

    def _layout(self):
        """byte offsets of (tracks, append state) behind the headers in the state buffer, and its size"""
        o_tab = self.streams * 16
        o_app = o_tab + self.streams * self.max_tracks * TRACK.itemsize
        return o_tab, o_app, o_app + 32

    def _initial(self):
        o_tab, o_app, size = self._layout()
        host = np.zeros(size, np.uint8)
        host[o_tab:o_app].view(TRACK)['id'] = -1
        return host

    def _buffers(self, dev):
        """(state uint8: headers int32 [streams][4], tracks dbx_track [streams][max_tracks], append state int64 [4]; records uint8
        [capacity * 112]) on the device, allocated once"""
        if self._state is None:
            dev = self.device if self.device is not None else dev
            self._state = torch.from_numpy(self._initial()).to(dev)
            self._dry = torch.empty_like(self._state)            # the copy of the state a graph's warm-up runs advance
            self._records = torch.empty(self.capacity * RECORD.itemsize, dtype=torch.uint8, device=dev)
        return self._state, self._records

    def _key(self, dev, first):
        """what a captured graph that tracks the streams from `first` on depends on: the tracker, its buffers' addresses and the
        parameters"""
        state, records = self._buffers(dev)
        return (first, self.serial, state.data_ptr(), records.data_ptr()) + self.params()

    def reset(self):
        """forget every track, id, frame count and record; the buffers (and the graphs captured on them) stay"""
        if self._state is not None:
            self._state.copy_(torch.from_numpy(self._initial()))

    def _host_state(self):
        o_tab, o_app, _ = self._layout()
        host = self._initial() if self._state is None else self._state[:o_app].cpu().numpy()
        return host[:o_tab].view(np.int32).reshape(self.streams, 4), host[o_tab:o_app].view(TRACK).reshape(self.streams, self.max_tracks)

    def headers(self):
        """one copy: int32 [streams, 4] = (frames seen, ids given, detections that got no track, reserved)"""
        return self._host_state()[0].copy()

    def live(self):
        """one copy of the state; per stream the structured array (TRACK) of its live slots, in slot order"""
        _, tracks = self._host_state()
        return [tracks[s][tracks[s]['id'] >= 0].copy() for s in range(self.streams)]

    def finished(self):
        """One copy of the append state, then one copy of exactly the records written: the structured array (RECORD: stream, track) of
        the tracks that were retired, in the order they ended (call by call, stream by stream, slot by slot).  Raises when records were
        dropped because the arena was full."""
        if self._state is None:
            return np.zeros(0, RECORD)
        o_app = self._layout()[1]
        cursor, dropped = (int(v) for v in self._state[o_app:o_app + 16].cpu().numpy().view(np.int64))
        if dropped > 0:
            raise RuntimeError('Tracker: %d records did not fit the arena of capacity=%d; track with a larger capacity'
                               % (dropped, self.capacity))
        return np.zeros(0, RECORD) if cursor == 0 else self._records[:cursor * RECORD.itemsize].cpu().numpy().view(RECORD)


# ------------------------------------------------------------------------------------------------------------ the launches
def _launch(tr, rows, stream0, dry=False, gallery=None, between=None):
    """dbx_track_update_batch + dbx_track_append on the device rows `rows` (rows.Rows), for streams stream0 .. stream0 + B - 1 of tracker
    `tr`.  gallery = (gal, crops, ok): dbx_track_gallery_update runs between the two, crops uint8 [B, slots, oh, ow, c] and ok int32
    [B, slots] being what dbx_plate_crops_batch wrote with sel = keep.  dry: the launches advance a scratch copy of the state and
    append nothing, and the gallery's reads it and writes nothing (commit = 0).  between(base, o_tab): called behind the update (and
    the gallery's launch) and before the append with the address of the state the update advanced and the table's offset in it, for
    launches that read the table there (zones._launch).  Returns device tensors (ids int32 [2, B, slots] =
    (track_id, track_hits), track_slot int32 [B, slots], retired uint8, tally int32 [B, 6])."""
    dev, B, slots = rows.dets.device, rows.B, rows.slots
    state, records = tr._buffers(dev)
    if dry:
        tr._dry.copy_(state)
        state = tr._dry
    o_tab, o_app, _ = tr._layout()
    base = state.data_ptr()
    ids = torch.empty((2, B, slots), dtype=torch.int32, device=dev)
    slot = torch.empty((B, slots), dtype=torch.int32, device=dev)
    retired = torch.empty(B * tr.max_tracks * TRACK.itemsize, dtype=torch.uint8, device=dev)
    tally = torch.empty((B, 6), dtype=torch.int32, device=dev)
    L = _lib.lib()
    check(L.dbx_track_update_batch(*rows.args(), C.c_void_p(base), C.c_void_p(base + o_tab), tr.streams, stream0, tr.max_tracks,
                                   tr.iou_thresh, tr.max_age, tr.alpha, tr.beta, tr.birth_score, ptr(ids[0]), ptr(slot), ptr(ids[1]),
                                   ptr(retired), ptr(tally), stream_ptr()))
    if gallery is not None:
        from .gallery import POLICIES, SHOT, SHOT_RECORD
        gal, crops, ok = gallery
        live, arena, gstate = gal._buffers(dev)
        n = tr.streams * tr.max_tracks
        check(L.dbx_track_gallery_update(C.c_void_p(base + o_tab), C.c_void_p(base), ptr(slot), ptr(crops), ptr(ok), ptr(retired), ptr(tally),
                                         C.c_void_p(base + o_app), ptr(live), C.c_void_p(live.data_ptr() + n * SHOT.itemsize), ptr(arena),
                                         C.c_void_p(arena.data_ptr() + gal.capacity * SHOT_RECORD.itemsize), ptr(gstate), B, slots,
                                         tr.streams, stream0, tr.max_tracks, gal.oh, gal.ow, gal.channels, gal.capacity,
                                         POLICIES[gal.policy], gal.min_score, 0 if dry else 1, stream_ptr()))
    if between is not None:
        between(base, o_tab)
    check(L.dbx_track_append(ptr(retired), ptr(tally), B, tr.max_tracks, stream0, None if dry else ptr(records), 0 if dry else tr.capacity,
                             C.c_void_p(base + o_app), stream_ptr()))
    return ids, slot, retired, tally


def _check_streams(fn, tracker, stream0, n):
    if not isinstance(tracker, Tracker):
        raise RuntimeError('%s: tracker must be a track.Tracker, got %s' % (fn, type(tracker).__name__))
    if not _integer(stream0) or stream0 < 0 or stream0 + n > tracker.streams:
        raise RuntimeError('%s: stream0=%r with %d images does not fit the tracker\'s %d streams' % (fn, stream0, n, tracker.streams))


def update_batch(dets, keeps, *, tracker, stream0=0):
    """The host results of any detect_* call tracked with ONE upload, the two launches and one copy back: entry j is the next frame of
    stream stream0 + j.

    dets, keeps: per image the float64 rows [n, 5|13] (numpy arrays or tensors) and the keep list, as detect_batch, detect_batch_thresh,
    detect_batch_resized and detect_pyramid return them; an image may have no rows and an empty list (its tracks coast).  At most 1024
    rows per image.

    Returns, per image, (track_id int32 [k], track_hits int32 [k]) for the k entries of its keep list in order: the id of the track the
    row continued or started (-1: none, the table was full or the row may not start one) and the number of rows that track has had."""
    fn = 'update_batch'
    p = R.pack_host(fn, dets, keeps, max_slots=MAX_SLOTS)
    _check_streams(fn, tracker, stream0, p.B)
    rows = p.upload(tracker.device if tracker.device is not None else torch.device('cuda'))      # the one upload
    h = _launch(tracker, rows, int(stream0))[0].cpu().numpy()                                      # the one copy back
    return [(h[0, i, :k.size].copy(), h[1, i, :k.size].copy()) for i, k in enumerate(p.lists)]


# ------------------------------------------------------------------------------------------------------------ net.track_batch
def _track_eager(tr, K, thresh, stream0, nms_thresh, dry_outside_capture):
    """The eager function of track_batch's chunks, for the streams from stream0 on: forward, decode (+ NMS), dbx_track_update_batch,
    dbx_track_append.  thresh: None for the top-K decode of K rows, or (score_thresh, max_dets).  Under _graph_replay the function also
    runs twice as a warm-up before the capture: with dry_outside_capture those runs advance a scratch copy of the state, so only replays
    count.  Returns the tensors that go to the host first, then every other tensor the launches wrote: a graph entry keeps them all,
    which pins the buffers its replays use."""
    def eager(net, images):
        s, l, hm, ll = DC._forward_maps(net, images)
        B = int(images.size(0))
        dry = dry_outside_capture and not torch.cuda.is_current_stream_capturing()
        rows, extra = R.decode_rows(s, l, hm, ll, B, K, thresh, nms_thresh)
        return (rows.dets, rows.keep) + extra + _launch(tr, rows, stream0, dry)
    return eager


_TOPK_HOST = (True, True, True, False, False, False)
_THRESH_HOST = (False, False, True, True, False, False, False)


def _unpack(mode, res, dc):
    """per image (dets, keep, track_id, track_hits) from a chunk's results: host tensors where the flags above say so, device otherwise"""
    if mode == 'topk':
        d, k, ids = res[0].numpy(), res[1].numpy(), res[2].numpy()
        packed = [(d[b].copy(), _keep_list(k[b])) for b in range(d.shape[0])]
    else:
        dets, keep, counts, ids = res[0], res[1], res[2].numpy().copy(), res[3].numpy()
        B = (counts.shape[0] - 1) // 3
        total = int(counts[3 * B])
        # the two copies whose sizes the counts decide
        packed = DC._unpack_packed(counts[2 * B:], dets[:total].cpu().numpy(), keep[:total + B].cpu().numpy(), dc)
    return [(d, kl, ids[0, b, :len(kl)].copy(), ids[1, b, :len(kl)].copy()) for b, (d, kl) in enumerate(packed)]


def track_batch(net, images, *, tracker, stream0=0, K=10, score_thresh=None, max_dets=1024, nms_thresh=0.4, max_batch=32):
    """Detection and tracking in one go: image j is the next frame of camera stream stream0 + j.  Per chunk of at most `max_batch` frames
    the forward, dbx_detect_batch (top-K) or dbx_detect_thresh_batch (score_thresh given: every pixel above it, at most max_dets per
    frame; a non-default K together with it raises), dbx_track_update_batch on the rows and keep lists where the decode left them, and
    dbx_track_append into `tracker`; chunk c starts at stream stream0 + c * max_batch.  The tracker's state never leaves the device;
    tracker.live() and tracker.finished() read it.

    images: a float [B,3,H,W] or uint8 [B,H,W,3] tensor, or a list of single frames of ONE shape (frames of other sizes go through
    detect_batch_resized / detect_pyramid and track.update_batch).  K and max_dets are at most 1024.

    Returns, per image in input order, (dets, keep, track_id, track_hits): dets and keep bit for bit detect_batch's or
    detect_batch_thresh's; track_id int32 [len(keep)], the id of the track row keep[j] continued or started (-1: none); track_hits int32
    [len(keep)], the rows that track has had, this one included (0 without a track).

    Eval mode replays ONE hipGraph per chunk from the cache detect() uses, under a tag of its own, keyed by (batch shape, dtype, (decode
    mode and its sizes, the chunk's first stream, the tracker, its buffers and its parameters), nms_thresh, compute dtype): the forward,
    the decode, the two tracking launches and the copies of dets, keep and the [2, B, slots] ids (top-K) or of the counts and the ids
    (threshold; the rows and lists then come with two copies of exactly their size) to pinned memory.  Every chunk position owns an
    entry and the cache holds _MAX_GRAPHS = 8 per network, so keep streams / max_batch at or below that.  The capture's warm-up runs
    advance a scratch copy of the state.  Train mode and DBX_GRAPH=0 run the same launches eagerly."""
    fn = 'track_batch'
    _check_streams(fn, tracker, stream0, DC._frame_count(fn, images))
    tc = DC._thresh_or_topk(fn, K, score_thresh, max_dets)
    if tc is None:
        R._check_K(fn, K, MAX_SLOTS)
    if tc is not None and tc[1] > MAX_SLOTS:
        raise RuntimeError('%s: max_dets=%r must be an integer in 1..%d' % (fn, max_dets, MAX_SLOTS))
    DC._one_shape(fn, images, with_dtype=True)
    mode = ('topk', int(K)) if tc is None else ('thresh', tc[1], tc[0])
    flags = _TOPK_HOST if tc is None else _THRESH_HOST
    dry, dc = DC._use_graph(net), DC._det_cols(net)

    def chunk(x, idx):
        first = int(stream0) + idx[0]
        key = (mode + tracker._key(x.device, first), float(nms_thresh))
        res = DC._run_chunk(net, 'track', x, key, _track_eager(tracker, int(K), tc, first, nms_thresh, dry), flags)
        return _unpack(mode[0], res, dc)
    return DC._detect_many(fn, images, max_batch, chunk, with_index=True)
