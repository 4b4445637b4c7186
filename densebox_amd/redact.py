"""Plate redaction on the GPU: the frame with every detected plate -- and every coasting track's predicted box, for the frames in which
the detector missed it -- filled, pixelated or blurred by ONE dbx_redact_batch launch behind the decode and the tracking update, so a
frame never travels to the host to be made publishable.

No reference counterpart: the semantics are this project's own (include/densebox_hip.h has the contract, tests/redact_ref.py restates
it in NumPy)."""
import ctypes as C

import numpy as np

from . import _lib, frames as F, rows as R
from ._lib import check, stream_ptr
from .decode import _integer
from .track import TRACK, _number

MAX_SLOTS = 1024             # dbx_redact_batch's bound on the list positions of a frame (the regions a tile meets live in LDS)
MAX_TRACKS = 256             # ... and on the track slots of a stream
METHODS = {'fill': 0, 'pixelate': 1, 'blur': 2}
SHAPES = {'box': 0, 'quad': 1}
assert C.sizeof(_lib.RedactStyle) == 40 and _lib.RedactStyle.min_score.offset == 32


class Redaction:
    """How dbx_redact_batch makes a plate unreadable.  method: 'fill' (channel ch takes color[ch]), 'pixelate' (cells of `cell` pixels,
    2..32, anchored to the frame's origin, each replaced by its rounded mean) or 'blur' (the exact (2 radius + 1)^2 box mean, radius
    1..16, edges replicated).  shape: 'box', 'quad' (the four landmarks of a 13-column row; a row without usable landmarks falls back to
    its box) or None: quad when the rows have 13 columns, else box.  grow 0..64 pixels and grow_pct 0..100 per cent of the region's size
    are added on every side.  coast: tracks that have gone 1..coast frames without a match are redacted at their predicted box; 0: none;
    None: the tracker's max_age, that is every coasting track.  min_score: rows below it are left readable.

    The defaults are a convention, NOT tuned values: no trained weights exist in this tree to tune them with."""

    def __init__(self, method='pixelate', shape=None, cell=12, radius=8, color=(0, 0, 0), grow=2, grow_pct=10, coast=None,
                 min_score=-float('inf')):
        if method not in METHODS:
            raise RuntimeError('Redaction: method=%r must be one of %s' % (method, sorted(METHODS)))
        if shape is not None and shape not in SHAPES:
            raise RuntimeError('Redaction: shape=%r must be None or one of %s' % (shape, sorted(SHAPES)))
        self.color = F._color('Redaction', 'color', color)
        self.cell, self.radius, self.grow, self.grow_pct = (F._bounded('Redaction', n, v, lo, hi) for n, v, lo, hi in (
            ('cell', cell, 2, 32), ('radius', radius, 1, 16), ('grow', grow, 0, 64), ('grow_pct', grow_pct, 0, 100)))
        if coast is not None and (not _integer(coast) or coast < 0 or coast >= 1 << 31):
            raise RuntimeError('Redaction: coast=%r must be None or a non-negative integer' % (coast,))
        if not _number(min_score):
            raise RuntimeError('Redaction: min_score=%r must be a number' % (min_score,))
        self.method, self.shape = method, shape
        self.coast, self.min_score = None if coast is None else int(coast), float(min_score)

    def key(self):
        """everything a launch bakes in, hashable (shape and coast unresolved: the rows' columns and the tracker are keyed elsewhere)"""
        return (self.method, self.shape, self.cell, self.radius, self.color, self.grow, self.grow_pct, self.coast, self.min_score)

    def record(self, det_cols=5, max_age=0):
        """the dbx_redact_style for rows of det_cols columns and a tracker of that max_age"""
        shape = SHAPES[self.shape] if self.shape is not None else int(det_cols == 13)
        return _lib.RedactStyle((C.c_uint8 * 4)(*self.color), METHODS[self.method], shape, self.cell, self.radius, self.grow, self.grow_pct,
                                int(max_age) if self.coast is None else self.coast, self.min_score)


def _redact_launch(table, c, max_h, max_w, rows, tracks, streams, stream0, max_tracks, record):
    """ONE dbx_redact_batch launch on the current stream over the device rows `rows` (rows.Rows) and device tensors (or raw addresses
    given as ints); nothing is copied from the host and nothing waits, so a graph capture may hold it"""
    check(_lib.lib().dbx_redact_batch(F._p(table), rows.B, c, max_h, max_w, *rows.args(batch=False), F._p(tracks), streams, stream0,
                                      max_tracks, C.byref(record), stream_ptr()))


def redact_batch(images, dets, keeps, *, tracks=None, style=None):
    """The results of any detect_* / track_* call redacted on their frames with ONE upload, ONE dbx_redact_batch launch and one copy
    back.

    images: a uint8 [B,H,W,C] tensor or a list of uint8 [H,W,C] images of any sizes (numpy arrays or tensors, on the CPU or the GPU; C
    is 1..4 and the same for all), as for viz.draw_batch.  dets, keeps: per image the float64 rows [n, 5|13] and the keep list, host or
    device, as every detect_* call returns them; at most 1024 rows per image.  tracks: per image a structured track.TRACK array of at
    most 256 records, as Tracker.live()[s] returns it for the image's stream, or None; with style.coast None every coasting track in it
    is redacted.  style: a redact.Redaction.

    Returns the redacted frames in input order, each of the kind of its input (numpy array, CPU tensor or CUDA tensor; CUDA results
    are views into one device arena).  The inputs are unchanged.  include/densebox_hip.h states what is written."""
    from . import rectify
    fn = 'redact_batch'
    st = F._style(fn, style, Redaction, 'redact.Redaction')
    host, kinds = rectify.host_images(fn, images, None)
    B = len(host)
    pk = R.pack_host(fn, dets, keeps, max_slots=MAX_SLOTS, n=B)
    mt = 0
    if tracks is not None:
        if not isinstance(tracks, (list, tuple)) or len(tracks) != B:
            raise RuntimeError('%s: tracks must be a list with one entry per image' % fn)
        trs = [np.asarray(t) for t in tracks]
        if any(t.dtype != TRACK or t.ndim != 1 for t in trs):
            raise RuntimeError('%s: every tracks entry must be a one-dimensional track.TRACK array' % fn)
        mt = max(1, max(t.size for t in trs))
        if mt > MAX_TRACKS:
            raise RuntimeError('%s: %d tracks for one image exceed %d' % (fn, mt, MAX_TRACKS))

    # the ONE upload: rows, keep lists, the track table, the frame table, then the frames that are on the host
    up = F.Upload(host, kinds, pk, before=[('tracks', B * mt * TRACK.itemsize, 8)])
    if tracks is not None:
        ht = up.view('tracks').view(TRACK).reshape(B, mt)
        ht['id'] = -1
        for i, t in enumerate(trs):
            ht[i, :t.size] = t
    _redact_launch(up.table, up.c, up.max_h, up.max_w, up.send(), up.addr('tracks') if tracks is not None else None, B, 0, mt,
                   st.record(pk.dc, (1 << 31) - 1))
    return up.results()


# ------------------------------------------------------------------------------------------------------------ net.redact_batch
def net_redact_batch(net, frames, *, tracker=None, stream0=0, K=10, nms_thresh=0.4, max_batch=32, style=None):
    """Detection, optionally tracking, and the redacted frames in one go: per chunk of at most `max_batch` frames the forward,
    dbx_detect_batch, dbx_track_update_batch + dbx_track_append when a tracker is given (frame j is the next frame of camera stream
    stream0 + j, as in track_batch), and ONE dbx_redact_batch, which covers every kept row and, with a tracker, every track of the
    stream that is coasting after the update: the plate the detector missed in this frame is redacted at its predicted box.

    frames: uint8 frames only -- a [B,H,W,3] tensor or a list of [H,W,3] images (numpy arrays or tensors) of ONE shape.  Top-K decode
    only, as annotate_batch; redact.redact_batch redacts the host results of every other call.

    Returns, per frame in input order, (dets, keep, track_id or None, redacted): dets, keep and track_id bit for bit detect_batch's /
    track_batch's; redacted uint8 [H,W,3] of the kind of the frame (numpy array, CPU tensor or CUDA tensor); the frames of a chunk share
    one buffer that the call owns.

    Eval mode replays ONE hipGraph per chunk from the cache detect() uses, under a tag of its own, keyed as annotate_batch's entries
    are with the Redaction's key in place of the style's.  The capture's warm-up runs advance a scratch copy of the tracker's state and
    redact from it.  Train mode and DBX_GRAPH=0 run the same launches eagerly."""
    fn = 'redact_batch'
    st = F._style(fn, style, Redaction, 'redact.Redaction')

    def redact(table, rows, H, W, first, ids, dry, _):
        """dbx_redact_batch over the tracker's table as the update left it (its scratch copy in the capture's warm-up runs)"""
        tr, table_at, streams, max_tracks, max_age = tracker, None, 0, 0, 0
        if tr is not None:
            state = tr._dry if dry else tr._buffers(rows.dets.device)[0]
            table_at, streams, max_tracks, max_age = state.data_ptr() + tr._layout()[0], tr.streams, tr.max_tracks, tr.max_age
        _redact_launch(table, 3, H, W, rows, table_at, streams, first, max_tracks, st.record(rows.dc, max_age))
    return F.run_net(fn, 'redact', net, frames, tracker=tracker, stream0=stream0, K=K, nms_thresh=nms_thresh, max_batch=max_batch,
                     max_slots=MAX_SLOTS, key_parts=(st.key(),), n_rest=1, paint=redact)
