"""Plate redaction on the GPU: the frame with every detected plate -- and every coasting track's predicted box, for the frames in which
the detector missed it -- filled, pixelated or blurred by ONE dbx_redact_batch launch behind the decode and the tracking update, so a
frame never travels to the host to be made publishable.

No reference counterpart: the semantics are this project's own (include/densebox_hip.h has the contract, tests/redact_ref.py restates
it in NumPy)."""
import ctypes as C

import numpy as np
import torch

from . import _lib, decode as DC, rows as R
from ._lib import check, ptr, stream_ptr
from .decode import _integer, _keep_list
from .track import TRACK, _number
from .viz import _color, _frame_records, _up, overlay_table

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
        try:
            self.color = _color('color', color)
        except RuntimeError as e:
            raise RuntimeError(str(e).replace('Style:', 'Redaction:', 1)) from None
        for name, v, lo, hi in (('cell', cell, 2, 32), ('radius', radius, 1, 16), ('grow', grow, 0, 64), ('grow_pct', grow_pct, 0, 100)):
            if not _integer(v) or not lo <= v <= hi:
                raise RuntimeError('Redaction: %s=%r must be an integer in %d..%d' % (name, v, lo, hi))
        if coast is not None and (not _integer(coast) or coast < 0 or coast >= 1 << 31):
            raise RuntimeError('Redaction: coast=%r must be None or a non-negative integer' % (coast,))
        if not _number(min_score):
            raise RuntimeError('Redaction: min_score=%r must be a number' % (min_score,))
        self.method, self.shape = method, shape
        self.cell, self.radius, self.grow, self.grow_pct = int(cell), int(radius), int(grow), int(grow_pct)
        self.coast, self.min_score = None if coast is None else int(coast), float(min_score)

    def key(self):
        """everything a launch bakes in, hashable (shape and coast unresolved: the rows' columns and the tracker are keyed elsewhere)"""
        return (self.method, self.shape, self.cell, self.radius, self.color, self.grow, self.grow_pct, self.coast, self.min_score)

    def record(self, det_cols=5, max_age=0):
        """the dbx_redact_style for rows of det_cols columns and a tracker of that max_age"""
        shape = SHAPES[self.shape] if self.shape is not None else int(det_cols == 13)
        return _lib.RedactStyle((C.c_uint8 * 4)(*self.color), METHODS[self.method], shape, self.cell, self.radius, self.grow, self.grow_pct,
                                int(max_age) if self.coast is None else self.coast, self.min_score)


def _style(fn, style):
    if style is None:
        return Redaction()
    if not isinstance(style, Redaction):
        raise RuntimeError('%s: style must be a redact.Redaction, got %s' % (fn, type(style).__name__))
    return style


def _redact_launch(table, c, max_h, max_w, rows, tracks, streams, stream0, max_tracks, record):
    """ONE dbx_redact_batch launch on the current stream over the device rows `rows` (rows.Rows) and device tensors (or raw addresses
    given as ints); nothing is copied from the host and nothing waits, so a graph capture may hold it"""
    def p(t):
        return C.c_void_p(t) if isinstance(t, int) else ptr(t)
    check(_lib.lib().dbx_redact_batch(p(table), rows.B, c, max_h, max_w, *rows.args(batch=False), p(tracks), streams, stream0, max_tracks,
                                      C.byref(record), stream_ptr()))


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
    st = _style(fn, style)
    host, kinds = rectify.host_images(fn, images, None)
    B, c = len(host), int(host[0].size(2))
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
    nd, nk, nt = pk.nd, pk.nk, B * mt * TRACK.itemsize
    o_keep, o_trk = nd, _up(nd + nk, 8)
    o_tab = o_trk + nt
    at = _up(o_tab + B * 24)
    o_src = []
    for im, kind in zip(host, kinds):
        o_src.append(None if kind == 'cuda' else at)
        if kind != 'cuda':
            at = _up(at + im.numel())
    total = at
    o_dst, out_bytes = [], 0
    for im in host:
        o_dst.append(out_bytes)
        out_bytes = _up(out_bytes + im.numel())
    dev = next((im.device for im in host if im.is_cuda), torch.device('cuda'))
    up = torch.empty(total, dtype=torch.uint8, device=dev)
    arena = torch.empty(out_bytes, dtype=torch.uint8, device=dev)            # always out of place: pixelate and blur need it
    src_dev = [im.contiguous() if kind == 'cuda' else None for im, kind in zip(host, kinds)]
    h = np.zeros(total, np.uint8)
    pk.write(h, 0, o_keep)
    if tracks is not None:
        ht = h[o_trk:o_tab].view(TRACK).reshape(B, mt)
        ht['id'] = -1
        for i, t in enumerate(trs):
            ht[i, :t.size] = t
    srcs = [up.data_ptr() + o if s is None else s.data_ptr() for o, s in zip(o_src, src_dev)]
    rec = _frame_records(srcs, [arena.data_ptr() + o for o in o_dst], [(int(im.size(0)), int(im.size(1))) for im in host])
    h[o_tab:o_tab + B * 24] = np.frombuffer(rec, np.uint8)
    for im, o in zip(host, o_src):
        if o is not None:
            h[o:o + im.numel()] = im.contiguous().numpy().reshape(-1)
    up.copy_(torch.from_numpy(h))
    base = up.data_ptr()
    _redact_launch(base + o_tab, c, max(int(im.size(0)) for im in host), max(int(im.size(1)) for im in host), pk.on(up, 0, o_keep),
                   base + o_trk if tracks is not None else None, B, 0, mt, st.record(pk.dc, (1 << 31) - 1))
    down = arena.cpu() if any(k != 'cuda' for k in kinds) else None        # (behind the launch on the stream: `up` and the frames are done with)
    out = []
    for im, kind, o in zip(host, kinds, o_dst):
        v = (arena if kind == 'cuda' else down)[o:o + im.numel()].view(im.shape)
        out.append(v.numpy() if kind == 'numpy' else v)
    return out


# ------------------------------------------------------------------------------------------------------------ net.redact_batch
def _redact_eager(K, tr, first, nms_thresh, style, dry_outside_capture):
    """The eager function of net.redact_batch's chunks: forward, dbx_detect_batch, the two tracking launches (tracker given),
    dbx_redact_batch, which reads the tracker's table as the update left it (its scratch copy in the capture's warm-up runs).  The
    frame table and the output frames are made on the first call for an input tensor (the warm-up, outside the capture) and reused for
    the same address afterwards.  Returns (dets, keep[, ids], redacted), then every other tensor the launches read or wrote: a graph
    entry keeps them all."""
    from . import track as T
    made = {}

    def eager(net, images):
        s, l, hm, ll = DC._forward_maps(net, images)
        B, H, W = int(images.size(0)), int(images.size(1)), int(images.size(2))
        dets, _, keep = DC._run_batch(s, l, K, lm_heat=hm, lm_loc=ll, nms_thresh=nms_thresh)
        rows = R.Rows(dets, keep, None, B, K)
        key = (images.data_ptr(), tuple(images.shape))
        if key not in made:
            out = torch.empty_like(images)
            made[key] = (out, overlay_table(list(images.unbind(0)), list(out.unbind(0))))
        out, table = made[key]
        res, rest = [dets, keep], [table]
        table_at, streams, max_tracks, max_age = None, 0, 0, 0
        if tr is not None:
            dry = dry_outside_capture and not torch.cuda.is_current_stream_capturing()
            ids, slot, retired, tally = T._launch(tr, rows, first, dry)
            res.append(ids)
            rest += [slot, retired, tally]
            state = tr._dry if dry else tr._buffers(images.device)[0]
            table_at, streams, max_tracks, max_age = state.data_ptr() + tr._layout()[0], tr.streams, tr.max_tracks, tr.max_age
        _redact_launch(table, 3, H, W, rows, table_at, streams, first, max_tracks, style.record(rows.dc, max_age))
        return tuple(res + [out] + rest)
    return eager


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
    from . import rectify, track as T
    fn = 'redact_batch'
    st = _style(fn, style)
    host, kinds = rectify.host_images(fn, frames, 3)
    if len({tuple(im.shape) for im in host}) > 1:
        raise RuntimeError('%s: the frames of a list must have one shape (stream j is image j), got %s'
                           % (fn, sorted({str(tuple(im.shape)) for im in host})))
    if tracker is not None:
        T._check_streams(fn, tracker, stream0, len(host))
    R._check_K(fn, K, MAX_SLOTS)
    if not _integer(max_batch) or max_batch < 1:
        raise RuntimeError('%s: max_batch=%r must be a positive integer' % (fn, max_batch))
    K = int(K)
    to_host = any(k != 'cuda' for k in kinds)
    x = DC._on_device(frames) if torch.is_tensor(frames) else rectify.to_device(frames, host)
    dry = DC._use_graph(net)

    def chunk(x, idx):
        first = int(stream0) + idx[0]
        key = ('topk', K, st.key(), to_host)
        if tracker is not None:
            key += tracker._key(x.device, first)
        eager = _redact_eager(K, tracker, first, nms_thresh, st, dry)
        n_res = 4 if tracker is not None else 3
        flags = (True,) * (n_res - 1) + (to_host,) + (False,) * (1 + (3 if tracker is not None else 0))
        res = DC._run_chunk(net, 'redact', x, (key, float(nms_thresh)), eager, flags)
        d, k = res[0].numpy(), res[1].numpy()
        ids = res[2].numpy() if tracker is not None else None
        # the results own their memory (a graph entry's buffers are overwritten by its next replay): the chunk's frames by ONE clone
        red = res[n_res - 1].clone()
        out = []
        for b in range(d.shape[0]):
            keep = _keep_list(k[b])
            out.append((d[b].copy(), keep, None if ids is None else ids[0, b, :len(keep)].copy(), red[b]))
        return out
    res = DC._detect_many(fn, x, max_batch, chunk, with_index=True)
    out = []
    for (d, keep, tid, red), kind in zip(res, kinds):
        if kind == 'cuda' and not red.is_cuda:
            red = red.cuda()                                         # (a CUDA frame in a list that also holds host frames)
        out.append((d, keep, tid, red.numpy() if kind == 'numpy' else red))
    return out
