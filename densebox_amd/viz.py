"""Annotated frames on the GPU: what the reference's ``viz_result`` (DenseBox.py:3484-3560) draws with OpenCV -- the box, a filled label
with the score, a disc per landmark, the rectified plate next to the box -- painted by ONE dbx_draw_overlay_batch launch behind the
decode, the plate crops and the tracking update, so a frame never travels to the host to be looked at.

The layout, default colours, thickness, radius and anchor points are viz_result's; the pixel semantics are this project's own
(include/densebox_hip.h has the contract, tests/viz_ref.py restates it in NumPy).  OpenCV is not part of the reference tree: parity with
cv2.rectangle / putText / circle is unpinned."""
import ctypes as C

import numpy as np

from . import _lib, frames as F, rows as R
from ._lib import check, stream_ptr
from .decode import _host

MAX_SLOTS = 1024             # dbx_draw_overlay_batch's bound on the list positions of a frame (the rows a tile meets live in LDS)
assert C.sizeof(_lib.OverlayStyle) == 28


class Style:
    """How dbx_draw_overlay_batch paints.  box_color: the outline and the label's background; text_color: the label's text; mark_color:
    the landmark discs -- channel ch of a painted pixel takes color[ch], so the order is the frame's (a missing entry is 0).  thickness
    1..16 of the outline; radius -1 (no discs) .. 32; font_scale 0 (no label) .. 8, the pixels per font pixel; inset_scale 1..8, the
    pixels per crop pixel.  The defaults are viz_result's values."""

    def __init__(self, box_color=(0, 215, 255), text_color=(225, 255, 255), mark_color=(0, 0, 255), thickness=2, radius=5, font_scale=2,
                 inset_scale=1):
        self.box_color, self.text_color, self.mark_color = (F._color('Style', n, v) for n, v in (
            ('box_color', box_color), ('text_color', text_color), ('mark_color', mark_color)))
        self.thickness, self.radius, self.font_scale, self.inset_scale = (F._bounded('Style', n, v, lo, hi) for n, v, lo, hi in (
            ('thickness', thickness, 1, 16), ('radius', radius, -1, 32), ('font_scale', font_scale, 0, 8), ('inset_scale', inset_scale, 1, 8)))

    def key(self):
        """everything a launch bakes in, hashable"""
        return (self.box_color, self.text_color, self.mark_color, self.thickness, self.radius, self.font_scale, self.inset_scale)

    def record(self):
        u4 = C.c_uint8 * 4
        return _lib.OverlayStyle(u4(*self.box_color), u4(*self.text_color), u4(*self.mark_color), self.thickness, self.radius,
                                 self.font_scale, self.inset_scale)


def label(score, track_id=None):
    """the text dbx_draw_overlay_batch writes for a row: '#<id> ' for an id >= 0, then '%.3f' of the score ('---' when it is not finite
    or |score| >= 1000); the library's own code, compiled for the host"""
    buf = C.create_string_buffer(32)
    n = _lib.lib().dbx_overlay_label(float(score), -1 if track_id is None else int(track_id), buf, 32)
    if n < 0:
        check(n)
    return buf.value.decode()


def font():
    """the library's 14 glyphs of '0123456789.-# ' as uint8 [14, 8]: row j of glyph g, bit i = column i"""
    out = np.zeros((14, 8), np.uint8)
    check(_lib.lib().dbx_overlay_font(out.ctypes.data_as(C.c_void_p)))
    return out


def _draw_launch(table, c, max_h, max_w, rows, track_id, crops, ok, ow, oh, style):
    """ONE dbx_draw_overlay_batch launch on the current stream over the device rows `rows` (rows.Rows) and device tensors (or raw
    addresses given as ints); nothing is copied from the host and nothing waits, so a graph capture may hold it"""
    rec = style.record()
    check(_lib.lib().dbx_draw_overlay_batch(F._p(table), rows.B, c, max_h, max_w, *rows.args(batch=False), F._p(track_id), F._p(crops), F._p(ok),
                                            ow, oh, C.byref(rec), stream_ptr()))


def draw_batch(images, dets, keeps, *, track_ids=None, crops=None, ok=None, style=None):
    """The results of any detect_* / track_* call drawn onto their frames with ONE upload and ONE dbx_draw_overlay_batch launch.

    images: a uint8 [B,H,W,C] tensor or a list of uint8 [H,W,C] images of any sizes (numpy arrays or tensors, on the CPU or the GPU; C
    is 1..4 and the same for all), as for rectify.perspective_transform_batch.  dets, keeps: per image the float64 rows [n, 5|13] and
    the keep list, host or device, as every detect_* call returns them; at most 1024 rows per image.  track_ids: per image the ids of
    the kept rows (track_batch's track_id), or None.  crops, ok: per image uint8 [len(keep), oh, ow, C] and the flags [len(keep)], as
    detect_plate_crops returns them (one crop size for the call), or both None for no inset.  style: a viz.Style.

    Returns the annotated frames in input order, each of the kind of its input (numpy array, CPU tensor or CUDA tensor; CUDA results
    are views into one device arena).  The inputs are unchanged.  include/densebox_hip.h states what is painted."""
    from . import rectify
    fn = 'draw_batch'
    st = F._style(fn, style, Style, 'viz.Style')
    host, kinds = rectify.host_images(fn, images, None)
    B, c = len(host), int(host[0].size(2))
    pk = R.pack_host(fn, dets, keeps, max_slots=MAX_SLOTS, n=B)
    lists, slots = pk.lists, pk.slots
    if track_ids is not None:
        if not isinstance(track_ids, (list, tuple)) or len(track_ids) != B:
            raise RuntimeError('%s: track_ids must be a list with one entry per image' % fn)
        ids = [np.asarray(_host(t), np.int64).reshape(-1) for t in track_ids]
        if any(t.size != k.size for t, k in zip(ids, lists)):
            raise RuntimeError('%s: every track_ids entry must hold one id per kept row' % fn)
    if (crops is None) != (ok is None):
        raise RuntimeError('%s: crops and ok must be given together' % fn)
    ow = oh = 0
    if crops is not None:
        if not isinstance(crops, (list, tuple)) or not isinstance(ok, (list, tuple)) or len(crops) != B or len(ok) != B:
            raise RuntimeError('%s: crops and ok must be lists with one entry per image' % fn)
        cr = [_host(x) for x in crops]
        oks = [np.asarray(_host(x)).reshape(-1) != 0 for x in ok]
        shapes = {tuple(x.shape[1:]) for x in cr if x.ndim == 4}
        if any(x.ndim != 4 or x.dtype != np.uint8 for x in cr) or len(shapes) != 1 or next(iter(shapes))[2] != c or 0 in next(iter(shapes)):
            raise RuntimeError('%s: every crops entry must be uint8 [k, oh, ow, %d] of one size; got %s' % (fn, c, [list(x.shape) for x in cr]))
        if any(x.shape[0] != k.size or o.size != k.size for x, o, k in zip(cr, oks, lists)):
            raise RuntimeError('%s: crops and ok must hold one entry per kept row' % fn)
        oh, ow = next(iter(shapes))[:2]

    # the ONE upload: rows, keep lists, ids, flags, the frame table, then the frames that are on the host and the crops
    ni, crop_bytes = B * slots * 4, oh * ow * c
    up = F.Upload(host, kinds, pk, before=[('ids', ni), ('ok', ni)], after=[('crops', B * slots * crop_bytes if crops is not None else 0)])
    hi, ho = (up.view(n).view(np.int32).reshape(B, slots) for n in ('ids', 'ok'))
    hi[:] = -1
    for i, k in enumerate(lists):
        if track_ids is not None:
            hi[i, :k.size] = np.clip(ids[i], -1, 2 ** 31 - 1)
        if crops is not None and k.size:
            ho[i, :k.size] = oks[i]
            up.view('crops')[i * slots * crop_bytes:(i * slots + k.size) * crop_bytes] = cr[i].reshape(-1)
    _draw_launch(up.table, c, up.max_h, up.max_w, up.send(), up.addr('ids') if track_ids is not None else None,
                 up.addr('crops') if crops is not None else None, up.addr('ok') if crops is not None else None, ow, oh, st)
    return up.results()


# ------------------------------------------------------------------------------------------------------------ net.annotate_batch
def annotate_batch(net, frames, *, tracker=None, stream0=0, inset=None, K=10, nms_thresh=0.4, max_batch=32, style=None):
    """Detection, optionally tracking, and the annotated frames in one go: per chunk of at most `max_batch` frames the forward,
    dbx_detect_batch, dbx_plate_crops_batch when inset=(width, height) is given (every kept row's plate rectified to that size and shown
    under its box; DenseBoxLM / DenseBoxLMLOC only), dbx_track_update_batch + dbx_track_append when a tracker is given (frame j is the next
    frame of camera stream stream0 + j, as in track_batch; the label then starts with the track's id), and ONE dbx_draw_overlay_batch.

    frames: uint8 frames only -- a [B,H,W,3] tensor or a list of [H,W,3] images (numpy arrays or tensors) of ONE shape.  Top-K decode
    only, for the reason detect_plate_crops gives; viz.draw_batch draws the host results of every other call.

    Returns, per frame in input order, (dets, keep, track_id or None, annotated): dets, keep and track_id bit for bit detect_batch's /
    track_batch's; annotated uint8 [H,W,3] of the kind of the frame (numpy array, CPU tensor or CUDA tensor); the frames of a chunk share one
    buffer that the call owns.

    Eval mode replays ONE hipGraph per chunk from the cache detect() uses, under a tag of its own, keyed by (batch shape, dtype, (K, the
    inset size, the style, frames to the host, and with a tracker the chunk's first stream, the tracker, its buffers and its
    parameters), nms_thresh, compute dtype).  The capture's warm-up runs advance a scratch copy of the tracker's state.  Train mode and
    DBX_GRAPH=0 run the same launches eagerly."""
    from . import decode as DC, rectify
    fn = 'annotate_batch'
    st = F._style(fn, style, Style, 'viz.Style')
    if inset is not None:
        DC._require_landmarks(fn, net, to='rectify for the inset')
        inset = rectify._crop_size(fn, inset)
    ow, oh = inset or (0, 0)

    def crops_of(images, rows, memo, rest):
        """dbx_plate_crops_batch over the kept rows, its frame table made once per input tensor"""
        if not inset:
            return None, None
        if 'table' not in memo:
            memo['table'] = rectify.frame_table(list(images.unbind(0)))
        crops, ok = rectify._crops_launch(memo['table'], rows.B, 3, rows.dets.data_ptr() + 5 * 8, rows.dc, rows.slots * rows.dc, rows.keep,
                                          rows.slots, ow, oh, images.device)
        rest += [crops, ok, memo['table']]
        return crops, ok

    def draw(table, rows, H, W, first, ids, dry, crops_ok):
        _draw_launch(table, 3, H, W, rows, None if ids is None else ids[0], *crops_ok, ow, oh, st)
    return F.run_net(fn, 'annotate', net, frames, tracker=tracker, stream0=stream0, K=K, nms_thresh=nms_thresh, max_batch=max_batch,
                     max_slots=MAX_SLOTS, key_parts=(inset, st.key()), n_rest=1 + (3 if inset else 0), paint=draw, between=crops_of)
