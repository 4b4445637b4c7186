"""Annotated frames on the GPU: what the reference's ``viz_result`` (DenseBox.py:3484-3560) draws with OpenCV -- the box, a filled label
with the score, a disc per landmark, the rectified plate next to the box -- painted by ONE dbx_draw_overlay_batch launch behind the
decode, the plate crops and the tracking update, so a frame never travels to the host to be looked at.

The layout, default colours, thickness, radius and anchor points are viz_result's; the pixel semantics are this project's own
(include/densebox_hip.h has the contract, tests/viz_ref.py restates it in NumPy).  OpenCV is not part of the reference tree: parity with
cv2.rectangle / putText / circle is unpinned."""
import ctypes as C

import numpy as np
import torch

from . import _lib, decode as DC, rows as R
from ._lib import check, ptr, stream_ptr
from .decode import _host, _integer, _keep_list

MAX_SLOTS = 1024             # dbx_draw_overlay_batch's bound on the list positions of a frame (the rows a tile meets live in LDS)
_ALIGN = 64                  # byte alignment of every frame in an arena (the kernel moves 16-byte words where src and dst allow)
assert C.sizeof(_lib.OverlayFrame) == 24 and C.sizeof(_lib.OverlayStyle) == 28


def _color(name, v):
    try:
        t = tuple(v)
    except TypeError:
        t = ()
    if not 1 <= len(t) <= 4 or not all(_integer(e) and 0 <= e <= 255 for e in t):
        raise RuntimeError('Style: %s=%r must hold 1 to 4 integers in 0..255' % (name, v))
    return tuple(int(e) for e in t) + (0,) * (4 - len(t))


class Style:
    """How dbx_draw_overlay_batch paints.  box_color: the outline and the label's background; text_color: the label's text; mark_color:
    the landmark discs -- channel ch of a painted pixel takes color[ch], so the order is the frame's (a missing entry is 0).  thickness
    1..16 of the outline; radius -1 (no discs) .. 32; font_scale 0 (no label) .. 8, the pixels per font pixel; inset_scale 1..8, the
    pixels per crop pixel.  The defaults are viz_result's values."""

    def __init__(self, box_color=(0, 215, 255), text_color=(225, 255, 255), mark_color=(0, 0, 255), thickness=2, radius=5, font_scale=2,
                 inset_scale=1):
        self.box_color, self.text_color, self.mark_color = (_color(n, v) for n, v in (
            ('box_color', box_color), ('text_color', text_color), ('mark_color', mark_color)))
        for name, v, lo, hi in (('thickness', thickness, 1, 16), ('radius', radius, -1, 32), ('font_scale', font_scale, 0, 8),
                                ('inset_scale', inset_scale, 1, 8)):
            if not _integer(v) or not lo <= v <= hi:
                raise RuntimeError('Style: %s=%r must be an integer in %d..%d' % (name, v, lo, hi))
        self.thickness, self.radius, self.font_scale, self.inset_scale = int(thickness), int(radius), int(font_scale), int(inset_scale)

    def key(self):
        """everything a launch bakes in, hashable"""
        return (self.box_color, self.text_color, self.mark_color, self.thickness, self.radius, self.font_scale, self.inset_scale)

    def record(self):
        u4 = C.c_uint8 * 4
        return _lib.OverlayStyle(u4(*self.box_color), u4(*self.text_color), u4(*self.mark_color), self.thickness, self.radius,
                                 self.font_scale, self.inset_scale)


def _style(fn, style):
    if style is None:
        return Style()
    if not isinstance(style, Style):
        raise RuntimeError('%s: style must be a viz.Style, got %s' % (fn, type(style).__name__))
    return style


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


def _frame_records(srcs, dsts, hw):
    rec = (_lib.OverlayFrame * len(srcs))()
    for r, s, d, (h, w) in zip(rec, srcs, dsts, hw):
        r.src, r.dst, r.h, r.w = s, d, h, w
    return rec


def overlay_table(src, dst):
    """The device table of dbx_overlay_frame records of contiguous uint8 [H,W,C] CUDA tensors src[b] -> dst[b] (one small upload).  It
    holds raw addresses: keep the tensors alive while the table is in use."""
    rec = _frame_records([s.data_ptr() for s in src], [d.data_ptr() for d in dst], [(int(s.size(0)), int(s.size(1))) for s in src])
    return torch.frombuffer(rec, dtype=torch.uint8).to(src[0].device)


def _draw_launch(table, c, max_h, max_w, rows, track_id, crops, ok, ow, oh, style):
    """ONE dbx_draw_overlay_batch launch on the current stream over the device rows `rows` (rows.Rows) and device tensors (or raw
    addresses given as ints); nothing is copied from the host and nothing waits, so a graph capture may hold it"""
    def p(t):
        return C.c_void_p(t) if isinstance(t, int) else ptr(t)
    rec = style.record()
    check(_lib.lib().dbx_draw_overlay_batch(p(table), rows.B, c, max_h, max_w, *rows.args(batch=False), p(track_id), p(crops), p(ok), ow, oh,
                                            C.byref(rec), stream_ptr()))


def _up(n, a=_ALIGN):
    return (n + a - 1) // a * a


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
    st = _style(fn, style)
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
    nd, nk, ni = pk.nd, pk.nk, B * slots * 4
    o_keep, o_ids, o_ok, o_tab = nd, nd + nk, nd + nk + ni, nd + nk + 2 * ni
    at = _up(o_tab + B * 24)
    o_src = []
    for im, kind in zip(host, kinds):
        o_src.append(None if kind == 'cuda' else at)
        if kind != 'cuda':
            at = _up(at + im.numel())
    o_crops = at
    crop_bytes = oh * ow * c
    total = at + (B * slots * crop_bytes if crops is not None else 0)
    o_dst, out_bytes = [], 0
    for im in host:
        o_dst.append(out_bytes)
        out_bytes = _up(out_bytes + im.numel())
    dev = next((im.device for im in host if im.is_cuda), torch.device('cuda'))
    up = torch.empty(total, dtype=torch.uint8, device=dev)
    arena = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    src_dev = [im.contiguous() if kind == 'cuda' else None for im, kind in zip(host, kinds)]
    h = np.zeros(total, np.uint8)
    pk.write(h, 0, o_keep)
    hi, ho = h[o_ids:o_ok].view(np.int32).reshape(B, slots), h[o_ok:o_tab].view(np.int32).reshape(B, slots)
    hi[:] = -1
    for i, k in enumerate(lists):
        if track_ids is not None:
            hi[i, :k.size] = np.clip(ids[i], -1, 2 ** 31 - 1)
        if crops is not None and k.size:
            ho[i, :k.size] = oks[i]
            h[o_crops + i * slots * crop_bytes:o_crops + (i * slots + k.size) * crop_bytes] = cr[i].reshape(-1)
    srcs = [up.data_ptr() + o if s is None else s.data_ptr() for o, s in zip(o_src, src_dev)]
    rec = _frame_records(srcs, [arena.data_ptr() + o for o in o_dst], [(int(im.size(0)), int(im.size(1))) for im in host])
    h[o_tab:o_tab + B * 24] = np.frombuffer(rec, np.uint8)
    for im, o in zip(host, o_src):
        if o is not None:
            h[o:o + im.numel()] = im.contiguous().numpy().reshape(-1)
    up.copy_(torch.from_numpy(h))
    base = up.data_ptr()
    _draw_launch(base + o_tab, c, max(int(im.size(0)) for im in host), max(int(im.size(1)) for im in host), pk.on(up, 0, o_keep),
                 base + o_ids if track_ids is not None else None, base + o_crops if crops is not None else None,
                 base + o_ok if crops is not None else None, ow, oh, st)
    down = arena.cpu() if any(k != 'cuda' for k in kinds) else None        # (behind the launch on the stream: `up` and the frames are done with)
    out = []
    for im, kind, o in zip(host, kinds, o_dst):
        v = (arena if kind == 'cuda' else down)[o:o + im.numel()].view(im.shape)
        out.append(v.numpy() if kind == 'numpy' else v)
    return out


# ------------------------------------------------------------------------------------------------------------ net.annotate_batch
def _annotate_eager(K, inset, tr, first, nms_thresh, style, dry_outside_capture):
    """The eager function of annotate_batch's chunks: forward, dbx_detect_batch, dbx_plate_crops_batch (inset given), the two tracking
    launches (tracker given), dbx_draw_overlay_batch.  The two frame tables and the output frames are made on the first call for an
    input tensor (the warm-up, outside the capture) and reused for the same address afterwards.  Returns (dets, keep[, ids], annotated),
    then every other tensor the launches read or wrote: a graph entry keeps them all."""
    from . import rectify, track as T
    made = {}

    def eager(net, images):
        s, l, hm, ll = DC._forward_maps(net, images)
        B, H, W = int(images.size(0)), int(images.size(1)), int(images.size(2))
        dets, _, keep = DC._run_batch(s, l, K, lm_heat=hm, lm_loc=ll, nms_thresh=nms_thresh)
        rows = R.Rows(dets, keep, None, B, K)
        dc = rows.dc
        key = (images.data_ptr(), tuple(images.shape))
        if key not in made:
            out = torch.empty_like(images)
            frames = list(images.unbind(0))
            made[key] = (out, overlay_table(frames, list(out.unbind(0))), rectify.frame_table(frames) if inset else None)
        out, table, crop_table = made[key]
        res, rest = [dets, keep], [table]
        crops = ok = None
        ow = oh = 0
        if inset:
            ow, oh = inset
            crops, ok = rectify._crops_launch(crop_table, B, 3, dets.data_ptr() + 5 * 8, dc, K * dc, keep, K, ow, oh, images.device)
            rest += [crops, ok, crop_table]
        ids = None
        if tr is not None:
            dry = dry_outside_capture and not torch.cuda.is_current_stream_capturing()
            ids, slot, retired, tally = T._launch(tr, rows, first, dry)
            res.append(ids)
            rest += [slot, retired, tally]
        _draw_launch(table, 3, H, W, rows, None if ids is None else ids[0], crops, ok, ow, oh, style)
        return tuple(res + [out] + rest)
    return eager


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
    from . import rectify, track as T
    fn = 'annotate_batch'
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
    if inset is not None:
        DC._require_landmarks(fn, net, to='rectify for the inset')
        inset = rectify._crop_size(fn, inset)
    K = int(K)
    to_host = any(k != 'cuda' for k in kinds)
    x = DC._on_device(frames) if torch.is_tensor(frames) else rectify.to_device(frames, host)
    dry = DC._use_graph(net)

    def chunk(x, idx):
        first = int(stream0) + idx[0]
        key = ('topk', K, inset, st.key(), to_host)
        if tracker is not None:
            key += tracker._key(x.device, first)
        eager = _annotate_eager(K, inset, tracker, first, nms_thresh, st, dry)
        n_res = 4 if tracker is not None else 3
        n_rest = 1 + (3 if inset else 0) + (3 if tracker is not None else 0)
        flags = (True,) * (n_res - 1) + (to_host,) + (False,) * n_rest
        res = DC._run_chunk(net, 'annotate', x, (key, float(nms_thresh)), eager, flags)
        d, k = res[0].numpy(), res[1].numpy()
        ids = res[2].numpy() if tracker is not None else None
        # the results own their memory (a graph entry's buffers are overwritten by its next replay): the chunk's frames by ONE clone,
        # device to device for CUDA frames
        ann = res[n_res - 1].clone()
        out = []
        for b in range(d.shape[0]):
            keep = _keep_list(k[b])
            out.append((d[b].copy(), keep, None if ids is None else ids[0, b, :len(keep)].copy(), ann[b]))
        return out
    res = DC._detect_many(fn, x, max_batch, chunk, with_index=True)
    out = []
    for (d, keep, tid, ann), kind in zip(res, kinds):
        if kind == 'cuda' and not ann.is_cuda:
            ann = ann.cuda()                                         # (a CUDA frame in a list that also holds host frames)
        out.append((d, keep, tid, ann.numpy() if kind == 'numpy' else ann))
    return out
