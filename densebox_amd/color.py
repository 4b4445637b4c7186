"""NV12 frames in and out: what a hardware video decoder hands out and an encoder takes, converted to and from the interleaved uint8 RGB
every inference entry point reads -- ONE upload and ONE launch per call (dbx_nv12_to_rgb_batch, dbx_rgb_to_nv12_batch) -- and the
net-level calls on NV12 frames: detect_batch_nv12, detect_batch_resized_nv12 (the resize reads the surface itself,
dbx_resize_cubic_batch_nv12) and redact_batch_nv12 (NV12 in, redacted NV12 out).

No reference counterpart: the semantics are this project's own (include/densebox_hip.h has the contract -- 14-bit integer arithmetic,
chroma replicated over its 2 x 2 block, NO chroma interpolation -- and tests/nv12_ref.py restates it in NumPy).  The round trip
RGB -> NV12 -> RGB is NOT the identity: chroma is averaged over 2 x 2 blocks, limited range has fewer than 256 levels, both ways round.

THE FRAME CONVENTION of this module: an NV12 frame of h x w pixels (both even) is ONE uint8 [h * 3 / 2, pitch] array or tensor (numpy,
CPU or CUDA): h rows of Y, then h / 2 rows of interleaved U V, all of `pitch` bytes of which the first w count; width= gives w when
pitch > w.  A batch is a [B, h * 3 / 2, pitch] tensor or a list of frames of any sizes.  Surfaces with other plane layouts (separate
allocations, two pitches) are reachable through the C ABI's dbx_nv12_frame records."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, stream_ptr
from .decode import _integer

_ALIGN = 64
STANDARDS = (601, 709)
RANGES = {'limited': 0, 'full': 1}
ORDERS = {'rgb': 0, 'bgr': 1}
assert C.sizeof(_lib.Nv12Frame) == 48 and C.sizeof(_lib.Nv12Params) == 16 and C.sizeof(_lib.ResizeJobNv12) == 88


def _up(n, a=_ALIGN):
    return (n + a - 1) // a * a


class Params:
    """How NV12 and RGB relate.  standard: 601 or 709 (the luma weights Kr, Kb); range: 'limited' (Y 16..235, chroma 16..240) or 'full';
    order: 'rgb' or 'bgr', the byte order of the interleaved image (the engine's uint8 input is RGB)."""

    def __init__(self, standard=601, range='limited', order='rgb'):
        if not _integer(standard) or standard not in STANDARDS:
            raise RuntimeError('Params: standard=%r must be one of %s' % (standard, list(STANDARDS)))
        if range not in RANGES:
            raise RuntimeError('Params: range=%r must be one of %s' % (range, sorted(RANGES)))
        if order not in ORDERS:
            raise RuntimeError('Params: order=%r must be one of %s' % (order, sorted(ORDERS)))
        self.standard, self.range, self.order = int(standard), range, order

    def key(self):
        return (self.standard, self.range, self.order)

    def record(self):
        return _lib.Nv12Params(self.standard, RANGES[self.range], ORDERS[self.order], 0)


def _params(fn, params):
    if params is None:
        return Params()
    if not isinstance(params, Params):
        raise RuntimeError('%s: params must be a color.Params, got %s' % (fn, type(params).__name__))
    return params


# ------------------------------------------------------------------------------------------------------------ frames
class _Frame:
    """one checked NV12 frame: t, the contiguous uint8 [h * 3 / 2, pitch] tensor; kind, 'cuda', 'cpu' or 'numpy'"""

    def __init__(self, t, kind, w):
        self.t, self.kind = t.contiguous(), kind
        self.h, self.w, self.pitch = int(t.size(0)) // 3 * 2, w, int(t.size(1))


def _frames(fn, frames, width):
    """Checks a uint8 [B, h*3/2, pitch] tensor or a list of uint8 [h*3/2, pitch] frames (numpy or torch) without touching the device:
    the list of _Frame.  width: None (w = pitch), one integer, or one integer per frame."""
    if torch.is_tensor(frames):
        if frames.dtype != torch.uint8 or frames.dim() != 3:
            raise RuntimeError('%s: a tensor of NV12 frames must be uint8 [B, h*3/2, pitch], got %s %s' % (fn, frames.dtype, list(frames.shape)))
        ts, kinds = list(frames.unbind(0)), ['cuda' if frames.is_cuda else 'cpu'] * int(frames.size(0))
    elif isinstance(frames, (list, tuple)):
        ts, kinds = [], []
        for b, f in enumerate(frames):
            if isinstance(f, np.ndarray):
                kinds.append('numpy')
                f = torch.from_numpy(np.ascontiguousarray(f))
            elif torch.is_tensor(f):
                kinds.append('cuda' if f.is_cuda else 'cpu')
            else:
                raise RuntimeError('%s: frames[%d] must be a numpy array or a tensor, got %s' % (fn, b, type(f).__name__))
            if f.dtype != torch.uint8 or f.dim() != 2:
                raise RuntimeError('%s: frames[%d] must be uint8 [h*3/2, pitch], got %s %s' % (fn, b, f.dtype, list(f.shape)))
            ts.append(f)
    else:
        raise RuntimeError('%s: frames must be a uint8 tensor or a list of NV12 frames, got %s' % (fn, type(frames).__name__))
    if len(ts) == 0:
        raise RuntimeError('%s: no frames' % fn)
    if width is None or _integer(width):
        widths = [width] * len(ts)
    elif isinstance(width, (list, tuple)) and len(width) == len(ts) and all(_integer(w) for w in width):
        widths = list(width)
    else:
        raise RuntimeError('%s: width=%r must be None, an integer or one integer per frame' % (fn, width))
    out = []
    for b, (t, kind, w) in enumerate(zip(ts, kinds, widths)):
        rows, pitch = int(t.size(0)), int(t.size(1))
        w = pitch if w is None else int(w)
        if rows < 3 or rows % 3:
            raise RuntimeError('%s: frames[%d] has %d rows: an NV12 frame has h * 3 / 2 rows with h even' % (fn, b, rows))
        if w > pitch:
            raise RuntimeError('%s: width=%d of frames[%d] exceeds its pitch of %d bytes' % (fn, w, b, pitch))
        if w < 2 or w % 2:
            raise RuntimeError('%s: width=%d of frames[%d] must be even and positive' % (fn, w, b))
        out.append(_Frame(t, kind, w))
    return out


def _device_of(items):
    return next((t.device for t in items if t.is_cuda), torch.device('cuda', torch.cuda.current_device()))


class _Upload:
    """The ONE upload of a call: room for `table_bytes` at offset 0, then the host tensors of `items` (a CUDA tensor stays where it is),
    each 64-aligned.  base[i] is item i's device address once sent."""

    def __init__(self, items, table_bytes):
        at, self._off = _up(table_bytes), []
        for t in items:
            self._off.append(None if t.is_cuda else at)
            if not t.is_cuda:
                at = _up(at + t.numel())
        self.dev = _device_of(items)
        self.up = torch.empty(at, dtype=torch.uint8, device=self.dev)
        self.h = np.zeros(at, np.uint8)
        for t, o in zip(items, self._off):
            if o is not None:
                self.h[o:o + t.numel()] = t.numpy().reshape(-1)
        self.items = items                       # (keeps the CUDA tensors alive while their addresses are in use)
        self.base = [t.data_ptr() if o is None else self.up.data_ptr() + o for t, o in zip(items, self._off)]

    def send(self, table=None):
        if table is not None:
            raw = np.frombuffer(table, np.uint8)
            self.h[:raw.size] = raw
        self.up.copy_(torch.from_numpy(self.h))


def _offsets(sizes):
    """(byte offsets, total) of blocks of `sizes` bytes in an arena: back to back when all are equal (the arena IS the stacked batch: the
    kernels take any alignment), else each 64-aligned"""
    if len(set(sizes)) == 1:
        return [i * sizes[0] for i in range(len(sizes))], len(sizes) * sizes[0]
    offs, at = [], 0
    for n in sizes:
        offs.append(at)
        at = _up(at + n)
    return offs, at


def _to_rgb(fn, fr, params):
    """ONE upload and ONE dbx_nv12_to_rgb_batch launch over the checked frames fr: (arena, offsets) of the uint8 [h, w, 3] results"""
    B = len(fr)
    up = _Upload([f.t for f in fr], B * 48)
    offs, total = _offsets([f.h * f.w * 3 for f in fr])
    arena = torch.empty(total, dtype=torch.uint8, device=up.dev)
    rec = (_lib.Nv12Frame * B)()
    for r, f, base, d in zip(rec, fr, up.base, offs):
        r.y, r.uv, r.rgb = base, base + f.h * f.pitch, arena.data_ptr() + d
        r.h, r.w, r.pitch_y, r.pitch_uv, r.pitch_rgb = f.h, f.w, f.pitch, f.pitch, 3 * f.w
    up.send(rec)
    check(_lib.lib().dbx_nv12_to_rgb_batch(C.c_void_p(up.up.data_ptr()), B, max(f.h for f in fr), max(f.w for f in fr),
                                           C.byref(params.record()), stream_ptr()))
    return arena, offs


def _from_rgb(fn, images, params):
    """ONE upload and ONE dbx_rgb_to_nv12_batch launch over contiguous uint8 [h, w, 3] tensors: (arena, offsets) of the uint8
    [h * 3 / 2, w] frames"""
    B = len(images)
    for b, im in enumerate(images):
        if int(im.size(0)) % 2 or int(im.size(1)) % 2:
            raise RuntimeError('%s: images[%d] is %d x %d pixels: NV12 needs an even height and width' % (fn, b, im.size(1), im.size(0)))
    up = _Upload(images, B * 48)
    offs, total = _offsets([im.numel() // 2 for im in images])
    arena = torch.empty(total, dtype=torch.uint8, device=up.dev)
    rec = (_lib.Nv12Frame * B)()
    for r, im, base, d in zip(rec, images, up.base, offs):
        h, w = int(im.size(0)), int(im.size(1))
        r.y, r.uv, r.rgb = arena.data_ptr() + d, arena.data_ptr() + d + h * w, base
        r.h, r.w, r.pitch_y, r.pitch_uv, r.pitch_rgb = h, w, w, w, 3 * w
    up.send(rec)
    check(_lib.lib().dbx_rgb_to_nv12_batch(C.c_void_p(up.up.data_ptr()), B, max(int(im.size(0)) for im in images),
                                           max(int(im.size(1)) for im in images), C.byref(params.record()), stream_ptr()))
    return arena, offs


def _in_kind(arena, offs, shapes, kinds):
    """the blocks of a device arena as tensors of `shapes`, each of its kind: one copy back when a kind is of the host"""
    down = arena.cpu() if any(k != 'cuda' for k in kinds) else None
    out = []
    for o, shape, kind in zip(offs, shapes, kinds):
        v = (arena if kind == 'cuda' else down)[o:o + int(np.prod(shape))].view(*shape)
        out.append(v.numpy() if kind == 'numpy' else v)
    return out


# ------------------------------------------------------------------------------------------------------------ the conversions
def nv12_to_rgb_batch(frames, width=None, params=None):
    """NV12 frames to interleaved RGB with ONE upload and ONE dbx_nv12_to_rgb_batch launch.

    frames: the module's frame convention -- a uint8 [B, h*3/2, pitch] tensor or a list of uint8 [h*3/2, pitch] frames of any sizes (numpy
    arrays or tensors, on the CPU or the GPU; a CUDA frame is read where it is).  width: w when pitch > w (one integer or one per
    frame).  params: a color.Params (default 601, limited, rgb).

    Returns uint8 [h, w, 3] CUDA tensors, views of one arena: one [B, h, w, 3] tensor for a batch tensor, a list for a list."""
    fn = 'nv12_to_rgb_batch'
    p = _params(fn, params)
    fr = _frames(fn, frames, width)
    arena, offs = _to_rgb(fn, fr, p)
    if torch.is_tensor(frames):
        return arena.view(len(fr), fr[0].h, fr[0].w, 3)
    return [arena[o:o + f.h * f.w * 3].view(f.h, f.w, 3) for f, o in zip(fr, offs)]


def rgb_to_nv12_batch(images, params=None):
    """The inverse, with ONE upload, ONE dbx_rgb_to_nv12_batch launch and one copy back: images a uint8 [B,H,W,3] tensor or a list of
    uint8 [H,W,3] images of any even sizes (numpy arrays or tensors, on the CPU or the GPU).  Returns the uint8 [H * 3 / 2, W] frames
    (pitch = W), each of the kind of its input (CUDA results are views of one arena): one [B, H*3/2, W] tensor for a batch tensor, a
    list for a list."""
    from . import rectify
    fn = 'rgb_to_nv12_batch'
    p = _params(fn, params)
    host, kinds = rectify.host_images(fn, images, 3)
    ims = [im.contiguous() for im in host]
    arena, offs = _from_rgb(fn, ims, p)
    shapes = [(int(im.size(0)) * 3 // 2, int(im.size(1))) for im in ims]
    if torch.is_tensor(images):
        v = arena.view(len(ims), *shapes[0])
        return v if images.is_cuda else v.cpu()
    return _in_kind(arena, offs, shapes, kinds)


# ------------------------------------------------------------------------------------------------------------ the net-level calls
def _one_size(fn, fr):
    sizes = sorted({(f.h, f.w) for f in fr})
    if len(sizes) > 1:
        raise RuntimeError('%s: the frames must have one size, got %s (detect_batch_resized_nv12 takes mixed sizes)' % (fn, sizes))
    return sizes[0]


def detect_batch_nv12(net, frames, width=None, params=None, K=10, nms_thresh=0.4, max_batch=32):
    """detect_batch on NV12 frames of ONE size: the dbx_nv12_to_rgb_batch launch (not captured: its table depends on the call, like the
    resize launch of detect_batch_resized), then detect_batch's tensor path on the uint8 [B,h,w,3] result, which never leaves the device.
    frames, width, params: as for nv12_to_rgb_batch.  Returns detect_batch's list of (dets, keep)."""
    from . import decode
    fn = 'detect_batch_nv12'
    p = _params(fn, params)
    fr = _frames(fn, frames, width)
    h, w = _one_size(fn, fr)
    arena, _ = _to_rgb(fn, fr, p)
    return decode.detect_batch(net, arena.view(len(fr), h, w, 3), K, nms_thresh, max_batch)


def detect_batch_resized_nv12(net, frames, size=720, width=None, params=None, K=10, nms_thresh=0.4, max_batch=32, score_thresh=None,
                              max_dets=1024):
    """detect_batch_resized on NV12 frames of ANY sizes: pad_img + the bicubic resize to size x size read the NV12 surface itself in ONE
    dbx_resize_cubic_batch_nv12 launch -- half the source bytes of the RGB path, and the full-resolution RGB frame is never written --
    then detect_batch / detect_batch_thresh on the uint8 [B, size, size, 3] tensor.  The resized frames are bit for bit those of
    detect_batch_resized on nv12_to_rgb_batch's frames, and the rows are mapped back to the source frames exactly as there."""
    from . import decode, resize
    fn = 'detect_batch_resized_nv12'
    tc = decode._thresh_or_topk(fn, K, score_thresh, max_dets)
    if not _integer(size) or size < 4 or size % 4:
        raise RuntimeError('%s: size=%r must be a positive multiple of 4 (the maps are size / 4)' % (fn, size))
    p = _params(fn, params)
    fr = _frames(fn, frames, width)
    x = resize._pad_resize_nv12_device(fr, int(size), p)
    res = decode.detect_batch(net, x, K, nms_thresh, max_batch) if tc is None else decode.detect_batch_thresh(net, x, tc[0], tc[1],
                                                                                                             nms_thresh, max_batch)
    return decode._map_back([(f.h, f.w) for f in fr], res, int(size))


def redact_batch_nv12(net, frames, *, width=None, tracker=None, stream0=0, K=10, nms_thresh=0.4, max_batch=32, style=None, params=None):
    """net.redact_batch with NV12 on both sides: the frames (ONE size; frame j is the next frame of camera stream stream0 + j) are
    converted on the device, redact_batch runs on the device RGB frames as it always does, and the redacted frames are converted back
    by ONE dbx_rgb_to_nv12_batch launch.  Returns, per frame in input order, (dets, keep, track_id or None, nv12): dets, keep and
    track_id are redact_batch's on the converted frames; nv12 is the redacted uint8 [h * 3 / 2, w] frame (pitch = w) of the kind of the
    input frame.  The luma and chroma of pixels no region covers are NOT the input's bytes: they made the round trip."""
    from . import redact
    fn = 'redact_batch_nv12'
    p = _params(fn, params)
    fr = _frames(fn, frames, width)
    h, w = _one_size(fn, fr)
    arena, _ = _to_rgb(fn, fr, p)
    res = redact.net_redact_batch(net, arena.view(len(fr), h, w, 3), tracker=tracker, stream0=stream0, K=K, nms_thresh=nms_thresh,
                                  max_batch=max_batch, style=style)
    out_arena, offs = _from_rgb(fn, [r[3].contiguous() for r in res], p)
    nv = _in_kind(out_arena, offs, [(h * 3 // 2, w)] * len(fr), [f.kind for f in fr])
    return [(d, keep, tid, f) for (d, keep, tid, _), f in zip(res, nv)]
