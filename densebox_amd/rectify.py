"""Plate rectification after decode: ``perspective_transform`` (DenseBox.py:3446-3481, called from ``viz_result``
:3546-3553) on the GPU -- same name, arguments and result (uint8 image of 1.5x the input size) as the reference, which
delegates to cv2.getPerspectiveTransform / cv2.warpPerspective.  OpenCV is not part of the reference tree: the kernels
follow its published algorithm (see csrc/post_ops.hip); parity with OpenCV itself is unpinned."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, stream_ptr


def dst_rectangle(src_pts):
    """The four destination corners the reference builds (:3462-3474): the axis-aligned rectangle spanned by the
    left/right/top/bottom extremes of (left-up, right-up, right-down, left-down)."""
    assert len(src_pts) == 4
    lu, ru, rd, ld = src_pts
    min_x, max_x = min(lu[0], ld[0]), max(ru[0], rd[0])
    min_y, max_y = min(lu[1], ru[1]), max(ld[1], rd[1])
    return [[min_x, min_y], [max_x, min_y], [max_x, max_y], [min_x, max_y]]


def get_perspective_matrix(src_pts, dst_pts):
    src = np.ascontiguousarray(np.float32(src_pts).reshape(8))
    dst = np.ascontiguousarray(np.float32(dst_pts).reshape(8))
    m = np.empty(9, dtype=np.float64)
    check(_lib.lib().dbx_perspective_matrix(src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p),
                                            m.ctypes.data_as(C.c_void_p)))
    return m.reshape(3, 3)


def warp_perspective(img, M, dsize):
    """img: uint8 [H, W, C] (numpy or a CUDA tensor); dsize = (width, height) like cv2.  Returns the same kind."""
    was_np = isinstance(img, np.ndarray)
    t = torch.as_tensor(img).cuda().contiguous()
    assert t.dtype == torch.uint8 and t.dim() == 3
    h, w, c = t.shape
    dw, dh = int(dsize[0]), int(dsize[1])
    out = torch.empty((dh, dw, c), dtype=torch.uint8, device=t.device)
    m = np.ascontiguousarray(np.asarray(M, dtype=np.float64).reshape(9))
    check(_lib.lib().dbx_warp_perspective_u8(C.c_void_p(t.data_ptr()), h, w, c, m.ctypes.data_as(C.c_void_p),
                                             C.c_void_p(out.data_ptr()), dh, dw, stream_ptr()))
    return out.cpu().numpy() if was_np else out


def perspective_transform(img, src_pts):
    """DenseBox.py:3446: warp so that the four plate corners land on their bounding rectangle; output is
    (int(W*1.5+0.5), int(H*1.5+0.5)) like the reference."""
    M = get_perspective_matrix(src_pts, dst_rectangle(src_pts))
    h, w = img.shape[0], img.shape[1]
    return warp_perspective(img, M, (int(w * 1.5 + 0.5), int(h * 1.5 + 0.5)))


_REGIONS = ('canvas', 'plate')
_ALIGN = 64                    # byte alignment of every job's output in the arena (the kernel stores 16-byte words when aligned)


def check_region(who, region):
    if region not in _REGIONS:
        raise RuntimeError("%s: region must be 'canvas' or 'plate', got %r" % (who, region))


def canvas_size(h, w):
    """(dh, dw) of the reference's 1.5x canvas for an h x w image."""
    return int(h * 1.5 + 0.5), int(w * 1.5 + 0.5)


def plate_window(dst_pts, dh, dw):
    """(x0, y0, oh, ow) of the destination rectangle's pixels inside a dh x dw canvas, or None when empty: x0 = max(0, floor(min_x)),
    x1 = min(dw-1, ceil(max_x)) inclusive, the same for y, over the float32 corner values the matrix is solved with."""
    d = np.float32(dst_pts).reshape(4, 2).tolist()           # (float32 values as Python floats: exact)
    xs, ys = [p[0] for p in d], [p[1] for p in d]
    x0, x1 = max(0, math.floor(min(xs))), min(dw - 1, math.ceil(max(xs)))
    y0, y1 = max(0, math.floor(min(ys))), min(dh - 1, math.ceil(max(ys)))
    if x1 < x0 or y1 < y0:
        return None
    return x0, y0, y1 - y0 + 1, x1 - x0 + 1


def _invertible(m):
    """The test dbx_warp_perspective_batch_u8 applies to every map before it launches (warp_inverse and the finiteness check in
    csrc/post_ops.hip; keep the two in step): every entry finite and the cofactor determinant, in the same operation order, non-zero.
    A map that passes here is never refused there, so one bad quad gives None instead of failing the whole call."""
    m = np.asarray(m, dtype=np.float64).reshape(9).tolist()
    if not all(math.isfinite(v) for v in m):
        return False
    det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])
    return det != 0.0


def _rect_job(quad, h, w, region):
    """(m9, dh, dw, x0, y0, oh, ow) of one quad on an h x w image, or None (degenerate corners, a non-finite coordinate, an empty
    plate window)."""
    try:
        q = np.asarray(quad, dtype=np.float64).reshape(4, 2)
    except (TypeError, ValueError):
        raise RuntimeError('perspective_transform_batch: a quad must be 4 (x, y) points, got %r' % (quad,))
    if not np.all(np.isfinite(np.float32(q))):
        return None
    q = q.tolist()
    dst = dst_rectangle(q)
    try:
        M = get_perspective_matrix(q, dst)
    except RuntimeError:                                       # dbx_perspective_matrix: degenerate corner configuration
        return None
    if not _invertible(M):
        return None
    dh, dw = canvas_size(h, w)
    if region == 'canvas':
        return M, dh, dw, 0, 0, dh, dw
    win = plate_window(dst, dh, dw)
    return None if win is None else (M, dh, dw) + win


def perspective_transform_batch(images, quads, *, region):
    """perspective_transform over many images and many quads per image in ONE kernel launch (dbx_warp_perspective_batch_u8).

    images: a uint8 [B,H,W,C] tensor, or a list of uint8 [H,W,C] images of any sizes (numpy arrays or tensors, on the CPU or the
    GPU); C is 1..4 and the same for all.  Each image is copied to the device at most once.  quads[b]: the list of 4-point quads
    (left-up, right-up, right-down, left-down) of image b.  region: 'canvas' -- the whole 1.5x canvas perspective_transform returns
    -- or 'plate' -- its window over the destination rectangle (plate_window).  Every matrix comes from get_perspective_matrix on the
    host.

    Returns out[b][j]: uint8 [oh, ow, C] of the kind of image b (CUDA tensors are views into one device arena; numpy arrays and CPU
    tensors come from one download of it), or None when the corners are degenerate, a coordinate is not finite or the plate window
    is empty.  The pixels are bit for bit those of perspective_transform."""
    check_region('perspective_transform_batch', region)
    host, kinds = host_images('perspective_transform_batch', images, None)
    if len(quads) != len(host):
        raise RuntimeError('perspective_transform_batch: %d lists of quads for %d images' % (len(quads), len(host)))
    return _warp_batch(to_device(images, host), kinds, quads, region)


def host_images(who, images, channels):
    """Checks a uint8 [B,H,W,C] tensor or a list of uint8 [H,W,C] images (numpy or torch) without touching the device: the list
    of per-image tensors (torch views of numpy arrays) and the kind -- 'cuda', 'cpu' or 'numpy' -- of each.  channels: the one
    channel count allowed, or None for 1..4."""
    want = '3' if channels == 3 else 'C'
    if torch.is_tensor(images):
        if images.dtype != torch.uint8 or images.dim() != 4:
            raise RuntimeError('%s: a tensor of images must be uint8 [B,H,W,%s], got %s %s' % (who, want, images.dtype, list(images.shape)))
        ims = list(images.unbind(0))
        kinds = ['cuda' if images.is_cuda else 'cpu'] * len(ims)
    elif isinstance(images, (list, tuple)):
        ims, kinds = [], []
        for b, im in enumerate(images):
            if isinstance(im, np.ndarray):
                kinds.append('numpy')
                im = torch.from_numpy(np.ascontiguousarray(im))
            elif torch.is_tensor(im):
                kinds.append('cuda' if im.is_cuda else 'cpu')
            else:
                raise RuntimeError('%s: images[%d] must be a numpy array or a tensor, got %s' % (who, b, type(im).__name__))
            if im.dtype != torch.uint8 or im.dim() != 3:
                raise RuntimeError('%s: images[%d] must be uint8 [H,W,%s], got %s %s' % (who, b, want, im.dtype, list(im.shape)))
            ims.append(im)
    else:
        raise RuntimeError('%s: images must be a uint8 tensor or a list of images, got %s' % (who, type(images).__name__))
    chans = sorted({int(im.size(2)) for im in ims})
    if len(chans) > 1 or not set(chans) <= ({channels} if channels else {1, 2, 3, 4}):
        raise RuntimeError('%s: every image needs %s channels, got %s' % (who, channels or 'the same count of 1..4', chans))
    if len(ims) == 0:
        raise RuntimeError('%s: no images' % who)
    return ims, kinds


def to_device(images, host):
    """Device copies of host_images' list, each image uploaded at most once (a batch tensor in one copy)."""
    if torch.is_tensor(images):
        return list((images if images.is_cuda else images.cuda()).contiguous().unbind(0))
    return [(im if im.is_cuda else im.cuda()).contiguous() for im in host]


def _warp_batch(dev, kinds, quads, region):
    """perspective_transform_batch on images already on the device: dev[b] a contiguous uint8 [H,W,C] CUDA tensor, kinds[b] the kind
    ('cuda', 'cpu' or 'numpy') image b's results are returned as."""
    c = int(dev[0].size(2))
    out = [[None] * len(qs) for qs in quads]
    spec, total = [], 0
    for b, qs in enumerate(quads):
        h, w = int(dev[b].size(0)), int(dev[b].size(1))
        for j, q in enumerate(qs):
            job = _rect_job(q, h, w, region)
            if job is None:
                continue
            spec.append((b, j, total) + job)
            total += (job[5] * job[6] * c + _ALIGN - 1) // _ALIGN * _ALIGN
    if not spec:
        return out
    device = dev[0].device
    arena = torch.empty(total, dtype=torch.uint8, device=device)
    jobs = (_lib.WarpJob * len(spec))()
    for r, (b, j, off, M, dh, dw, x0, y0, oh, ow) in zip(jobs, spec):
        r.src = dev[b].data_ptr()
        r.sh, r.sw = int(dev[b].size(0)), int(dev[b].size(1))
        r.m9[:] = [float(v) for v in np.asarray(M, dtype=np.float64).reshape(9)]
        r.dh, r.dw, r.x0, r.y0, r.oh, r.ow, r.dst_off = dh, dw, x0, y0, oh, ow, off
    L = _lib.lib()
    ws = torch.empty(L.dbx_warp_batch_workspace_bytes(len(spec)), dtype=torch.uint8, device=device)
    check(L.dbx_warp_perspective_batch_u8(jobs, len(spec), c, C.c_void_p(arena.data_ptr()), C.c_void_p(ws.data_ptr()),
                                          stream_ptr()))
    host = arena.cpu() if any(kinds[b] != 'cuda' for b, *_ in spec) else None
    for (b, j, off, M, dh, dw, x0, y0, oh, ow) in spec:
        src = arena if kinds[b] == 'cuda' else host
        v = src[off:off + oh * ow * c].view(oh, ow, c)
        out[b][j] = v.numpy() if kinds[b] == 'numpy' else v
    return out


# ---------------------------------------------------------------------------------------------- fixed-size plate crops
def _crop_size(who, size):
    """(ow, oh) of a crop size given as an integer or (width, height): resize._check_size's rules, and a sequence holds exactly two."""
    from .resize import _check_size
    if not isinstance(size, (int, np.integer)) or isinstance(size, (bool, np.bool_)):
        try:
            n = len(size)
        except TypeError:
            n = -1
        if n != 2:
            raise RuntimeError('%s: size must be an integer or (width, height), got %r' % (who, size))
    return _check_size(who, size)


def plate_rectangle(size):
    """The four destination corners of a crop of size = (width, height): (0,0), (w-1,0), (w-1,h-1), (0,h-1) -- the corners of the quad
    land on the centres of the first and last pixel, as dst_rectangle's do on the canvas."""
    w, h = _crop_size('plate_rectangle', size)
    return [[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]]


def frame_records(dev):
    """The ctypes array of dbx_crop_frame records {src, sh, sw} of contiguous uint8 [H,W,C] CUDA tensors.  It holds raw addresses: keep
    `dev` alive while the records are in use."""
    rec = (_lib.CropFrame * len(dev))()
    for r, im in zip(rec, dev):
        r.src, r.sh, r.sw = im.data_ptr(), int(im.size(0)), int(im.size(1))
    return rec


def frame_table(dev):
    """frame_records(dev) as a device table (one small upload)"""
    return torch.frombuffer(frame_records(dev), dtype=torch.uint8).to(dev[0].device)


def _crops_launch(table, nframes, c, quads_ptr, row_stride, frame_stride, sel, slots, ow, oh, device, with_m9=False):
    """ONE dbx_plate_crops_batch launch on the current stream: (crops uint8 [nframes, slots, oh, ow, c], ok int32 [nframes, slots][, m9
    float64 [nframes, slots, 9]]) device tensors.  Nothing is copied from the host and nothing waits, so a graph capture may hold it."""
    crops = torch.empty((nframes, slots, oh, ow, c), dtype=torch.uint8, device=device)
    ok = torch.empty((nframes, slots), dtype=torch.int32, device=device)
    m9 = torch.empty((nframes, slots, 9), dtype=torch.float64, device=device) if with_m9 else None
    check(_lib.lib().dbx_plate_crops_batch(C.c_void_p(table.data_ptr()), nframes, c, C.c_void_p(quads_ptr), row_stride, frame_stride,
                                           _lib.ptr(sel), slots, ow, oh, C.c_void_p(crops.data_ptr()), C.c_void_p(ok.data_ptr()),
                                           _lib.ptr(m9), stream_ptr()))
    return (crops, ok, m9) if with_m9 else (crops, ok)


def _quad_rows(who, b, qs):
    """quads[b] as a float64 [Q_b, 8] array: a list of 4-point quads, or a [Q_b, 8] / [Q_b, 4, 2] array or tensor."""
    if torch.is_tensor(qs):
        qs = qs.detach().cpu().numpy()
    try:
        a = np.asarray(qs, dtype=np.float64)
    except (TypeError, ValueError):
        raise RuntimeError('%s: quads[%d] must hold quads of 8 numbers (4 (x, y) points), got %r' % (who, b, qs))
    if a.size == 0 and a.ndim <= 1:
        return np.zeros((0, 8), dtype=np.float64)
    if not ((a.ndim == 2 and a.shape[1] == 8) or (a.ndim == 3 and a.shape[1:] == (4, 2))):
        raise RuntimeError('%s: quads[%d] must hold quads of 8 numbers (4 (x, y) points), got shape %s' % (who, b, list(a.shape)))
    return np.ascontiguousarray(a.reshape(a.shape[0], 8))


def plate_crops_batch(images, quads, *, size):
    """Every quad of every image rectified to ONE crop size in ONE launch (dbx_plate_crops_batch): the input a plate recogniser takes.

    images: as for perspective_transform_batch (a uint8 [B,H,W,C] tensor or a list of uint8 [H,W,C] images of any sizes, numpy or
    torch, CPU or GPU; C is 1..4 and the same for all); each image is uploaded at most once.  quads[b]: the quads (left-up, right-up,
    right-down, left-down) of image b -- a list of 4-point quads, or a float [Q_b, 8] or [Q_b, 4, 2] array or tensor.  size: (width,
    height) of a crop, or one integer for both.  The quads travel to the device padded to the largest Q_b, with a count per image,
    next to the frame table; the homographies are solved there (dbx_perspective_matrix's solve, compiled for the device) onto
    plate_rectangle(size).

    Returns per image (crops, ok): crops uint8 [Q_b, oh, ow, C] of the image's kind (CUDA tensors are views into one device arena;
    numpy arrays and CPU tensors come from one download of it), ok a numpy bool [Q_b].  Crop j is bit for bit
    warp_perspective(image, get_perspective_matrix(quad, plate_rectangle(size)), size) where ok[j]; it is all zeros where not:
    degenerate corners, a coordinate that is not finite in float32, a singular map -- the cases perspective_transform_batch gives
    None for."""
    who = 'plate_crops_batch'
    ow, oh = _crop_size(who, size)
    host, kinds = host_images(who, images, None)
    if len(quads) != len(host):
        raise RuntimeError('%s: %d lists of quads for %d images' % (who, len(quads), len(host)))
    rows = [_quad_rows(who, b, qs) for b, qs in enumerate(quads)]
    B, c, slots = len(host), int(host[0].size(2)), max(len(r) for r in rows)
    if slots == 0:
        ok = torch.zeros((B, 0), dtype=torch.int32)
        crops = [torch.zeros((0, oh, ow, c), dtype=torch.uint8) for _ in range(B)]
        crops = [cr.cuda() if k == 'cuda' else cr for cr, k in zip(crops, kinds)]
    else:
        packed = np.zeros((B, slots, 8), dtype=np.float64)
        sel = np.zeros((B, slots + 1), dtype=np.int32)
        for b, r in enumerate(rows):
            packed[b, :len(r)] = r
            sel[b, 0] = len(r)
            sel[b, 1:1 + len(r)] = np.arange(len(r))
        dev = to_device(images, host)
        device = dev[0].device
        d_quads, d_sel = torch.from_numpy(packed).to(device), torch.from_numpy(sel).to(device)
        table = frame_table(dev)
        arena, ok = _crops_launch(table, B, c, d_quads.data_ptr(), 8, slots * 8, d_sel, slots, ow, oh, device)
        down = arena.cpu() if any(k != 'cuda' for k in kinds) else None
        crops = [(arena if k == 'cuda' else down)[b, :len(rows[b])] for b, k in enumerate(kinds)]
        ok = ok.cpu()                                          # (behind the launch on the stream: dev and table are done with)
    ok = ok.numpy() != 0
    return [(cr.numpy() if k == 'numpy' else cr, ok[b, :len(rows[b])].copy()) for b, (cr, k) in enumerate(zip(crops, kinds))]
