"""Pad + bicubic resize on the GPU: ``pad_img`` followed by ``cv2.resize(img, (size, size), interpolation=cv2.INTER_CUBIC)``
(``batch_pad_resize``, DenseBox.py:1282-1340) and the patch cutters' ``cv2.resize`` of a cropped window
(process_plate.py:244-252), over many images in ONE kernel launch (dbx_resize_cubic_batch_u8).  OpenCV is not part of the
reference tree: the kernel restates the generic C path of its 8-bit INTER_CUBIC (see csrc/resize_ops.hip); parity with an
OpenCV build is unpinned, and OpenCV's own SIMD builds may differ from that path in the last bit."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, stream_ptr
from .rectify import host_images, to_device

PAD_VALUE = 128


def pad_geometry(h, w):
    """(side, pad_x, pad_y) of pad_img on an h x w image: the side of the square, and the columns / rows added on the left / top
    (the right / bottom gets the extra pixel of an odd difference)."""
    h, w = int(h), int(w)
    lu = abs(h - w) // 2
    return max(h, w), (lu if h > w else 0), (lu if h <= w else 0)


def pad_img(img):
    """DenseBox.py:1282: pads the short side of a numpy [H,W] or [H,W,3] image to a square with grey 128."""
    if not isinstance(img, np.ndarray):
        raise RuntimeError('pad_img: the image must be a numpy array, got %s' % type(img).__name__)
    if not (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3)):
        raise RuntimeError('pad_img: the image must be [H,W] or [H,W,3], got %s' % list(img.shape))
    h, w = img.shape[:2]
    side, px, py = pad_geometry(h, w)
    padding = ((py, side - h - py), (px, side - w - px)) + ((0, 0),) * (img.ndim - 2)
    return np.pad(img, padding, 'constant', constant_values=PAD_VALUE)


def _launch_jobs(dev, spec, offs, c, arena):
    """ONE dbx_resize_cubic_batch_u8 launch over spec = [(b, cx0, cy0, cw, ch, pad_l, pad_t, pad_r, pad_b, dh, dw)], job i writing its
    [dh, dw, c] block at byte offs[i] of the uint8 CUDA tensor `arena`.  dev[b]: contiguous uint8 [H,W,c] CUDA tensors."""
    jobs = (_lib.ResizeJob * len(spec))()
    for r, (b, cx0, cy0, cw, ch, pl, pt, pr, pb, jh, jw), off in zip(jobs, spec, offs):
        r.src = dev[b].data_ptr()
        r.sh, r.sw = int(dev[b].size(0)), int(dev[b].size(1))
        r.cx0, r.cy0, r.cw, r.ch = cx0, cy0, cw, ch
        r.pad_l, r.pad_t, r.pad_r, r.pad_b, r.pad_value = pl, pt, pr, pb, PAD_VALUE
        r.dh, r.dw, r.dst_off = jh, jw, off
    L = _lib.lib()
    ws = torch.empty(L.dbx_resize_batch_workspace_bytes(len(spec)), dtype=torch.uint8, device=arena.device)
    check(L.dbx_resize_cubic_batch_u8(jobs, len(spec), c, C.c_void_p(arena.data_ptr()), C.c_void_p(ws.data_ptr()), stream_ptr()))


def _resize_jobs(dev, spec, c):
    """ONE launch over spec = [(b, cx0, cy0, cw, ch, pad_l, pad_t, pad_r, pad_b, dh, dw)], all with the same dh x dw: the uint8
    [len(spec), dh, dw, c] CUDA tensor of the jobs' results in order.  dev[b]: contiguous uint8 [H,W,c] CUDA tensors."""
    dh, dw = spec[0][9], spec[0][10]
    block = dh * dw * c            # the jobs' blocks back to back ARE the result: the kernel stores aligned words at any offset
    out = torch.empty((len(spec), dh, dw, c), dtype=torch.uint8, device=dev[0].device)
    _launch_jobs(dev, spec, [i * block for i in range(len(spec))], c, out)
    return out


def _check_size(who, size):
    try:
        w, h = (size, size) if isinstance(size, (int, np.integer)) else (int(size[0]), int(size[1]))
    except (TypeError, ValueError, IndexError):
        raise RuntimeError('%s: size must be an integer or (width, height), got %r' % (who, size))
    if w < 1 or h < 1:
        raise RuntimeError('%s: size=%r must be positive' % (who, size))
    return int(w), int(h)


def _pad_spec(dev, size):
    """pad_img + resize to size x size of every image of dev, as _resize_jobs' job tuples."""
    spec = []
    for b, im in enumerate(dev):
        h, w = int(im.size(0)), int(im.size(1))
        side, px, py = pad_geometry(h, w)
        spec.append((b, 0, 0, w, h, px, py, side - w - px, side - h - py, size, size))
    return spec


def _pad_resize_device(dev, size):
    """pad_resize_batch on images already on the device."""
    return _resize_jobs(dev, _pad_spec(dev, size), int(dev[0].size(2)))


def _pad_resize_levels(dev, sizes):
    """_pad_resize_device at every size of `sizes` in ONE launch of len(dev) * len(sizes) jobs: a list with one uint8
    [B, size, size, C] CUDA tensor per size.  The tensors are views of one arena -- a level's jobs write back to back, so its block of
    the arena IS that tensor -- and every job is the one _pad_resize_device builds for that size."""
    c = int(dev[0].size(2))
    spec, offs, starts, pos = [], [], [], 0
    for size in sizes:
        starts.append(pos)
        for job in _pad_spec(dev, int(size)):
            spec.append(job)
            offs.append(pos)
            pos += int(size) * int(size) * c
    arena = torch.empty(pos, dtype=torch.uint8, device=dev[0].device)
    _launch_jobs(dev, spec, offs, c, arena)
    B = len(dev)
    return [arena[st:st + B * int(sz) * int(sz) * c].view(B, int(sz), int(sz), c) for st, sz in zip(starts, sizes)]


def level_xform(h, w, size):
    """(scale, off_x, off_y) that maps coordinates in the size x size resize of pad_img of an h x w frame back to the frame:
    x_src = x * scale - off_x, y_src = y * scale - off_y, with scale = side / size and the offsets pad_geometry's padding."""
    side, pad_x, pad_y = pad_geometry(h, w)
    return side / int(size), float(pad_x), float(pad_y)


def pad_resize_batch(images, size=720):
    """batch_pad_resize's pixel work (DenseBox.py:1317-1340) in ONE kernel launch: per image, cv2.resize(pad_img(im), (size, size),
    interpolation=cv2.INTER_CUBIC).  The padded square is never materialised.

    images: a uint8 [B,H,W,C] tensor, or a list of uint8 [H,W,C] images of any sizes (numpy arrays or tensors, on the CPU or the
    GPU); C is 1..4 and the same for all.  Each image is copied to the device at most once.  Returns a uint8 [B, size, size, C]
    CUDA tensor."""
    if not isinstance(size, (int, np.integer)) or size < 1:
        raise RuntimeError('pad_resize_batch: size must be a positive integer (the side of the square), got %r' % (size,))
    host, _ = host_images('pad_resize_batch', images, None)
    return _pad_resize_device(to_device(images, host), int(size))


def crop_resize_batch(images, windows, size=(240, 240)):
    """The pixel half of the reference's patch cutters in ONE kernel launch: per image b and window (x0, y0, x1, y1) of windows[b],
    cv2.resize(img[y0:y1, x0:x1], size, interpolation=cv2.INTER_CUBIC).  Windows are integers with Python-slice semantics
    (negative values count from the end and both ends are clamped to the image, as a numpy slice does); an empty slice is refused.

    images: as for pad_resize_batch.  size: (width, height) as in cv2.  Returns a uint8 [P, height, width, C] CUDA tensor in
    image-then-window order."""
    dw, dh = _check_size('crop_resize_batch', size)
    host, _ = host_images('crop_resize_batch', images, None)
    spec = _window_spec('crop_resize_batch', [(int(im.size(0)), int(im.size(1))) for im in host], windows, dh, dw)
    return _resize_jobs(to_device(images, host), spec, int(host[0].size(2)))


def _window_spec(fn, hw, windows, dh, dw):
    """the job tuples of windows[b] on image b of hw[b] = (h, w) pixels, each resized to dh x dw"""
    if not isinstance(windows, (list, tuple)) or len(windows) != len(hw):
        raise RuntimeError('%s: %s lists of windows for %d images' % (fn, len(windows) if isinstance(windows, (list, tuple)) else 'no', len(hw)))
    spec = []
    for b, ((h, w), wins) in enumerate(zip(hw, windows)):
        for win in wins:
            try:
                x0, y0, x1, y1 = (int(v) for v in win)
                if any(int(v) != v for v in win):
                    raise ValueError
            except (TypeError, ValueError):
                raise RuntimeError('%s: a window must be 4 integers (x0, y0, x1, y1), got %r for image %d' % (fn, win, b))
            xa, xb, _ = slice(x0, x1).indices(w)
            ya, yb, _ = slice(y0, y1).indices(h)
            if xb <= xa or yb <= ya:
                raise RuntimeError('%s: window %r of image %d (%d x %d) is an empty slice' % (fn, tuple(win), b, h, w))
            spec.append((b, xa, ya, xb - xa, yb - ya, 0, 0, 0, 0, dh, dw))
    if not spec:
        raise RuntimeError('%s: no windows' % fn)
    return spec


# ------------------------------------------------------------------------------------------------------------ NV12 sources
def _resize_jobs_nv12(fr, spec, params):
    """_resize_jobs on NV12 surfaces: ONE upload of the frames that are on the host and ONE dbx_resize_cubic_batch_nv12 launch over
    spec (job tuples as _resize_jobs takes them, b indexing the checked color._Frame list fr); the uint8 [len(spec), dh, dw, 3] CUDA
    tensor.  The converted full-resolution frame is never written."""
    from . import color
    dh, dw = spec[0][9], spec[0][10]
    up = color._Upload([f.t for f in fr], 0)
    up.send()
    out = torch.empty((len(spec), dh, dw, 3), dtype=torch.uint8, device=up.dev)
    jobs = (_lib.ResizeJobNv12 * len(spec))()
    for i, (r, (b, cx0, cy0, cw, ch, pl, pt, pr, pb, jh, jw)) in enumerate(zip(jobs, spec)):
        f = fr[b]
        r.y, r.uv, r.pitch_y, r.pitch_uv, r.sh, r.sw = up.base[b], up.base[b] + f.h * f.pitch, f.pitch, f.pitch, f.h, f.w
        r.cx0, r.cy0, r.cw, r.ch = cx0, cy0, cw, ch
        r.pad_l, r.pad_t, r.pad_r, r.pad_b, r.pad_value = pl, pt, pr, pb, PAD_VALUE
        r.dh, r.dw, r.dst_off = jh, jw, i * dh * dw * 3
    L = _lib.lib()
    ws = torch.empty(L.dbx_resize_batch_nv12_workspace_bytes(len(spec)), dtype=torch.uint8, device=up.dev)
    check(L.dbx_resize_cubic_batch_nv12(jobs, len(spec), C.byref(params.record()), C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()),
                                        stream_ptr()))
    return out


def _pad_resize_nv12_device(fr, size, params):
    """pad_resize_batch_nv12 on checked frames"""
    spec = []
    for b, f in enumerate(fr):
        side, px, py = pad_geometry(f.h, f.w)
        spec.append((b, 0, 0, f.w, f.h, px, py, side - f.w - px, side - f.h - py, size, size))
    return _resize_jobs_nv12(fr, spec, params)


def pad_resize_batch_nv12(frames, size=720, width=None, params=None):
    """pad_resize_batch on NV12 frames in ONE fused launch (dbx_resize_cubic_batch_nv12): bit for bit
    pad_resize_batch(color.nv12_to_rgb_batch(frames, width, params), size), but every tap is fetched from the NV12 surface and converted
    on the fly -- 1.5 source bytes per pixel in the place of 3, and no full-resolution RGB frame.  frames, width, params: as for
    color.nv12_to_rgb_batch.  Returns a uint8 [B, size, size, 3] CUDA tensor."""
    from . import color
    fn = 'pad_resize_batch_nv12'
    if not isinstance(size, (int, np.integer)) or size < 1:
        raise RuntimeError('%s: size must be a positive integer (the side of the square), got %r' % (fn, size))
    p = color._params(fn, params)
    return _pad_resize_nv12_device(color._frames(fn, frames, width), int(size), p)


def crop_resize_batch_nv12(frames, windows, size=(240, 240), width=None, params=None):
    """crop_resize_batch on NV12 frames in ONE fused launch: per frame b and window (x0, y0, x1, y1) of windows[b] (integers with
    Python-slice semantics; odd coordinates are fine: chroma is indexed by absolute source coordinates), the bicubic resize of the
    converted window to size = (width, height).  Returns a uint8 [P, height, width, 3] CUDA tensor in frame-then-window order."""
    from . import color
    fn = 'crop_resize_batch_nv12'
    dw, dh = _check_size(fn, size)
    p = color._params(fn, params)
    fr = color._frames(fn, frames, width)
    return _resize_jobs_nv12(fr, _window_spec(fn, [(f.h, f.w) for f in fr], windows, dh, dw), p)
