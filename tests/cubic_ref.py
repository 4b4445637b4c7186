"""Plain NumPy integer restatement of the 8-bit bicubic resize the batched resize kernel computes (the generic C path of OpenCV's
INTER_CUBIC: float32 coefficients with A = -0.75 rounded to 11-bit fixed point, a replicate border, integer accumulation,
(acc + 2^21) >> 22).  It is the oracle of tests/test_hip_resize_batch.py, shares no code with the package, and is itself pinned
against torch's CPU bicubic interpolation in tests/test_resize_abi.py."""
import numpy as np

COEF_BITS = 11


def cubic_taps(n_src, n_dst):
    """Per destination index of an axis with n_src samples resized to n_dst: (first tap index s - 1, int64 [n_dst]; the four
    16-bit coefficients, int64 [n_dst, 4])."""
    scale = np.float64(n_src) / np.float64(n_dst)
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    f = (f - s).astype(np.float32)
    A, one = np.float32(-0.75), np.float32(1)
    f1, g = (f + one).astype(np.float32), (one - f).astype(np.float32)
    c0 = ((A * f1 - np.float32(5) * A) * f1 + np.float32(8) * A) * f1 - np.float32(4) * A
    c1 = ((A + np.float32(2)) * f - (A + np.float32(3))) * f * f + one
    c2 = ((A + np.float32(2)) * g - (A + np.float32(3))) * g * g + one
    c3 = one - c0 - c1 - c2
    c = np.stack([c0, c1, c2, c3], axis=1)
    assert c.dtype == np.float32
    q = np.rint(c * np.float32(1 << COEF_BITS))                     # nearest, ties to even; no sum correction
    return s.astype(np.int64) - 1, np.clip(q, -32768, 32767).astype(np.int64)


def resize_cubic_u8(virtual_source, dh, dw):
    """uint8 [vh, vw] or [vh, vw, C] -> uint8 [dh, dw(, C)]."""
    v = np.asarray(virtual_source)
    assert v.dtype == np.uint8 and v.ndim in (2, 3) and dh >= 1 and dw >= 1
    src = (v if v.ndim == 3 else v[:, :, None]).astype(np.int64)
    vh, vw = src.shape[:2]
    x0, alpha = cubic_taps(vw, dw)
    y0, beta = cubic_taps(vh, dh)
    hor = np.zeros((vh, dw, src.shape[2]), dtype=np.int64)
    for k in range(4):
        hor += src[:, np.clip(x0 + k, 0, vw - 1), :] * alpha[:, k][None, :, None]
    acc = np.zeros((dh, dw, src.shape[2]), dtype=np.int64)
    bound = np.zeros((dh, 1, 1), dtype=np.int64)
    for k in range(4):
        rows = hor[np.clip(y0 + k, 0, vh - 1)]
        acc += rows * beta[:, k][:, None, None]
        bound += np.abs(beta[:, k])[:, None, None] * np.abs(rows).max(axis=(1, 2), keepdims=True)
    # the kernel accumulates in 32 bits: every partial sum, in any order, is bounded by sum |beta| * max |row|
    assert int(bound.max()) < 2 ** 31 and int(np.abs(acc).max()) < 2 ** 31, (int(bound.max()), int(np.abs(acc).max()))
    out = np.clip((acc + (1 << (2 * COEF_BITS - 1))) >> (2 * COEF_BITS), 0, 255).astype(np.uint8)
    return out if v.ndim == 3 else out[:, :, 0]


def virtual_source(img, crop=None, pad=(0, 0, 0, 0), pad_value=0):
    """np.pad of img[cy0:cy0 + ch, cx0:cx0 + cw] (crop = (cx0, cy0, cw, ch), default the whole image) with pad = (left, top,
    right, bottom) columns / rows of pad_value."""
    img = np.asarray(img)
    cx0, cy0, cw, ch = crop if crop is not None else (0, 0, img.shape[1], img.shape[0])
    assert 0 <= cx0 and 0 <= cy0 and cw >= 1 and ch >= 1 and cx0 + cw <= img.shape[1] and cy0 + ch <= img.shape[0]
    l, t, r, b = pad
    widths = ((t, b), (l, r)) + ((0, 0),) * (img.ndim - 2)
    return np.pad(img[cy0:cy0 + ch, cx0:cx0 + cw], widths, 'constant', constant_values=pad_value)


def pad_square(img, value=128):
    """The geometry of the reference's pad_img, restated: the short side padded to the long one, the extra pixel of an odd
    difference on the right / bottom."""
    h, w = img.shape[:2]
    lu = abs(h - w) // 2
    rd = abs(h - w) - lu
    return virtual_source(img, None, (0, lu, 0, rd) if h <= w else (lu, 0, rd, 0), value)


def pad_resize(img, size):
    return resize_cubic_u8(pad_square(img), size, size)
