"""NumPy restatement of the NV12 semantics include/densebox_hip.h states (this project's own): the 14-bit integer conversion in both
directions, with the coefficients DERIVED from Kr and Kb (the header holds them as constants; tests/test_nv12_ref.py compares the two),
the float64 formula they approximate, and the fused resize as cubic_ref applied to the converted frame."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'densebox_hip.h')

KRB = {601: (0.299, 0.114), 709: (0.2126, 0.0722)}
VARIANTS = [(601, 'limited'), (601, 'full'), (709, 'limited'), (709, 'full')]
ONE = 16384.0


def _scales(rng):
    """(ys, cs, yo) of the direction to RGB; the other direction uses their reciprocals"""
    return (255.0 / 219.0, 255.0 / 224.0, 16) if rng == 'limited' else (1.0, 1.0, 0)


def to_rgb_float(standard, rng):
    """(ky, rv, gu, gv, bu) as float64"""
    kr, kb = KRB[standard]
    kg = 1.0 - kr - kb
    ys, cs, _ = _scales(rng)
    return (ys, cs * 2.0 * (1.0 - kr), -cs * 2.0 * kb * (1.0 - kb) / kg, -cs * 2.0 * kr * (1.0 - kr) / kg, cs * 2.0 * (1.0 - kb))


def from_rgb_float(standard, rng):
    """((yr, yg, yb), (ur, ug, ub), (vr, vg, vb)) as float64"""
    kr, kb = KRB[standard]
    kg = 1.0 - kr - kb
    ys, cs, _ = _scales(rng)
    ys, cs = 1.0 / ys, 1.0 / cs
    return ((ys * kr, ys * kg, ys * kb),
            tuple(cs * v / (2.0 * (1.0 - kb)) for v in (-kr, -kg, 1.0 - kb)),
            tuple(cs * v / (2.0 * (1.0 - kr)) for v in (1.0 - kr, -kg, -kb)))


def to_rgb_coef(standard, rng):
    return tuple(int(np.rint(c * ONE)) for c in to_rgb_float(standard, rng))


def from_rgb_coef(standard, rng):
    return tuple(int(np.rint(c * ONE)) for row in from_rgb_float(standard, rng) for c in row)


def header_constants():
    """{(standard, range): (the five to-RGB integers, the nine from-RGB integers)} as include/densebox_hip.h defines them"""
    src = open(HEADER).read()
    out = {}
    for std, rng in VARIANTS:
        got = []
        for way in ('TO_RGB', 'FROM_RGB'):
            m = re.search(r'#define\s+DBX_NV12_%d_%s_%s\s+([-0-9, ]+)\n' % (std, rng.upper(), way), src)
            assert m, 'DBX_NV12_%d_%s_%s is not defined' % (std, rng.upper(), way)
            got.append(tuple(int(v) for v in m.group(1).split(',')))
        out[(std, rng)] = tuple(got)
    return out


def _clip8(v):
    return np.clip(v, 0, 255).astype(np.uint8)


def yuv_to_rgb(Y, U, V, standard=601, rng='limited', order='rgb'):
    """the pixel rule on integer arrays of one shape: uint8 [..., 3]"""
    ky, rv, gu, gv, bu = to_rgb_coef(standard, rng)
    yo = _scales(rng)[2]
    C, D, E = Y.astype(np.int64) - yo, U.astype(np.int64) - 128, V.astype(np.int64) - 128
    R = _clip8((ky * C + rv * E + 8192) >> 14)
    G = _clip8((ky * C + gu * D + gv * E + 8192) >> 14)
    B = _clip8((ky * C + bu * D + 8192) >> 14)
    return np.stack([R, G, B] if order == 'rgb' else [B, G, R], axis=-1)


def yuv_to_rgb_float(Y, U, V, standard=601, rng='limited'):
    """the float64 formula, rounded to nearest and clipped: what the integers approximate"""
    ky, rv, gu, gv, bu = to_rgb_float(standard, rng)
    yo = _scales(rng)[2]
    C, D, E = Y.astype(np.float64) - yo, U.astype(np.float64) - 128, V.astype(np.float64) - 128
    return np.stack([_clip8(np.rint(ky * C + rv * E)), _clip8(np.rint(ky * C + gu * D + gv * E)), _clip8(np.rint(ky * C + bu * D))], axis=-1)


def split(frame, w=None):
    """(Y [h, w], UV [h/2, w]) views of a [h * 3 / 2, pitch] frame"""
    rows, pitch = frame.shape
    assert rows % 3 == 0
    h = rows // 3 * 2
    w = pitch if w is None else w
    assert w % 2 == 0 and 0 < w <= pitch
    return frame[:h, :w], frame[h:, :w]


def nv12_to_rgb(frame, w=None, standard=601, rng='limited', order='rgb'):
    """uint8 [h, w, 3] of a uint8 [h * 3 / 2, pitch] frame: chroma replicated over its 2 x 2 block, no interpolation"""
    Y, UV = split(np.asarray(frame), w)
    U = np.repeat(np.repeat(UV[:, 0::2], 2, axis=0), 2, axis=1)
    V = np.repeat(np.repeat(UV[:, 1::2], 2, axis=0), 2, axis=1)
    return yuv_to_rgb(Y, U, V, standard, rng, order)


def rgb_to_yuv_blocks(img, standard=601, rng='limited', order='rgb'):
    """(Y [h, w], U [h/2, w/2], V [h/2, w/2]) uint8 of a uint8 [h, w, 3] image with even h and w"""
    img = np.asarray(img)
    h, w = img.shape[:2]
    assert h % 2 == 0 and w % 2 == 0 and h > 0 and w > 0
    k = from_rgb_coef(standard, rng)
    yo = _scales(rng)[2]
    p = img.astype(np.int64)
    if order == 'bgr':
        p = p[..., ::-1]
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = _clip8(((k[0] * R + k[1] * G + k[2] * B + 8192) >> 14) + yo)
    s = p.reshape(h // 2, 2, w // 2, 2, 3).sum(axis=(1, 3))
    U = _clip8(((k[3] * s[..., 0] + k[4] * s[..., 1] + k[5] * s[..., 2] + 32768) >> 16) + 128)
    V = _clip8(((k[6] * s[..., 0] + k[7] * s[..., 1] + k[8] * s[..., 2] + 32768) >> 16) + 128)
    return Y, U, V


def rgb_to_yuv_float(img, standard=601, rng='limited'):
    """the float64 formula on the block MEANS for chroma, rounded to nearest and clipped"""
    (yr, yg, yb), (ur, ug, ub), (vr, vg, vb) = from_rgb_float(standard, rng)
    yo = _scales(rng)[2]
    p = np.asarray(img).astype(np.float64)
    h, w = p.shape[:2]
    Y = _clip8(np.rint(yr * p[..., 0] + yg * p[..., 1] + yb * p[..., 2]) + yo)
    m = p.reshape(h // 2, 2, w // 2, 2, 3).sum(axis=(1, 3)) / 4.0
    U = _clip8(np.rint(ur * m[..., 0] + ug * m[..., 1] + ub * m[..., 2]) + 128)
    V = _clip8(np.rint(vr * m[..., 0] + vg * m[..., 1] + vb * m[..., 2]) + 128)
    return Y, U, V


def rgb_to_nv12(img, standard=601, rng='limited', order='rgb'):
    """the uint8 [h * 3 / 2, w] frame of a uint8 [h, w, 3] image"""
    Y, U, V = rgb_to_yuv_blocks(img, standard, rng, order)
    h, w = Y.shape
    out = np.empty((h * 3 // 2, w), np.uint8)
    out[:h] = Y
    out[h:, 0::2], out[h:, 1::2] = U, V
    return out


def resize_nv12(frame, dsize, w=None, window=None, pad=(0, 0, 0, 0), pad_value=128, **params):
    """the fused resize: cubic_ref's resize of the converted frame's window (x0, y0, x1, y1) with pad = (l, t, r, b) constant columns
    / rows of pad_value in all three channels around it; dsize = (width, height)"""
    import cubic_ref
    rgb = nv12_to_rgb(frame, w, **params)
    crop = None
    if window is not None:
        x0, y0, x1, y1 = window
        crop = (x0, y0, x1 - x0, y1 - y0)
    return cubic_ref.resize_cubic_u8(cubic_ref.virtual_source(rgb, crop, pad, pad_value), dsize[1], dsize[0])
