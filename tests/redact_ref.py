"""NumPy / Python-int restatement of dbx_redact_batch (include/densebox_hip.h has the contract), one frame at a time: the regions of the
kept rows and of the coasting tracks as Python ints, their coverage as a mask over the whole frame, the value of every pixel from the
source alone.  It shares nothing with the kernel's tiles, lists or staged sums; C's truncating division is spelled out (tdiv)."""
import math

import numpy as np

STYLE = dict(method='pixelate', shape=None, cell=12, radius=8, color=(0, 0, 0), grow=2, grow_pct=10, coast=0, min_score=-math.inf)


def tdiv(a, b):
    """C's a / b on ints: the quotient truncated toward zero"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def sgn(v):
    return (v > 0) - (v < 0)


def usable(v):
    return math.isfinite(v) and abs(v) < 2.0 ** 30


def I(v):
    """v + 0.5 in float64, truncated toward zero"""
    return int(float(v) + 0.5)


def box_region(box, st):
    """(xa, xb, ya, yb), inclusive and not yet clipped, of the grown box; None when a coordinate is not usable"""
    b = [float(v) for v in box]
    if not all(usable(v) for v in b):
        return None
    X1, Y1, X2, Y2 = (I(v) for v in b)
    L, R, Tp, Bt = min(X1, X2), max(X1, X2), min(Y1, Y2), max(Y1, Y2)
    gx = st['grow'] + tdiv((R - L + 1) * st['grow_pct'], 100)
    gy = st['grow'] + tdiv((Bt - Tp + 1) * st['grow_pct'], 100)
    return L - gx, R + gx, Tp - gy, Bt + gy


def quad_vertices(lm, st):
    """G_0..G_3 in quarter pixels as [(x, y)] * 4 from the eight landmark values; None when the row falls back to its box"""
    lm = [float(v) for v in lm]
    if not all(math.isfinite(v) and abs(v) < 2.0 ** 20 for v in lm):
        return None
    P = [(I(lm[2 * q]), I(lm[2 * q + 1])) for q in range(4)]
    if sum(P[q][0] * P[(q + 1) % 4][1] - P[(q + 1) % 4][0] * P[q][1] for q in range(4)) == 0:
        return None
    G = []
    for q in range(4):
        g = []
        for axis in range(2):
            S = sum(p[axis] for p in P)
            d = 4 * P[q][axis] - S
            g.append(4 * P[q][axis] + tdiv(d * st['grow_pct'], 100) + 4 * st['grow'] * sgn(d))
        G.append(tuple(g))
    return G


def regions(dets, keep, tracks, st):
    """the regions of a frame: ('box', (xa, xb, ya, yb)) or ('quad', [G_0..G_3])"""
    dets = np.asarray(dets, np.float64)
    quad = st['shape'] == 'quad' or (st['shape'] is None and dets.ndim == 2 and dets.shape[1] == 13)
    out = []
    for row_no in keep:
        if row_no < 0 or row_no >= dets.shape[0]:
            continue
        row = [float(v) for v in dets[row_no]]
        if row[4] < st['min_score']:                              # (false for a NaN score: it is redacted)
            continue
        box = box_region(row[:4], st)
        if box is None:
            continue
        G = quad_vertices(row[5:13], st) if quad and len(row) == 13 else None
        out.append(('quad', G) if G is not None else ('box', box))
    if tracks is not None and st['coast'] > 0:
        for t in tracks:
            if int(t['id']) >= 0 and 1 <= int(t['age']) <= st['coast']:
                box = box_region(t['box'], st)
                if box is not None:
                    out.append(('box', box))
    return out


def _triangle(a, b, c, X, Y):
    area2 = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    if area2 == 0:
        return np.zeros(X.shape, bool)
    s = sgn(area2)
    inside = np.ones(X.shape, bool)
    for p, q in ((a, b), (b, c), (c, a)):
        inside &= s * ((q[0] - p[0]) * (Y - p[1]) - (q[1] - p[1]) * (X - p[0])) >= 0
    return inside


def mask_of(region, h, w):
    """the pixels of an h x w frame that the region covers"""
    kind, v = region
    m = np.zeros((h, w), bool)
    if kind == 'box':
        xa, xb, ya, yb = v
        m[max(ya, 0):max(min(yb, h - 1) + 1, 0), max(xa, 0):max(min(xb, w - 1) + 1, 0)] = True
        return m
    yy, xx = np.mgrid[:h, :w].astype(np.int64)
    return _triangle(v[0], v[1], v[2], 4 * xx, 4 * yy) | _triangle(v[0], v[2], v[3], 4 * xx, 4 * yy)


def _style(style):
    st = dict(STYLE)
    st.update(style or {})
    return st


def covered(h, w, dets, keep, tracks=None, style=None):
    """int [h, w]: how many regions cover each pixel"""
    count = np.zeros((h, w), np.int64)
    for region in regions(dets, keep, tracks, _style(style)):
        count += mask_of(region, h, w)
    return count


_VALUES = {}


def values(img, style=None):
    """what every pixel would become if a region covered it: a function of the source alone (memoised on the image's bytes)"""
    st = _style(style)
    img = np.asarray(img, np.uint8)
    h, w, c = img.shape
    method = st['method']
    if method == 'fill':
        out = np.empty_like(img)
        out[:] = np.array((tuple(st['color']) + (0,) * 4)[:c], np.uint8)
        return out
    key = (img.shape, img.tobytes(), method, st['cell'] if method == 'pixelate' else st['radius'])
    if key in _VALUES:
        return _VALUES[key]
    src = img.astype(np.int64)
    out = np.empty_like(img)
    if method == 'pixelate':
        s = st['cell']
        for ya in range(0, h, s):
            for xa in range(0, w, s):
                yb, xb = min(ya + s, h), min(xa + s, w)
                n = (yb - ya) * (xb - xa)
                out[ya:yb, xa:xb] = (src[ya:yb, xa:xb].sum(axis=(0, 1)) + n // 2) // n
    else:
        assert method == 'blur', method
        r = st['radius']
        A = (2 * r + 1) ** 2
        ys, xs = np.clip(np.arange(-r, h + r), 0, h - 1), np.clip(np.arange(-r, w + r), 0, w - 1)
        pad = src[ys][:, xs]                                          # replicated edges: pad[y + r + dy][x + r + dx]
        total = np.zeros_like(src)
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                total += pad[dy:dy + h, dx:dx + w]
        out[:] = (total + A // 2) // A
    if len(_VALUES) > 64:
        _VALUES.clear()
    _VALUES[key] = out
    return out


def redact(img, dets, keep, tracks=None, style=None, count=None):
    """One frame: img uint8 [h, w, c]; dets float64 [n, 5|13]; keep the list of kept rows (an entry outside 0..n-1 is ignored); tracks a
    structured array with 'box', 'id' and 'age' (track.TRACK), or None.  style: a dict over STYLE; shape None means quad for rows of 13
    columns.  count: an int array [h, w] that receives the number of regions covering each pixel.  Returns the redacted copy."""
    img = np.asarray(img, np.uint8)
    h, w, _ = img.shape
    n = covered(h, w, dets, keep, tracks, style)
    if count is not None:
        count += n
    out = np.array(img, copy=True)
    m = n > 0
    out[m] = values(img, style)[m]
    return out
