"""NumPy restatement of the pyramid merge (test helper, the oracle of tests/test_hip_pyramid.py): the rows of every level mapped back
to the source frame and concatenated level by level, and the reference's greedy NMS with the tie order made explicit."""
import numpy as np


def x_cols(dc):
    return [0, 2] + list(range(5, dc, 2))


def y_cols(dc):
    return [1, 3] + list(range(6, dc, 2))


def merge(level_dets, xforms):
    """level_dets: L arrays [K, dc] (dc = 5 or 13) of one frame; xforms: L (scale, off_x, off_y).  The [L * K, dc] float64 array whose
    row l * K + r is row r of level l with x * scale - off_x on the x columns, y * scale - off_y on the y columns -- two float64
    NumPy operations, the product rounded before the subtraction -- and the score column 4 copied."""
    out = []
    for d, (scale, off_x, off_y) in zip(level_dets, xforms):
        d = np.array(d, dtype=np.float64, copy=True)
        xs, ys = x_cols(d.shape[1]), y_cols(d.shape[1])
        d[:, xs] = d[:, xs] * np.float64(scale) - np.float64(off_x)
        d[:, ys] = d[:, ys] * np.float64(scale) - np.float64(off_y)
        out.append(d)
    return np.concatenate(out, axis=0)


def nms_stable(dets, thresh=0.4):
    """oracle.densebox_oracle.nms with the sort pinned: order = argsort(kind='stable')[::-1], so equal scores go HIGHER row index
    first (and NaN scores, which NumPy sorts last, come first).  The +1 pixel IoU and `ovr <= thresh` are the oracle's."""
    dets = np.asarray(dets, np.float64)
    x1, y1, x2, y2, sc = dets[:, 0], dets[:, 1], dets[:, 2], dets[:, 3], dets[:, 4]
    areas = (x2 - x1 + 1) * (y2 - y1 + 1)
    order = sc.argsort(kind='stable')[::-1]
    keep = []
    while order.size > 0:
        i = order[0]
        keep.append(int(i))
        rest = order[1:]
        with np.errstate(divide='ignore', invalid='ignore'):
            w = np.maximum(0.0, np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]) + 1)
            h = np.maximum(0.0, np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]) + 1)
            inter = w * h
            ovr = inter / (areas[i] + areas[rest] - inter)
        order = rest[ovr <= thresh]
    return keep


def random_frame(rs, n, dc, span=1920.0, quantise=None, nan_every=0):
    """n seeded boxes [n, dc] in a span x span frame: plate-like boxes 40..300 wide clustered around a few centres (so that many
    overlap), continuous scores unless quantise (scores rounded to 1 / quantise: ties), every nan_every-th score NaN."""
    nc = max(1, n // 6)
    cx, cy = rs.uniform(0, span, nc), rs.uniform(0, span, nc)
    which = rs.randint(0, nc, n)
    w, h = rs.uniform(40, 300, n), rs.uniform(15, 120, n)
    x1 = cx[which] + rs.uniform(-40, 40, n) - w / 2
    y1 = cy[which] + rs.uniform(-20, 20, n) - h / 2
    d = np.zeros((n, dc), np.float64)
    d[:, 0], d[:, 1], d[:, 2], d[:, 3] = x1, y1, x1 + w, y1 + h
    d[:, 4] = rs.uniform(0.0, 1.0, n)
    if quantise:
        d[:, 4] = np.round(d[:, 4] * quantise) / quantise
    else:
        assert len(np.unique(d[:, 4])) == n, 'the generator must give pairwise distinct scores'
    if nan_every:
        d[::nan_every, 4] = np.nan
    if dc == 13:
        d[:, 5:13] = rs.uniform(-50, span + 50, (n, 8))
    return d
