"""Plain Python / NumPy restatement of tiled detection's host and device arithmetic (test helper, the oracle of tests/test_tiles_*.py and
tests/test_hip_tiles*.py; it shares no code with the package): the plan of a frame, the map of a tile's rows to source-frame
coordinates, the ownership rule, the packing per frame and the NMS (pyramid_ref.nms_stable, the restatement the pyramid tests use)."""
import numpy as np

import pyramid_ref as P

INF = float('inf')
TILE = np.dtype([('frame', '<i4'), ('x0', '<i4'), ('y0', '<i4'), ('side', '<i4'), ('cw', '<i4'), ('ch', '<i4'), ('scale', '<f8'),
                 ('lo2x', '<f8'), ('hi2x', '<f8'), ('lo2y', '<f8'), ('hi2y', '<f8')])
NONE, CORE = 0, 1


def axis(L, S, overlap):
    """(starts, lo2, hi2) of the windows of side S along an axis of length L: one window at 0 when L <= S, else ceil((L - S) / D) + 1
    windows at min(i * D, L - S) with D = S - overlap; the doubled core bounds, -inf / +inf at the ends, s_i + S + s_(i+1) between."""
    assert L >= 1 and S >= 1 and 0 <= overlap and 2 * overlap <= S
    D = S - overlap
    n = 1 if L <= S else -((S - L) // D) + 1               # ceil((L - S) / D) + 1 in integers
    starts = [0] if L <= S else [min(i * D, L - S) for i in range(n)]
    mids = [starts[i] + S + starts[i + 1] for i in range(n - 1)]
    return starts, [-INF] + [float(m) for m in mids], [float(m) for m in mids] + [INF]


def plan(h, w, S, overlap, frame=0, scale=1.0):
    """the record array of one frame's tiles, row-major (y outer, x inner)"""
    xs, lx, hx = axis(w, S, overlap)
    ys, ly, hy = axis(h, S, overlap)
    out = np.zeros(len(xs) * len(ys), TILE)
    for iy, y0 in enumerate(ys):
        for ix, x0 in enumerate(xs):
            out[iy * len(xs) + ix] = (frame, x0, y0, S, min(S, w - x0), min(S, h - y0), scale, lx[ix], hx[ix], ly[iy], hy[iy])
    return out


def core_hits(table, rects):
    """bool per tile: its core (the points p with lo2 <= 2 p < hi2 on both axes) meets one of the integer rectangles (x0, y0, x1, y1),
    x0 <= p < x1"""
    hit = np.zeros(table.shape[0], bool)
    for i, t in enumerate(table):
        for x0, y0, x1, y1 in rects:
            if 2 * x0 < t['hi2x'] and 2 * x1 > t['lo2x'] and 2 * y0 < t['hi2y'] and 2 * y1 > t['lo2y']:
                hit[i] = True
    return hit


def map_rows(d, tile):
    """the rows of one tile in source-frame coordinates: d * scale - off with off = -origin, two float64 NumPy operations (the product
    is rounded before the subtraction); column 4 copied"""
    d = np.array(d, dtype=np.float64, copy=True).reshape(-1, np.shape(d)[-1])
    xs, ys = P.x_cols(d.shape[1]), P.y_cols(d.shape[1])
    scale, off_x, off_y = np.float64(tile['scale']), -np.float64(tile['x0']), -np.float64(tile['y0'])
    d[:, xs] = d[:, xs] * scale - off_x
    d[:, ys] = d[:, ys] * scale - off_y
    return d


def marks(mapped, tile, rule):
    """int32 per mapped row: 1 iff lo2x <= x1 + x2 < hi2x and lo2y <= y1 + y2 < hi2y (float64; NaN compares false), or 1 for NONE"""
    if rule == NONE:
        return np.ones(mapped.shape[0], np.int32)
    with np.errstate(invalid='ignore', over='ignore'):
        sx, sy = mapped[:, 0] + mapped[:, 2], mapped[:, 1] + mapped[:, 3]
        ok = (tile['lo2x'] <= sx) & (sx < tile['hi2x']) & (tile['lo2y'] <= sy) & (sy < tile['hi2y'])
    return ok.astype(np.int32)


def clamp(n, cap):
    return min(max(int(n), 0), cap)


def stitch(tile_rows, counts, table, frames, rpt, rule, thresh=0.4):
    """tile_rows[t]: the [rpt, dc] slot rows of tile t; counts[t]: its delivered count (None: rpt each), clamped to 0..rpt.
    Returns (stage, per frame results): stage = list per tile of (mapped rows [cnt, dc], marks [cnt]); per frame
    (packed rows [m, dc], keep list, table index of every row's tile [m]), the owned rows in tile order, then row order."""
    stage = []
    for t, tile in enumerate(table):
        cnt = rpt if counts is None else clamp(counts[t], rpt)
        m = map_rows(np.asarray(tile_rows[t])[:cnt], tile)
        stage.append((m, marks(m, tile, rule)))
    out = []
    dc = np.asarray(tile_rows[0]).shape[-1]
    for b in range(frames):
        rows, idx = [np.zeros((0, dc))], [np.zeros(0, np.int64)]
        for t, tile in enumerate(table):
            if tile['frame'] == b:
                m, k = stage[t]
                rows.append(m[k != 0])
                idx.append(np.full(int((k != 0).sum()), t, np.int64))
        rows = np.concatenate(rows)
        out.append((rows, P.nms_stable(rows, thresh) if rows.shape[0] else [], np.concatenate(idx)))
    return stage, out


def pairs_and_prefix(stage, out):
    """the count words of dbx_tile_nms_batch: per tile (delivered, owned), then the [frames + 1] prefix of the frames' row counts"""
    pairs = [v for m, k in stage for v in (m.shape[0], int((k != 0).sum()))]
    return np.array(pairs + [0] + list(np.cumsum([r.shape[0] for r, _, _ in out])), np.int32)


def tile_pixels(frame, tile, side_out, cubic):
    """the tile's pixels: the window cropped, padded right / bottom with 128 to side x side, resized by cubic_ref to side_out"""
    s, cw, ch = int(tile['side']), int(tile['cw']), int(tile['ch'])
    v = cubic.virtual_source(frame, (int(tile['x0']), int(tile['y0']), cw, ch), (0, 0, s - cw, s - ch), 128)
    return cubic.resize_cubic_u8(v, side_out, side_out)


# ---------------------------------------------------------------------------------------------------------------- crafted cases
# frame shapes (h, w) whose plans at S = 64, overlap = 16 have 1, 6, 2 and 64 tiles
SHAPES = {1: (50, 40), 6: (96, 160), 2: (64, 100), 64: (400, 400)}
CASES = {'1x1x1': ((1,), 1), '3x(1,6,2)x10': ((1, 6, 2), 10), '1x64x64': ((64,), 64)}


def case_table(tiles_per_frame, scale=1.0):
    """the table of a call whose frame b has tiles_per_frame[b] tiles (SHAPES); scale < 1: the windows are magnified"""
    parts = [plan(SHAPES[n][0], SHAPES[n][1], 64, 16, b, scale) for b, n in enumerate(tiles_per_frame)]
    assert [p.shape[0] for p in parts] == list(tiles_per_frame)
    return np.concatenate(parts)


def case_rows(seed, table, rpt, dc, nan=True):
    """Seeded slot rows [n_tiles, rpt, dc] in TILE coordinates on a quarter-pixel lattice (times scale: exact in float64): boxes 6..24
    wide around a few centres per tile, the centres up to 6 pixels outside the window, scores on a 1 / 64 lattice (ties).  Row 0 of every
    tile with a right-hand neighbour and row 1 of that neighbour are the SAME source box, its centre exactly on their common core boundary.
    nan: a few NaN scores and NaN boxes."""
    rs = np.random.RandomState(seed)
    n = table.shape[0]
    d = np.zeros((n, rpt, dc), np.float64)
    for t, tile in enumerate(table):
        side = tile['side'] / tile['scale']                           # the window in tile pixels
        nc = max(1, rpt // 5)
        cx, cy = rs.randint(-24, int(4 * side) + 24, nc) / 4.0, rs.randint(-24, int(4 * side) + 24, nc) / 4.0
        which = rs.randint(0, nc, rpt)
        w, h = rs.randint(24, 96, rpt) / 4.0, rs.randint(12, 48, rpt) / 4.0
        x1 = cx[which] + rs.randint(-12, 12, rpt) / 4.0 - w / 2
        y1 = cy[which] + rs.randint(-6, 6, rpt) / 4.0 - h / 2
        d[t, :, 0], d[t, :, 1], d[t, :, 2], d[t, :, 3] = x1, y1, x1 + w, y1 + h
        d[t, :, 4] = rs.randint(0, 65, rpt) / 64.0
        if dc == 13:
            d[t, :, 5:] = rs.randint(-40, int(4 * side) + 40, (rpt, 8)) / 4.0
    for t in range(n - 1):
        a, b = table[t], table[t + 1]
        if a['frame'] == b['frame'] and a['y0'] == b['y0'] and np.isfinite(a['hi2x']):
            assert a['hi2x'] == b['lo2x']
            # source box 10 x 6 with x1 + x2 = the boundary, its centre row inside both windows
            sx1, sy1 = (a['hi2x'] - 10.0) / 2, a['y0'] + 20.0
            for q, t_q, r in ((a, t, 0), (b, t + 1, min(1, rpt - 1))):   # row 0 in the left tile, row 1 in the right one
                d[t_q, r, :4] = [(sx1 - q['x0']) / q['scale'], (sy1 - q['y0']) / q['scale'], (sx1 + 10.0 - q['x0']) / q['scale'],
                                 (sy1 + 6.0 - q['y0']) / q['scale']]
                d[t_q, r, 4] = 2.0                                     # above every other score: it is kept wherever it is owned
                if dc == 13:                                           # the landmarks: the box corners, the same source points in both
                    d[t_q, r, 5:] = d[t_q, r, [0, 1, 2, 1, 2, 3, 0, 3]]
    if nan and rpt >= 4:
        for t in range(n):
            d[t, rpt - 1, 4] = np.nan                                 # a NaN score (ranked first by the NMS)
            d[t, rpt - 2, rs.randint(0, 4)] = np.nan                  # a NaN box: never owned under CORE
    return d


def case_counts(seed, n, rpt):
    """device count words for the threshold mode: 0, negative, above rpt and in between"""
    rs = np.random.RandomState(seed)
    c = rs.randint(0, rpt + 1, n)
    for i, v in zip(rs.permutation(n)[:3], (0, -5, rpt + 7)):
        c[i] = v
    return c.astype(np.int32)

