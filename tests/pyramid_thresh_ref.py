"""NumPy restatement of the variable-count pyramid merge (dbx_merge_nms_thresh_batch) for the tests, and the seeded cases its kernel
tests run on.  It adds no arithmetic of its own: the union is pyramid_ref.merge on the first n_(l,b) rows of every level, the keep list
pyramid_ref.nms_stable on it.  Not collected."""
import numpy as np

import pyramid_ref as P

# (scale, off_x, off_y) per level: 1080 x 1920 at 480 / 720 / 1080, and a portrait frame with an odd difference at 320
XFORMS = [(1920 / 480, 0.0, 420.0), (1920 / 720, 0.0, 420.0), (1920 / 1080, 0.0, 420.0), (517 / 320, 108.0, 0.0)]


def clamp(n, cap):
    return min(max(int(n), 0), int(cap))


def merge_nms(level_dets, counts, xforms, cap, thresh=0.4):
    """One frame.  level_dets: L arrays [cap, dc] of which the first clamp(counts[l]) rows count; xforms: L (scale, off_x, off_y).
    Returns (union float64 [m, dc], keep list of union rows)."""
    dc = level_dets[0].shape[1]
    parts = [np.asarray(d, np.float64)[:clamp(n, cap)] for d, n in zip(level_dets, counts)]
    union = P.merge(parts, xforms).reshape(-1, dc)
    return union, P.nms_stable(union, thresh)


def frame_levels(rs, kind, levels, cap, dc):
    """`cap` rows for every level of one frame, in RESIZED-frame coordinates.  kind 0: continuous scores; 1: scores quantised to 1/8
    (ties within and ACROSS levels); 2: every 7th score NaN and every 11th row with a NaN coordinate; 3: the same rows at every level
    (identical boxes and scores after the map: frame_xforms gives such a frame one transform)."""
    if kind == 3:
        d = P.random_frame(rs, cap, dc, span=700.0)
        return [d.copy() for _ in range(levels)]
    out = [P.random_frame(rs, cap, dc, span=1920.0 / XFORMS[l % 4][0], quantise=8 if kind == 1 else None, nan_every=7 if kind == 2 else 0)
           for l in range(levels)]
    if kind == 2:
        for l, d in enumerate(out):
            d[3::11, l % 4] = np.nan
    return out


def frame_xforms(kind, b, levels):
    return [XFORMS[1] if kind == 3 else (XFORMS[3] if (b % 2 == 1 and l == 0) else XFORMS[l % 4]) for l in range(levels)]


def count_pattern(p, levels, cap):
    """per-level counts of a frame: 0 all at the cap; 1 empty at every level; 2 the 64-row block edges; 3 empty at some levels; 4 edges
    the other way round"""
    return [[cap] * 4, [0] * 4, [63, 64, 65, 1], [0, cap // 2, 0, 7], [1, 65, 64, 63]][p][:levels]


def grid_case(levels, batch, dc, cap=100):
    """(frames, counts, xforms) with frames[b][l] = [cap, dc] rows, counts[b][l], xforms[b][l]"""
    rs = np.random.RandomState(100 * levels + 10 * batch + dc)
    patterns = list(range(batch)) if batch > 1 else [[0, 2, 4, 3][levels - 1]]
    kinds = [(b + levels) % 4 for b in range(batch)]
    frames = [frame_levels(rs, k, levels, cap, dc) for k in kinds]
    counts = [count_pattern(p, levels, cap) for p in patterns]
    xforms = [frame_xforms(k, b, levels) for b, k in enumerate(kinds)]
    return frames, counts, xforms


def full_case(which):
    """unions of exactly 4096 rows: 4 levels at 1024 rows each (and a second frame with a hole), or one level at 4096"""
    rs = np.random.RandomState(4096 + which)
    if which == 0:
        levels, cap, dc, counts = 4, 1024, 5, [[1024] * 4, [1024, 0, 1000, 1]]
    else:
        levels, cap, dc, counts = 1, 4096, 13, [[4096]]
    frames = [frame_levels(rs, b, levels, cap, dc) for b in range(len(counts))]
    xforms = [frame_xforms(b, b, levels) for b in range(len(counts))]
    return frames, counts, xforms, cap


def non_trivial(frames, counts, xforms, cap, thresh=0.4):
    """(some frame has rows of two levels, some frame loses a row to the NMS and keeps more than one) under the restatement alone"""
    two = any(sum(clamp(n, cap) > 0 for n in c) >= 2 for c in counts)
    nms = False
    for f, c, x in zip(frames, counts, xforms):
        union, keep = merge_nms(f, c, x, cap, thresh)
        nms = nms or (1 < len(keep) < len(union))
    return two, nms
