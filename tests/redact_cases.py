"""The crafted rows, tracks and styles that tests/test_redact_abi.py (dbx_redact_host, no GPU) and tests/test_hip_redact.py (the kernel)
both compare with the restatement (tests/redact_ref.py)."""
import numpy as np

from densebox_amd import track as T

NAN, INF = float('nan'), float('inf')
COAST = 3
SIZES = [(1, 1), (5, 7), (17, 33), (67, 130)]
BASE = dict(color=(200, 100, 50, 25), grow=1, grow_pct=10, coast=COAST, min_score=0.1)
METHODS = ([dict(method='fill')] + [dict(method='pixelate', cell=s) for s in (2, 3, 7, 32)]
           + [dict(method='blur', radius=r) for r in (1, 5, 16)])


def styles():
    """every (method and its size) x shape, as keyword arguments of redact.Redaction and as style dicts of the restatement"""
    return [dict(BASE, shape=shape, **m) for m in METHODS for shape in ('box', 'quad')]


def _bounds(lm):
    return [min(lm[0::2]), min(lm[1::2]), max(lm[0::2]), max(lm[1::2])]


def crafted(h, w):
    """13-column rows for an h x w frame that exercise every clipping, rejection and fall-back rule.  Everything but the row clipped at
    the right border (which stays in the top rows) ends at x <= 0.6 w, so the bottom right corner of a frame larger than 1 x 1 stays
    uncovered."""
    boxes = [
        [0.15 * w, 0.3 * h, 0.4 * w, 0.6 * h],                       # inside
        [-5.3, 0.5 * h, 0.2, 0.5 * h + 0.4],                         # clipped at the left border
        [w - 1.2, 0.1 * h, w + 6.0, 0.1 * h + 0.4],                  # ... the right
        [0.5 * w, -6.0, 0.5 * w + 0.4, 0.2],                         # ... the top
        [0.3 * w, h - 1.2, 0.3 * w + 0.4, h + 5.0],                  # ... the bottom
        [w + 50.0, h + 50.0, w + 80.0, h + 70.0],                    # wholly outside
        [-100.0, -100.0, -60.0, -70.0],
        [0.6 * w, 0.9 * h, 0.5 * w, 0.75 * h],                       # inverted
        [0.45 * w, 0.45 * h, 0.45 * w, 0.45 * h],                    # one pixel
        [0.3 * w, 0.35 * h, 0.5 * w, 0.55 * h],                      # two that overlap
        [0.35 * w, 0.45 * h, 0.55 * w, 0.7 * h],
        [NAN, 1.0, 5.0, 6.0],                                        # not usable: no region
        [1.0, 2.0, INF, 6.0],
        [1.0, 2.0 ** 30, 3.0, 4.0],
    ]
    rows = np.zeros((len(boxes) + 9, 13))
    n = len(boxes)
    for i, b in enumerate(boxes):
        x1, y1, x2, y2 = b
        rows[i, :4] = b
        rows[i, 5:] = [x1, y1, x2, y1, x2, y2, x1, y2]               # the box's corners, clockwise on the screen
    quads = [
        [0.1 * w, 0.6 * h, 0.35 * w, 0.55 * h, 0.4 * w, 0.8 * h, 0.15 * w, 0.9 * h],              # clockwise on the screen
        [0.58 * w, 0.05 * h, 0.6 * w, 0.35 * h, 0.4 * w, 0.3 * h, 0.45 * w, 0.1 * h],             # counter-clockwise
        [0.05 * w, 0.05 * h, 0.3 * w, 0.1 * h, 0.12 * w, 0.12 * h, 0.1 * w, 0.3 * h],             # concave at P_2
        [0.5 * w, 0.8 * h] * 4,                                                                   # zero area: the box
        [3.0, 9.0, 7.0, 9.0, 11.0, 9.0, 7.0, 15.0],                                               # tri(G_0, G_1, G_2) has zero area
        [0.0, 0.0, 0.2 * w, 0.2 * h, 0.2 * w, 0.0, 0.0, 0.2 * h],                                 # a bow tie: zero shoelace
    ]
    for j, lm in enumerate(quads):
        rows[n + j, :4], rows[n + j, 5:] = _bounds(lm), lm
    # a landmark at -2^20, a NaN landmark, a landmark just inside the bound: the first two fall back to the box; the third is a sliver
    # whose growth, a tenth of its size, pushes it across the whole width: it stays in the top rows
    for j, v in enumerate((-2.0 ** 20, NAN, 1 - 2.0 ** 20)):
        rows[n + 6 + j, :4] = [0.2 * w + j, 0.0, 0.3 * w + j, 0.1 * h]
        rows[n + 6 + j, 5:] = [0.2 * w + j, 0.0, 0.3 * w + j, 0.0, 0.3 * w + j, 0.1 * h, v, 0.1 * h]
    rows[:, 4] = 0.5
    rows[0, 4], rows[9, 4], rows[3, 4], rows[7, 4] = NAN, 0.05, 0.1, INF       # NaN: redacted; below min_score = 0.1: skipped; at it: redacted
    return rows


def keep_lists(h, w):
    """raw keep records [count, entries...] for crafted(h, w) on `slots = n` list positions: every row in a seeded order; entries out of
    range among them; a count above slots"""
    n = crafted(h, w).shape[0]
    order = [int(v) for v in np.random.RandomState(h * 1000 + w).permutation(n)]
    return [[n] + order, [n] + [-1, n, 1 << 30] + order[:n - 3], [n + 5] + order]


def tracks(h, w):
    """a stream's table of 8 slots: coasting at ages 1 and COAST (redacted), matched (age 0), too old, free slots, an unusable box"""
    t = np.zeros(8, T.TRACK)
    t['id'] = [4, 5, 6, 7, -1, 9, -1, 11]
    t['age'] = [1, COAST, 0, COAST + 1, 1, 2, 0, -1]
    t['box'] = [[0.05 * w, 0.75 * h, 0.2 * w, 0.85 * h], [0.1 * w, 0.02 * h, 0.25 * w, 0.08 * h], [0.5 * w, 0.6 * h, 0.6 * w, 0.7 * h],
                [0.2 * w, 0.05 * h, 0.3 * w, 0.15 * h], [0.4 * w, 0.4 * h, 0.5 * w, 0.5 * h], [NAN, 1.0, 2.0, 3.0],
                [0.0, 0.0, w, h], [0.0, 0.0, w, h]]
    t['vel'], t['score'] = 0.25, 0.5
    return t


def effective(raw, n, slots):
    """the list the kernel walks for a raw keep record: the count clamped to 0..min(n, slots)"""
    k = min(max(int(raw[0]), 0), min(n, slots))
    return [int(v) for v in raw[1:1 + k]]
