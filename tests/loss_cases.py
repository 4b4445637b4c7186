"""Inputs and references for the fused-loss edge cases (tests/test_loss_cases.py on the CPU, tests/test_hip_loss_cases.py on the GPU).

Plain NumPy / torch CPU on top of oracle/densebox_oracle.py, which stays the reference: nothing here computes a mask or a target the
oracle does not.  What this module adds is (a) the tables -- boxes over every edge of the 60 x 60 grid, landmarks in the border rows and
columns -- each row named for the branch of the reference's slice arithmetic it was sized for, with a predicate that says so from
``O._rect`` / ``O._py_slice`` alone; (b) ``loss64``, the scalar reference (the oracle's ``torch.sum`` is a float32 sum and less exact than
the kernel's double accumulation); (c) ``tie_order``, the selection rule of the kernel's two top-K paths restated; (d) a variant of the
label arithmetic with two switches, used only to show that the tables are sensitive to the two readings a kernel could get wrong.
"""
import os

import numpy as np
import torch

from oracle import densebox_oracle as O

HW = 60
NPIX = HW * HW
KINDS = ('DenseBox', 'DenseBoxLM', 'DenseBoxLMLOC')
TOL_LOSS = 2.0 ** -22            # the kernel rounds a double sum of non-negative terms to float32 once (2**-24); the rest is margin
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


# ------------------------------------------------------------------------------------------------ geometry
def spans(box):
    """Raw and normalised extents of one box: 'raw0' / 'raw2' = (ox, ex, oy, ey) of the centre rectangle and of the gray rectangle,
    'core' / 'zero' / 'recore' = ((ya, yb), (xa, xb)) of init_score_map's ones, mask_gray_zone_cls's zeroed block and its re-set core."""
    b = np.asarray(box, np.float32)
    ox, ex = O._rect(b[0], b[2], 0.3, 0.0)
    oy, ey = O._rect(b[1], b[3], 0.3, 0.0)
    gx, hx = O._rect(b[0], b[2], 0.3, 2.0)
    gy, hy = O._rect(b[1], b[3], 0.3, 2.0)
    return {'raw0': (ox, ex, oy, ey), 'raw2': (gx, hx, gy, hy),
            'core': (O._py_slice(oy, ey + 1), O._py_slice(ox, ex + 1)),
            'zero': (O._py_slice(gy, hy), O._py_slice(gx, hx)),
            'recore': (O._py_slice(gy + 2, hy - 2 + 1), O._py_slice(gx + 2, hx - 2 + 1))}


def _area(sp):
    return (sp[0][1] - sp[0][0]) * (sp[1][1] - sp[1][0])


def _axes(raw):
    return ((raw[0], raw[1]), (raw[2], raw[3]))


# branch name -> predicate on spans(box): what the row named for it has to hit, decided from the reference's arithmetic alone
BRANCH = {
    # a start in -60..-1 wraps to the far side and the slice [start + 60, stop) is empty although the rectangle overlaps the grid
    'wrap-empty': lambda s: _area(s['core']) == 0 and any(-HW <= o < 0 <= e + 1 for o, e in _axes(s['raw0'])),
    # centre - half + 0.5 in (-1, 0): int() truncates toward zero, the core starts at 0, while the gray rectangle's start wraps
    'trunc-to-zero': lambda s: s['raw0'][0] == 0 and s['raw0'][2] == 0 and _area(s['core']) > 1 and _area(s['zero']) == 0
    and s['raw2'][0] < 0 and _area(s['recore']) == _area(s['core']),
    'single-pixel-at-origin': lambda s: s['core'] == ((0, 1), (0, 1)) and s['raw0'] == (0, 0, 0, 0),
    'clamped-end': lambda s: _area(s['core']) > 0 and all(e + 1 > HW and o < HW for o, e in _axes(s['raw0'])),
    'inside': lambda s: _area(s['core']) > 1 and all(0 <= o and e + 1 <= HW for o, e in _axes(s['raw2'])),
    'last-pixel': lambda s: s['core'] == ((HW - 1, HW), (HW - 1, HW)),
    # the core starts at 60 (empty) while the zeroed block still has pixels: selected negatives are erased and nothing is re-set
    'zero-block-no-core': lambda s: _area(s['core']) == 0 and _area(s['zero']) > 0 and _area(s['recore']) == 0,
    'zero-size': lambda s: _area(s['core']) == 1 and s['raw0'][0] == s['raw0'][1] and s['raw0'][2] == s['raw0'][3] and s['raw0'][0] > 0,
    'reversed': lambda s: _area(s['core']) == 0 and all(0 <= e < o < HW for o, e in _axes(s['raw0'])),
    'half-ties': lambda s: _area(s['core']) == 4 and all(0 < o and e + 1 < HW for o, e in _axes(s['raw2'])),
    # both ends below -60: clamped to 0 after the wrap, empty, nothing zeroed
    'below-wrap': lambda s: _area(s['core']) == 0 and _area(s['zero']) == 0 and all(e + 1 < -HW for o, e in _axes(s['raw0'])),
    'beyond-end': lambda s: _area(s['core']) == 0 and _area(s['zero']) == 0 and any(o > HW for o, e in _axes(s['raw2'])),
    'far-left': lambda s: _area(s['core']) == 0 and s['raw0'][1] + 1 < -HW and 0 <= s['raw0'][2] and s['raw0'][3] + 1 <= HW,
    'wide-right': lambda s: _area(s['core']) == 0 and s['raw0'][0] > HW and 0 <= s['raw0'][2] and s['raw0'][3] + 1 <= HW,
    # an all-zero box: the pixel at the origin is positive, the gray rectangle's start wraps (nothing zeroed) and the re-set core is
    # the single pixel (1, 1) -- not the positive one
    'all-zero': lambda s: s['core'] == ((0, 1), (0, 1)) and _area(s['zero']) == 0 and s['recore'] == ((1, 2), (1, 2)),
}

# (name, box, branch, positives the oracle gives -- asserted in test_loss_cases.py)
BOXES = [
    ('left-top-wrap', (-10., -6., 8., 4.), 'wrap-empty', 0),
    ('centred-on-origin', (-3., -3., 3., 3.), 'trunc-to-zero', 9),          # pixels 0..2
    ('tiny-on-origin', (-0.4, -0.4, 0.4, 0.4), 'single-pixel-at-origin', 1),
    ('over-right-bottom', (50., 50., 70., 70.), 'clamped-end', 9),          # pixels 57..59
    ('over-right-bottom-frac', (55., 55., 64.9, 64.9), 'clamped-end', 4),
    ('larger-than-grid', (-30., -30., 90., 90.), 'inside', 1369),
    ('whole-grid', (0., 0., 60., 60.), 'inside', 361),
    ('last-pixel', (59., 59., 60., 60.), 'last-pixel', 1),
    ('right-edge-block', (58.5, 0., 61.5, 3.), 'zero-block-no-core', 0),
    ('zero-size', (30., 30., 30., 30.), 'zero-size', 1),
    ('reversed-corners', (40., 40., 20., 20.), 'reversed', 0),
    ('half-ties', (10.5, 10.5, 13.5, 13.5), 'half-ties', 4),
    ('below-wrap', (-70., -70., -62., -62.), 'below-wrap', 0),
    ('beyond-end', (70., 70., 80., 80.), 'beyond-end', 0),
    ('far-left', (-200., 10., -100., 20.), 'far-left', 0),
    ('wide-right', (0., 28., 200., 32.), 'wide-right', 0),
    ('all-zero', (0., 0., 0., 0.), 'all-zero', 1),
]


def fixture_interior_rows():
    """(bbox, vert) rows of the 14-row ``labels`` fixture whose centre and gray rectangles lie inside the grid on both axes."""
    g = np.load(os.path.join(_GOLDEN, 'labels.npz'), allow_pickle=False)
    keep = [i for i in range(g['bbox'].shape[0]) if BRANCH['inside'](spans(g['bbox'][i]))]
    return g['bbox'][keep].astype(np.float32), g['vert'][keep].astype(np.float32)


def box_table():
    """[B,4] float32: the named rows, then the interior rows of the ``labels`` fixture."""
    return np.concatenate([np.asarray([b for _, b, _, _ in BOXES], np.float32), fixture_interior_rows()[0]])


# ------------------------------------------------------------------------------------------------ landmarks
# (x0, y0, ..., x3, y3), all in range after int(v + 0.5) for every kind; rows and columns 0, 1, 2, 57, 58, 59 all occur, values exactly on
# .5 (int(v + 0.5) goes up: 0.5 -> 1, 56.5 -> 57, 58.5 -> 59), -0.5 and -1.25 (int() truncates toward zero: pixel 0), two landmarks of
# one patch on one pixel (rows 3, 6), landmarks inside and outside the boxes they are paired with (the tables' lengths are coprime)
LANDMARKS = np.asarray([
    (0., 0., 59., 0., 59., 59., 0., 59.),                  # the four corners: empty zero-block on both axes / clipped at 59
    (1., 1., 58., 1., 58., 58., 1., 58.),                  # rows / columns 1 (empty block by wrap) and 58 (clipped)
    (2., 2., 57., 2., 57., 57., 2., 57.),                  # 2 and 57: the first / last full 5 x 5 blocks
    (30., 0., 30., 0., 0., 30., 59., 30.),                 # one axis at the border; landmarks 0 and 1 on the same pixel
    (0.5, 1.5, 56.5, 57.5, 58.5, 0.5, 1.5, 58.5),          # exactly on .5 -> (1,2) (57,58) (59,1) (2,59)
    (-0.5, -0.5, -1.25, 30., 30., -1.25, 59.49, 59.49),    # negative values that still round to pixel 0; just below the clamp
    (12., 12., 12., 12., 12., 12., 12., 12.),              # all four on one pixel (inside the half-ties box)
    (1., 30., 58., 30., 30., 1., 30., 58.),                # mixed: one axis interior, the other at 1 / 58
    (2., 57., 57., 2., 0., 1., 59., 58.),
    (20.25, 21.75, 40.5, 22.25, 40.75, 30.5, 19.5, 29.75),
    (45., 10., 10., 45., 31., 29., 29., 31.),
], np.float32)
# DenseBoxLMLOC only (init_lm_heatmap_pn clamps to 59; the other kinds would index row / column 60): values in [59.5, 60)
LANDMARKS_CLAMPED = np.asarray([
    (59.5, 10., 10., 59.75, 59.99, 59.5, 59.5, 0.),
    (59.75, 59.75, 1., 59.5, 59.5, 2., 30., 59.99),
], np.float32)


def landmark_table(kind):
    return np.concatenate([LANDMARKS, LANDMARKS_CLAMPED]) if kind == 'DenseBoxLMLOC' else LANDMARKS.copy()


def lm_pixels(vertices, clamp):
    """[N,4,2] (x, y) as int(v + float32(0.5)), with ``clamp`` then min(., 59) -- init_lm_heatmap / init_lm_heatmap_pn."""
    v = np.asarray(vertices, np.float32).reshape(-1, 4, 2)
    p = np.trunc(v + np.float32(0.5)).astype(np.int64)
    return np.minimum(p, HW - 1) if clamp else p


LABEL_CYCLE = (1., 2., -1., 0., 1.)       # period 5; 28 boxes, 11 / 13 landmark rows: pairwise coprime, so the pairings shift every cycle


def make_batch(kind, n, seed=0, boxes=None):
    """n patches cycling the box table, the landmark table of ``kind`` and LABEL_CYCLE, with randn network outputs.
    Returns (outs [list of float32 arrays in the order of ``kind``], bbox [n,4], vert [n,8], lab [n,1])."""
    bt = box_table() if boxes is None else np.asarray(boxes, np.float32)
    lt = landmark_table(kind)
    idx = np.arange(n)
    bbox, vert = bt[idx % len(bt)].copy(), lt[idx % len(lt)].copy()
    lab = np.asarray(LABEL_CYCLE, np.float32)[idx % len(LABEL_CYCLE)].reshape(n, 1)
    rs = np.random.RandomState(seed)
    outs = [rs.randn(*sh).astype(np.float32) for sh in out_shapes(kind, n)]
    return outs, bbox, vert, lab


def out_shapes(kind, n):
    if kind == 'DenseBox':
        return [(n, 1, HW, HW), (n, 4, HW, HW)]
    if kind == 'DenseBoxLM':
        return [(n, 1, HW, HW), (n, 4, HW, HW), (n, 4, HW, HW), (n, 1, HW, HW)]
    return [(n, 1, HW, HW), (n, 1, HW, HW), (n, 4, HW, HW), (n, 4, HW, HW), (n, 8, HW, HW)]


def split_outs(kind, outs):
    """dict score / loc / lm / rf / lmloc (None where the kind has none) from the kind's output order."""
    if kind == 'DenseBox':
        return dict(score=outs[0], loc=outs[1], lm=None, rf=None, lmloc=None)
    if kind == 'DenseBoxLM':
        return dict(score=outs[0], loc=outs[1], lm=outs[2], rf=outs[3], lmloc=None)
    return dict(score=outs[0], rf=outs[1], loc=outs[2], lm=outs[3], lmloc=outs[4])


def draw_rand_neg(rs, n, half):
    return np.stack([rs.choice(NPIX, half, replace=False) for _ in range(n)]).astype(np.int64) if half else np.zeros((n, 0), np.int64)


def draw_lm_rand_neg(rs, n):
    return rs.randint(0, NPIX, size=(4, n, 1)).astype(np.int64)


def p_for_half(half, batch):
    """A positive_num_global that makes neg_counts(P, batch) give ``half`` (DenseBox.py:2074, :2081)."""
    P = 2 * half * batch
    assert O.neg_counts(P, batch)[1] == half
    return P


# ------------------------------------------------------------------------------------------------ selection rule
def neg_loss(out, gt):
    """float32 (out - gt)**2 * (1 - gt), flattened per patch -- what the kernel and hard_negatives() rank (DenseBox.py:2077)."""
    out, gt = np.asarray(out, np.float32), np.asarray(gt, np.float32)
    d = out - gt
    return ((d * d) * (np.float32(1.0) - gt)).reshape(out.shape[0], -1)


def tie_order(neg, k):
    """The documented rule of both top-K paths: indices sorted by (loss descending, index ascending), first k.  [N,3600] -> [N,k] int64."""
    neg = np.asarray(neg)
    out = np.zeros((neg.shape[0], k), np.int64)
    for r in range(neg.shape[0]):
        out[r] = np.lexsort((np.arange(neg.shape[1]), -neg[r].astype(np.float64)))[:k]
    return out


TIE_VALUES = np.asarray([0., 0.25, -0.25, 0.5, -0.5, 1.], np.float32)


def tie_batch(n=8, seed=77, constant_patch=None):
    """A DenseBoxLMLOC batch over the first rows of the table whose score and landmark maps are drawn from TIE_VALUES: a freshly
    initialised or saturated map, full of exactly equal losses.  ``constant_patch``: that patch's score and landmark maps are all 0.5."""
    outs, bbox, vert, lab = make_batch('DenseBoxLMLOC', n, seed=seed)
    rs = np.random.RandomState(seed)
    outs[0] = TIE_VALUES[rs.randint(0, len(TIE_VALUES), size=outs[0].shape)]
    outs[3] = TIE_VALUES[rs.randint(0, len(TIE_VALUES), size=outs[3].shape)]
    if constant_patch is not None:
        outs[0][constant_patch] = 0.5
        outs[3][constant_patch] = 0.5
    return outs, bbox, vert, lab


def hard_lists(kind, outs, bbox, vert, lab, half):
    """(hard [N,half], lm_hard [4,N,1] or None) by tie_order from the oracle's own label maps."""
    pn = kind == 'DenseBoxLMLOC'
    o = split_outs(kind, outs)
    gt = O.init_score_map(bbox, lab if pn else None)
    hard = tie_order(neg_loss(o['score'], gt), half)
    if kind == 'DenseBox':
        return hard, None
    heat = O.init_lm_heatmap(vert, lab if pn else None)
    lm_hard = np.stack([tie_order(neg_loss(o['lm'][:, j:j + 1], heat[:, j:j + 1]), 1) for j in range(4)])
    return hard, lm_hard


# ------------------------------------------------------------------------------------------------ scalar reference
def loss64(res, outs, kind, lambda_loc=3.0, lambda_det=1.0, lambda_lm=0.5, per_patch=False):
    """The loss as the float64 sum of the per-element float32 terms m * (d * d), masks and targets from ``res`` (O.loss_step's result),
    lambdas applied in float64 as loss_step combines them (kind 'DenseBox' has no lambda_det: DenseBox.py:2917).  ``per_patch``: [N]."""
    o = split_outs(kind, [np.asarray(t.detach() if torch.is_tensor(t) else t, np.float32) for t in outs])
    m, gt = res['mask'], res['gt']

    def term(mask, out, tgt):
        d = out - tgt.astype(np.float32)
        t = mask.astype(np.float32) * (d * d)
        assert t.dtype == np.float32
        return t.astype(np.float64).reshape(t.shape[0], -1).sum(axis=1)
    mg = m * gt
    cls, loc = term(m, o['score'], gt), term(mg, o['loc'], res['loc_gt'])
    if kind == 'DenseBox':
        tot = cls + lambda_loc * loc
    else:
        tot = lambda_det * (cls + lambda_loc * loc) + lambda_lm * term(res['lm_mask'], o['lm'], res['heat_gt']) + term(m, o['rf'], gt)
        if kind == 'DenseBoxLMLOC':
            tot = tot + term(mg, o['lmloc'], res['lmloc_gt'])
    return tot if per_patch else float(tot.sum())


def grad_masks(kind, res):
    """name -> the {0,1} map outside which dL/d(out) must be exactly 0, broadcastable to the output."""
    m = res['mask']
    mg = m * res['gt']
    if kind == 'DenseBox':
        return dict(score=m, loc=mg)
    d = dict(score=m, loc=mg, lm=res['lm_mask'], rf=m)
    if kind == 'DenseBoxLMLOC':
        d['lmloc'] = mg
    return d


# ------------------------------------------------------------------------------------------------ sensitivity variants
def score_map_variant(bbox, end_inclusive=True, wrap=True):
    """init_score_map with two switches: ``end_inclusive`` False reads the stop ``ey + 1`` as ``ey``; ``wrap`` False clamps a negative
    start / stop to 0 where python wraps it.  (True, True) is the oracle's map -- asserted in test_loss_cases.py."""
    def sl(a, b):
        if wrap:
            return O._py_slice(a, b)
        a, b = min(max(a, 0), HW), min(max(b, 0), HW)
        return a, max(a, b)
    bbox = np.asarray(bbox, np.float32)
    m = np.zeros((bbox.shape[0], 1, HW, HW), np.float32)
    for i in range(bbox.shape[0]):
        ox, ex = O._rect(bbox[i, 0], bbox[i, 2], 0.3, 0.0)
        oy, ey = O._rect(bbox[i, 1], bbox[i, 3], 0.3, 0.0)
        inc = 1 if end_inclusive else 0
        (ya, yb), (xa, xb) = sl(oy, ey + inc), sl(ox, ex + inc)
        m[i, 0, ya:yb, xa:xb] = 1.0
    return m
