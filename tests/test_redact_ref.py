"""The NumPy restatement of dbx_redact_batch (tests/redact_ref.py) pinned to values worked by hand, so that the kernel and dbx_redact_host
are compared with something that is itself checked."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import redact_ref as V  # noqa: E402

NAN = float('nan')
PLAIN = dict(grow=0, grow_pct=0, shape='box')
TRACK = np.dtype([('box', '<f8', (4,)), ('id', '<i4'), ('age', '<i4')])


def _row(box, score=0.5, lm=None):
    r = np.zeros((1, 13 if lm is not None else 5))
    r[0, :4], r[0, 4] = box, score
    if lm is not None:
        r[0, 5:] = lm
    return r


def test_truncating_division():
    assert [V.tdiv(7, 2), V.tdiv(-7, 2), V.tdiv(-400, 100), V.tdiv(-160, 100), V.tdiv(0, 100), V.tdiv(-99, 100)] == [3, -3, -4, -1, 0, 0]
    assert [V.I(26.5), V.I(10.2), V.I(-3.7), V.I(-0.4)] == [27, 10, -3, 0]


def test_constant_frame():
    img = np.full((9, 11, 3), 77, np.uint8)
    row = _row([2, 1, 4, 3])
    for st in (dict(method='pixelate', cell=4), dict(method='pixelate', cell=2), dict(method='blur', radius=3), dict(method='blur', radius=16)):
        assert np.array_equal(V.redact(img, row, [0], style=dict(PLAIN, **st)), img)
    got = V.redact(img, row, [0], style=dict(PLAIN, method='fill', color=(1, 2, 3)))
    want = img.copy()
    want[1:4, 2:5] = (1, 2, 3)
    assert np.array_equal(got, want)


def test_ramp_under_cell_4_with_ragged_last_cells():
    """img[y][x] = 10 y + x on a 5 x 7 frame: the cells are x 0..3 | 4..6 by y 0..3 | 4, of n = 16, 12, 4 and 3 pixels, with sums 264, 240,
    166 and 135: (264 + 8) / 16 = 17, (240 + 6) / 12 = 20 (from 20.5), (166 + 2) / 4 = 42, (135 + 1) / 3 = 45 (from 45.33)"""
    img = (10 * np.arange(5)[:, None] + np.arange(7)[None, :]).astype(np.uint8)[:, :, None]
    st = dict(PLAIN, method='pixelate', cell=4)
    whole = V.redact(img, _row([0, 0, 6, 4]), [0], style=st)[:, :, 0]
    want = np.zeros((5, 7), np.uint8)
    want[:4, :4], want[:4, 4:], want[4, :4], want[4, 4:] = 17, 20, 42, 45
    assert np.array_equal(whole, want)
    part = V.redact(img, _row([3, 3, 4, 4]), [0], style=st)[:, :, 0]              # the pixels of a cell outside the region count in its sum
    want = img[:, :, 0].copy()
    want[3, 3], want[3, 4], want[4, 3], want[4, 4] = 17, 20, 42, 45
    assert np.array_equal(part, want)


def test_bright_dot_under_radius_1():
    """replicated edges give the corner weight 4/9: (4 * 255 + 4) / 9 = 113; its edge neighbours 2/9: 57; the diagonal one 1/9: 28"""
    st = dict(PLAIN, method='blur', radius=1)
    img = np.zeros((5, 5, 1), np.uint8)
    img[0, 0] = 255
    got = V.redact(img, _row([0, 0, 4, 4]), [0], style=st)[:, :, 0]
    want = np.zeros((5, 5), np.uint8)
    want[0, 0], want[0, 1], want[1, 0], want[1, 1] = 113, 57, 57, 28
    assert np.array_equal(got, want)
    img = np.zeros((5, 5, 1), np.uint8)
    img[2, 2] = 255
    got = V.redact(img, _row([0, 0, 4, 4]), [0], style=st)[:, :, 0]
    want = np.zeros((5, 5), np.uint8)
    want[1:4, 1:4] = 28                                                             # (255 + 4) / 9
    assert np.array_equal(got, want)


def test_grow_arithmetic_of_a_box():
    """X1, Y1, X2, Y2 = 10, 21, 30, 27: 21 x 7 pixels; gx = 3 + 21 * 25 / 100 = 3 + 5, gy = 3 + 7 * 25 / 100 = 3 + 1"""
    st = dict(V.STYLE, grow=3, grow_pct=25)
    assert V.box_region([10.2, 20.7, 30.4, 26.5], st) == (2, 38, 17, 31)
    assert V.box_region([30.4, 26.5, 10.2, 20.7], st) == (2, 38, 17, 31)           # inverted
    assert V.box_region([5, 5, 5, 5], dict(V.STYLE, grow=0, grow_pct=99)) == (5, 5, 5, 5)
    assert V.box_region([NAN, 0, 1, 1], st) is None and V.box_region([0, 0, 2.0 ** 30, 1], st) is None
    m = V.mask_of(('box', (2, 38, 17, 31)), 25, 35)
    want = np.zeros((25, 35), bool)
    want[17:25, 2:35] = True
    assert np.array_equal(m, want)


def test_grow_arithmetic_of_quads():
    st = dict(V.STYLE, grow=2, grow_pct=10)
    # axis aligned: S = (80, 96); P_0: d = (-40, -16): G = (40 - 4 - 8, 80 - 1 - 8)
    G = V.quad_vertices([10, 20, 30, 20, 30, 28, 10, 28], st)
    assert G == [(28, 71), (132, 71), (132, 121), (28, 121)]
    yy, xx = np.mgrid[:40, :40]
    assert np.array_equal(V.mask_of(('quad', G), 40, 40), (xx >= 7) & (xx <= 33) & (yy >= 18) & (yy <= 30))     # 28 <= 4x <= 132, 71 <= 4y <= 121
    # a diamond: S = (80, 80); P_0: d = (0, -40): G = (80, 40 - 4 - 8); sgn(0) = 0 adds nothing
    G = V.quad_vertices([20, 10, 30, 20, 20, 30, 10, 20], st)
    assert G == [(80, 28), (132, 80), (80, 132), (28, 80)]
    assert np.array_equal(V.mask_of(('quad', G), 40, 40), abs(xx - 20) + abs(yy - 20) <= 13)                     # |4x - 80| + |4y - 80| <= 52
    # no growth: the quad's own vertices in quarter pixels, I() applied to each landmark
    assert V.quad_vertices([10.5, 20.4, 30, 20, 30, 28, 10, 28], dict(V.STYLE, grow=0, grow_pct=0)) == [(44, 80), (120, 80), (120, 112), (40, 112)]


def test_both_orientations_cover_the_same_pixels():
    st = dict(V.STYLE, grow=1, grow_pct=15)
    lm = [12, 8, 33, 5, 36, 22, 9, 27]
    back = [lm[0], lm[1], lm[6], lm[7], lm[4], lm[5], lm[2], lm[3]]
    a, b = V.mask_of(('quad', V.quad_vertices(lm, st)), 32, 45), V.mask_of(('quad', V.quad_vertices(back, st)), 32, 45)
    assert np.array_equal(a, b) and a.sum() > 300 and not a.all()
    zero = [(0, 0), (8, 8), (16, 16), (24, 24)]                                    # both triangles of zero area: nothing
    assert not V.mask_of(('quad', zero), 10, 10).any()


def test_fallbacks_to_the_box():
    st = dict(V.STYLE, shape='quad', grow=0, grow_pct=0)
    assert V.quad_vertices([0, 0, 10, 10, 10, 0, 0, 10], st) is None               # a bow tie: shoelace 0 - 100 + 100 + 0
    assert V.quad_vertices([0, 0, 2.0 ** 20, 0, 5, 5, 0, 5], st) is None
    assert V.quad_vertices([0, 0, 2.0 ** 20 - 1, 0, 5, 5, 0, 5], st) is not None
    assert V.quad_vertices([0, 0, NAN, 0, 5, 5, 0, 5], st) is None
    assert V.quad_vertices([4, 4] * 4, st) is None
    row = _row([0, 0, 10, 10], lm=[0, 0, 10, 10, 10, 0, 0, 10])
    assert V.regions(row, [0], None, st) == [('box', (0, 10, 0, 10))]
    row = _row([0, 0, 10, 10], lm=[0, 0, 10, 0, 10, 10, 0, 10])
    assert V.regions(row, [0], None, st) == [('quad', [(0, 0), (40, 0), (40, 40), (0, 40)])]
    assert V.regions(row, [0], None, dict(st, shape='box')) == [('box', (0, 10, 0, 10))]
    assert V.regions(row, [0], None, dict(st, shape=None))[0][0] == 'quad' and V.regions(row[:, :5], [0], None, dict(st, shape=None))[0][0] == 'box'
    assert V.regions(_row([NAN, 0, 10, 10], lm=[0, 0, 10, 0, 10, 10, 0, 10]), [0], None, st) == []     # no usable box: no region at all


def test_scores_and_keep_entries():
    st = dict(PLAIN, min_score=0.3)
    rows = np.array([[1, 1, 2, 2, NAN], [4, 4, 5, 5, 0.29], [7, 7, 8, 8, 0.3]])
    assert V.regions(rows, [0, 1, 2], None, dict(V.STYLE, **st)) == [('box', (1, 2, 1, 2)), ('box', (7, 8, 7, 8))]
    assert V.regions(rows, [-1, 3, 2], None, dict(V.STYLE, **st)) == [('box', (7, 8, 7, 8))]
    img = np.arange(100, dtype=np.uint8).reshape(10, 10, 1)
    count = np.zeros((10, 10), np.int64)
    got = V.redact(img, rows, [0, 0, 1], style=dict(st, method='fill', color=(255,)), count=count)
    assert count[1:3, 1:3].tolist() == [[2, 2], [2, 2]] and count.sum() == 8
    want = img.copy()
    want[1:3, 1:3] = 255
    assert np.array_equal(got, want)


def test_coasting_tracks():
    t = np.zeros(5, TRACK)
    t['id'] = [1, 2, 3, 4, -1]
    t['age'] = [3, 4, 0, 1, 1]
    t['box'] = [[1, 1, 2, 2], [4, 4, 5, 5], [7, 7, 8, 8], [NAN, 0, 1, 1], [0, 0, 9, 9]]
    st = dict(V.STYLE, grow=0, grow_pct=0, coast=3)
    none = np.zeros((0, 13))
    assert V.regions(none, [], t, st) == [('box', (1, 2, 1, 2))]                   # age = coast; coast + 1, 0, an unusable box, a free slot: none
    assert V.regions(none, [], t, dict(st, coast=4)) == [('box', (1, 2, 1, 2)), ('box', (4, 5, 4, 5))]
    assert V.regions(none, [], t, dict(st, coast=0)) == [] and V.regions(none, [], None, st) == []
    assert V.regions(none, [], t, dict(st, shape='quad'))[0][0] == 'box'           # tracks are always boxes
