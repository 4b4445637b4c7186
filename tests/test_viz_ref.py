"""CPU-side checks of the overlay's text and font, which the library compiles for the host as well (dbx_overlay_font,
dbx_overlay_label), and of the NumPy restatement itself (tests/viz_ref.py) on hand-computed 12 x 12 cases."""
import ctypes as C
import os
import sys

import numpy as np

from densebox_amd import _lib, viz

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import viz_ref as V  # noqa: E402

NAN, INF = float('nan'), float('inf')


def test_font_equals_the_restatements_table():
    got = viz.font()
    assert got.shape == (14, 8) and got.dtype == np.uint8
    assert np.array_equal(got, V.FONT)
    assert not (got & 0xE0).any() and not got[:, 7].any() and not got[13].any()          # 5 x 7 in the 6 x 8 cell; the space is empty
    assert len({bytes(g) for g in got}) == 14


def _labels(values):
    L = _lib.lib()
    buf = C.create_string_buffer(32)
    bad = []
    for v in values:
        for tid in (-1, 0, 2147483647):
            n = L.dbx_overlay_label(float(v), tid, buf, 32)
            got = buf.value.decode()
            if n != len(got) or n > 21 or got != V.label(v, tid):
                bad.append((v, tid, got, V.label(v, tid)))
    return bad


def test_label_equals_percent_3f_on_seeded_float32_values():
    rs = np.random.RandomState(5)
    v = (rs.standard_normal(100000) * rs.choice([1e-3, 1.0, 30.0, 400.0], 100000)).astype(np.float32).astype(np.float64)
    assert (np.abs(v) >= 1000).any() and (np.abs(v) < 1e-3).any()
    assert _labels(v) == []


def test_label_on_every_multiple_of_a_two_thousandth_below_one():
    assert _labels([k / 2000 for k in range(2000)]) == []
    assert _labels([-k / 2000 for k in range(2000)]) == []


def test_label_special_values():
    assert _labels([0.0, -0.0, 5e-324, -5e-324, 999.9994, 999.9996, -999.9996, 1000.0, -1000.0, INF, -INF, NAN, 1e300, 0.0005, 0.0015,
                    0.0025, 0.5, 999.9995, 2.0 ** -60, 2.0 ** -64, 2.0 ** -65, 2.0 ** -1000]) == []
    assert viz.label(999.9996) == '1000.000' and viz.label(999.9994) == '999.999'
    assert viz.label(-0.0) == '-0.000' and viz.label(5e-324) == '0.000' and viz.label(0.0) == '0.000'
    assert viz.label(1000.0) == viz.label(INF) == viz.label(NAN) == viz.label(-INF) == '---'
    assert viz.label(0.0005) == '0.001' and viz.label(0.0015) == '0.002' and viz.label(0.0025) == '0.003'      # the binary values, not ties
    assert viz.label(0.5, 0) == '#0 0.500' and viz.label(-999.9996, 2147483647) == '#2147483647 -1000.000'
    assert len(viz.label(-999.9996, 2147483647)) == 21
    assert viz.label(0.25, -1) == viz.label(0.25, None) == '0.250'
    assert _lib.lib().dbx_overlay_label(0.5, 1, C.create_string_buffer(21), 21) == -1                           # 21 characters and the NUL
    assert _lib.lib().dbx_overlay_label(0.5, 1, None, 32) == -1 and b'overlay_label' in _lib.lib().dbx_last_error()
    assert _lib.lib().dbx_overlay_font(None) == -1


def _art(img, legend):
    return [''.join(legend[int(v)] for v in row) for row in img[:, :, 0]]


PLAIN = dict(box_color=(1,), text_color=(2,), mark_color=(3,), radius=-1, font_scale=0)


def _outline(t):
    d = np.array([[3.2, 1.6, 7.5, 7.4, 0.5]])                    # I(): 3, 2, 8, 7
    return _art(V.draw(np.zeros((12, 12, 1), np.uint8), d, [0], style=dict(PLAIN, thickness=t)), '.#')


def test_restatement_outline_thickness_1():
    assert _outline(1) == ['............',
                           '............',
                           '...######...',
                           '...#....#...',
                           '...#....#...',
                           '...#....#...',
                           '...#....#...',
                           '...######...',
                           '............',
                           '............',
                           '............',
                           '............']


def test_restatement_outline_thickness_2():
    assert _outline(2) == ['............',
                           '..########..',
                           '..########..',
                           '..##....##..',
                           '..##....##..',
                           '..##....##..',
                           '..##....##..',
                           '..########..',
                           '..########..',
                           '............',
                           '............',
                           '............']


def test_restatement_outline_thickness_3():
    assert _outline(3) == ['............',
                           '..########..',
                           '..########..',
                           '..########..',
                           '..###..###..',
                           '..###..###..',
                           '..########..',
                           '..########..',
                           '..########..',
                           '............',
                           '............',
                           '............']


def test_restatement_disc_of_radius_2():
    d = np.full((1, 13), NAN)
    d[0, :5] = [100, 100, 120, 110, 0.5]                         # the box is outside the frame
    d[0, 5:7] = [5.9, 6.2]                                       # T(): (5, 6); the other three landmarks are NaN and skipped
    assert _art(V.draw(np.zeros((12, 12, 1), np.uint8), d, [0], style=dict(PLAIN, thickness=1, radius=2)), '.#@o') == [
        '............',
        '............',
        '............',
        '............',
        '.....o......',
        '....ooo.....',
        '...ooooo....',
        '....ooo.....',
        '.....o......',
        '............',
        '............',
        '............']


def test_restatement_glyph_at_scale_1():
    d = np.array([[0.0, 11.0, 0.0, 11.0, 7.0]])                  # "7.000": the 7 at x 2..6, y 1..7, the point at x 9..10, y 6..7
    assert _art(V.draw(np.zeros((12, 12, 1), np.uint8), d, [0], style=dict(PLAIN, thickness=1, font_scale=1)), '.BT') == [
        'BBBBBBBBBBBB',
        'BBTTTTTBBBBB',
        'BBBBBBTBBBBB',
        'BBBBBTBBBBBB',
        'BBBBTBBBBBBB',
        'BBBTBBBBBBBB',
        'BBBTBBBBBTTB',
        'BBBTBBBBBTTB',
        'BBBBBBBBBBBB',
        'BBBBBBBBBBBB',
        'BBBBBBBBBBBB',
        'BBBBBBBBBBBB']


def test_restatement_glyph_at_scale_2():
    d = np.array([[0.0, 18.0, 0.0, 18.0, 7.0]])                  # the 7 in 2 x 2 blocks from (2, 0); the background from y = -3 to 18
    assert _art(V.draw(np.zeros((12, 12, 1), np.uint8), d, [0], style=dict(PLAIN, thickness=1, font_scale=2)), '.BT') == [
        'BBTTTTTTTTTT',
        'BBTTTTTTTTTT',
        'BBBBBBBBBBTT',
        'BBBBBBBBBBTT',
        'BBBBBBBBTTBB',
        'BBBBBBBBTTBB',
        'BBBBBBTTBBBB',
        'BBBBBBTTBBBB',
        'BBBBTTBBBBBB',
        'BBBBTTBBBBBB',
        'BBBBTTBBBBBB',
        'BBBBTTBBBBBB']


def test_restatement_paints_later_rows_over_earlier_and_counts_coverage():
    d = np.array([[2.0, 2.0, 6.0, 6.0, 0.1], [4.0, 4.0, 9.0, 9.0, 0.2]])
    count = np.zeros((12, 12), np.int64)
    a = V.draw(np.zeros((12, 12, 1), np.uint8), d, [0, 1], style=dict(PLAIN, thickness=1), count=count)
    assert count.max() == 2 and count[4, 6] == 2 and count[6, 4] == 2 and count[0, 0] == 0
    b = V.draw(np.zeros((12, 12, 1), np.uint8), d, [1, 0, 7, -1], style=dict(PLAIN, thickness=1))                 # (bad entries paint nothing)
    assert np.array_equal(a, b)                                                                                   # one colour: order is invisible
    two = V.draw(np.zeros((12, 12, 3), np.uint8), d[:, [0, 1, 2, 3, 4]], [0, 1], style=dict(PLAIN, box_color=(5, 6), thickness=1))
    assert two[2, 2].tolist() == [5, 6, 0]                                                                        # a short colour is padded with 0
