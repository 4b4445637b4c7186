"""The restatement of the zone semantics (tests/zones_ref.py) pinned to hand-computed cases, and the seeded sequences the GPU tests
replay checked, on the restatement alone, to hold enough of every kind of event that no GPU test can pass vacuously.  No GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_ref as TR  # noqa: E402
import zones_ref as Z  # noqa: E402

# A = (0, 0) -> B = (0, 40): cross(B - A, P - A) = -40 * px, so side(P) is true for px <= 0
LINE = (0, 0, 0, 40)
SQUARE = [(0, 0), (40, 0), (40, 40), (0, 40)]


def test_a_step_over_the_line_in_each_direction():
    assert Z.side(LINE, (10, 20)) is False and Z.side(LINE, (-10, 20)) is True and Z.side(LINE, (0, 20)) is True
    # t(Q) = cross((-20, 0), Q - P0) = -20 * (qy - 20): t(A) = 400, t(B) = -400
    assert Z.crossing(LINE, (10, 20), (-10, 20)) == Z.FORWARD
    assert Z.crossing(LINE, (-10, 20), (10, 20)) == Z.BACKWARD
    assert Z.crossing(LINE, (10, 20), (30, 25)) is None and Z.crossing(LINE, (-10, 20), (-30, 25)) is None


def test_landing_on_the_line_and_going_on_is_one_crossing_in_total():
    # a point ON the line has side true.  From the false side the landing is the crossing and leaving to the true side is none ...
    assert Z.crossing(LINE, (10, 20), (0, 20)) == Z.FORWARD and Z.crossing(LINE, (0, 20), (-10, 20)) is None
    # ... from the true side the landing is none and leaving to the false side is the crossing
    assert Z.crossing(LINE, (-10, 20), (0, 20)) is None and Z.crossing(LINE, (0, 20), (10, 20)) == Z.BACKWARD
    # turning back on the line: none from the true side; from the false side the forward crossing is undone by a backward one
    assert Z.crossing(LINE, (0, 20), (-10, 30)) is None
    assert [Z.crossing(LINE, (10, 20), (0, 20)), Z.crossing(LINE, (0, 20), (10, 30))] == [Z.FORWARD, Z.BACKWARD]
    # moving along the line is no crossing
    assert Z.crossing(LINE, (0, 10), (0, 30)) is None


def test_beyond_an_end_point_and_through_the_end_points():
    # the infinite line is crossed at y = 50, beyond B: t(A) = 1000 and t(B) = 200 have one sign
    assert Z.crossing(LINE, (10, 50), (-10, 50)) is None and Z.crossing(LINE, (10, -1), (-10, -1)) is None
    # Half-open: an end point ON the move has t = 0, which counts as t >= 0.  Moving towards -x, t(Q) = -20 * (qy - y): through A
    # t(A) = 0 (true) and t(B) = -800 (false): a crossing; through B t(A) = 800 and t(B) = 0 are both true: none.
    assert Z.crossing(LINE, (10, 0), (-10, 0)) == Z.FORWARD
    assert Z.crossing(LINE, (10, 40), (-10, 40)) is None
    # moving towards +x the signs flip, t(Q) = 20 * (qy - y): through A both are true (0 and 800): none; through B t(A) = -800: a crossing
    assert Z.crossing(LINE, (-10, 0), (10, 0)) is None
    assert Z.crossing(LINE, (-10, 40), (10, 40)) == Z.BACKWARD


def test_points_on_vertices_edges_and_the_ray_through_a_vertex():
    # vertices: only the one with the smallest x and y belongs to the square
    assert [Z.inside(SQUARE, p) for p in SQUARE] == [True, False, False, False]
    # horizontal edges: the one at the smaller y is inside, the other outside; vertical ones: smaller x inside
    assert Z.inside(SQUARE, (20, 0)) and not Z.inside(SQUARE, (20, 40))
    assert Z.inside(SQUARE, (0, 20)) and not Z.inside(SQUARE, (40, 20))
    assert Z.inside(SQUARE, (20, 20)) and not Z.inside(SQUARE, (-1, 20)) and not Z.inside(SQUARE, (20, 41))
    # the ray towards +x from (10, 20) leaves the diamond through its vertex (40, 20): counted once; from (-10, 20) it passes through
    # (0, 20) and (40, 20): an even count
    diamond = [(20, 0), (40, 20), (20, 40), (0, 20)]
    assert Z.inside(diamond, (10, 20)) and not Z.inside(diamond, (-10, 20)) and not Z.inside(diamond, (50, 20))
    assert Z.inside(diamond, (20, 20)) and not Z.inside(diamond, (5, 5))


def test_concave_polygon_in_both_orientations_and_a_bow_tie():
    ell = [(0, 0), (40, 0), (40, 20), (20, 20), (20, 40), (0, 40)]
    for poly in (ell, ell[::-1], ell[2:] + ell[:2]):
        assert Z.inside(poly, (10, 30)) and Z.inside(poly, (30, 10)) and Z.inside(poly, (10, 10))
        assert not Z.inside(poly, (30, 30)) and not Z.inside(poly, (20, 30)) and Z.inside(poly, (19, 30))
    grid = [(x, y) for x in range(-4, 45, 3) for y in range(-4, 45, 3)]
    assert [Z.inside(ell, p) for p in grid] == [Z.inside(ell[::-1], p) for p in grid]
    assert sum(Z.inside(ell, p) for p in grid) > 20
    # (0,0) -> (40,40) -> (40,0) -> (0,40): two triangles that meet in (20, 20); above and below the crossing is outside
    tie = [(0, 0), (40, 40), (40, 0), (0, 40)]
    assert Z.inside(tie, (5, 20)) and Z.inside(tie, (35, 20))
    assert not Z.inside(tie, (20, 5)) and not Z.inside(tie, (20, 35)) and not Z.inside(tie, (45, 20))
    assert [Z.inside(tie, p) for p in grid] == [Z.inside(tie[::-1], p) for p in grid]


def test_anchor_rounding_and_validity():
    # centre x = 10.125 is 40.5 quarter pixels: rounds up, as 10.375 (41.5) does; just below stays
    assert Z.anchor([0.0, 0.0, 20.25, 0.0]) == (41, 0)
    assert Z.anchor([0.0, 0.0, 20.75, 0.0]) == (42, 0)
    assert Z.anchor([0.0, 0.0, 20.24, 0.0]) == (40, 0)
    assert Z.anchor([0.0, 0.0, -20.25, 0.0]) == (-40, 0) and Z.anchor([0.0, 0.0, -20.26, 0.0]) == (-41, 0)
    assert Z.anchor([0.0, 3.0, 0.0, 7.125], 'centre') == (0, 20) and Z.anchor([0.0, 3.0, 0.0, 7.125], 'bottom') == (0, 29)
    assert Z.anchor([0.0, 3.0, 0.0, 7.375], 'bottom') == (0, 30) and Z.anchor([0.0, 100.0, 0.0, -7.125], 'bottom') == (0, -28)
    for bad in (np.nan, np.inf, -np.inf, 1048576.0, -1048576.0):
        for c in range(4):
            box = [1.0, 2.0, 3.0, 4.0]
            box[c] = bad
            assert Z.anchor(box) is None and Z.anchor(box, 'bottom') is None
    assert Z.anchor([1048575.75] * 4) == (4194303, 4194303) and Z.anchor([-1048575.75] * 4, 'bottom') == (-4194303, -4194303)
    assert Z.quarter(10.125) == 41 and Z.quarter(-10.125) == -40 and Z.quarter(10.1) == 40


def _table(T, *slots):
    """a tracker table of T slots; slots: (slot, id, hits, box)"""
    tab = np.zeros(T, TR.TRACK)
    tab['id'] = -1
    for t, tid, hits, box in slots:
        tab[t]['id'], tab[t]['hits'], tab[t]['box'] = tid, hits, box
    return tab


def _box(cx, cy):
    return [cx - 5.0, cy - 5.0, cx + 5.0, cy + 5.0]


CFG = Z.Config(lines=[LINE], regions=[SQUARE])


def _z(z):
    return [int(z[n]) for n in ('owner_id', 'has_prev', 'px', 'py', 'inside')]


def _fields(ev):
    return [tuple(int(e[n]) for n in Z.EVENT.names) for e in ev]


def test_update_walks_a_track_over_a_line_into_a_region_and_out():
    zs = Z.new_state(1, 2)
    hdr = np.array([1, 1, 0, 0], np.int32)
    # frame 0: first seen at (-5, 5) pixels = (-20, 20) quarter pixels: outside, no previous point
    assert Z.update_frame(CFG, zs[0][0], zs[1][0], zs[2][0], hdr, _table(2, (1, 7, 1, _box(-5, 5))), 3) == []
    assert _z(zs[0][0][1]) == [7, 1, -20, 20, 0] and _z(zs[0][0][0]) == [-1, 0, 0, 0, 0]
    # frame 1: to (5, 5) = (20, 20): side true -> false is backward over line 0, then enter region 0
    hdr[0] = 2
    ev = Z.update_frame(CFG, zs[0][0], zs[1][0], zs[2][0], hdr, _table(2, (1, 7, 2, _box(5, 5))), 3)
    assert _fields(ev) == [(3, 7, Z.BACKWARD, 0, 1, 2, 20, 20), (3, 7, Z.ENTER, 0, 1, 2, 20, 20)]
    # frame 2: an invalid anchor: nothing happens, the point is forgotten, the region bit stays
    hdr[0] = 3
    assert Z.update_frame(CFG, zs[0][0], zs[1][0], zs[2][0], hdr, _table(2, (1, 7, 3, [0.0, 0.0, np.inf, 0.0])), 3) == []
    assert _z(zs[0][0][1]) == [7, 0, 20, 20, 1]
    # frame 3: back at (-5, 5): no crossing without a previous point, but the exit
    hdr[0] = 4
    ev = Z.update_frame(CFG, zs[0][0], zs[1][0], zs[2][0], hdr, _table(2, (1, 7, 3, _box(-5, 5))), 3)
    assert _fields(ev) == [(3, 7, Z.EXIT, 0, 3, 3, -20, 20)]
    assert zs[1][0][0].tolist() == [0, 1] and zs[2][0][0].tolist() == [1, 1, 0]


def test_min_hits_three_enters_on_the_first_frame_it_qualifies():
    zs = Z.new_state(1, 1)
    hdr = np.array([0, 1, 0, 0], np.int32)
    for hits in (1, 2):
        hdr[0] += 1
        assert Z.update_frame(CFG, zs[0][0], zs[1][0], zs[2][0], hdr, _table(1, (0, 4, hits, _box(5 * hits - 10, 5))), 0, min_hits=3) == []
        assert _z(zs[0][0][0]) == [-1, 0, 0, 0, 0]                    # no zone state below min_hits
    hdr[0] += 1
    ev = Z.update_frame(CFG, zs[0][0], zs[1][0], zs[2][0], hdr, _table(1, (0, 4, 3, _box(5, 5))), 0, min_hits=3)
    assert _fields(ev) == [(0, 4, Z.ENTER, 0, 2, 3, 20, 20)]                    # the line was stepped over before it qualified: not counted
    assert zs[1][0].sum() == 0


def test_slot_reuse_in_one_frame_ends_the_old_id_inside_and_enters_the_new_one():
    zs = Z.new_state(1, 2)
    hdr = np.array([1, 1, 0, 0], np.int32)
    Z.update_frame(CFG, zs[0][0], zs[1][0], zs[2][0], hdr, _table(2, (0, 5, 1, _box(5, 5)), (1, 6, 1, _box(6, 6))), 0)
    assert zs[2][0][0].tolist() == [2, 0, 2]
    hdr[0] = 2                                                                  # id 5 retired and id 9 born into its slot; id 6 retired, slot free
    ev = Z.update_frame(CFG, zs[0][0], zs[1][0], zs[2][0], hdr, _table(2, (0, 9, 1, _box(7, 7))), 0)
    assert _fields(ev) == [(0, 5, Z.ENDED, 0, 1, 0, 20, 20), (0, 9, Z.ENTER, 0, 1, 1, 28, 28), (0, 6, Z.ENDED, 0, 1, 0, 24, 24)]
    assert zs[2][0][0].tolist() == [3, 2, 1] and _z(zs[0][0][1]) == [-1, 0, 0, 0, 0]
    assert _z(zs[0][0][0]) == [9, 1, 28, 28, 1]


def test_filter_keeps_rows_by_their_anchor():
    cfg = Z.Config(masks=[(0, SQUARE), (1, [(8, 8), (16, 8), (16, 16), (8, 16)])])
    dets = np.array([_box(5, 5) + [0.9], _box(3, 3) + [0.8], _box(20, 5) + [0.7], [np.nan, 0, 1, 1, 0.9], _box(0, 0) + [0.6]])
    # anchors (20, 20): inside; (12, 12): excluded; (80, 20): outside; invalid; (0, 0): on the square's own vertex, inside
    assert Z.filter_keep(cfg, dets, [4, 3, 2, 1, 0, 7, -1]) == [4, 0]
    assert Z.filter_keep(Z.Config(), dets, [4, 3, 7, -1]) == [4, 3, 7, -1]                # no mask: copied as it is
    assert Z.filter_keep(Z.Config(masks=[(1, SQUARE)]), dets, [0, 1, 2, 3, 4]) == [2]    # no include polygon: everything not excluded


def test_arena_overflow():
    e = [Z._event(0, i, 2, 0, 0, 1, (0, 0)) for i in range(5)]
    astate, arena = np.zeros(4, np.int64), []
    Z.append(astate, arena, 2, [e[:1], e[1:3]])
    assert astate.tolist() == [2, 1, 3, 0] and [int(a['track_id']) for a in arena] == [0, 1]
    Z.append(astate, arena, 2, [[], e[3:]])
    assert astate.tolist() == [2, 3, 5, 0] and len(arena) == 2
    astate, arena = np.zeros(4, np.int64), []
    Z.append(astate, arena, 0, [e])
    assert astate.tolist() == [0, 5, 5, 0] and arena == []


def test_the_sequence_set_holds_enough_of_everything():
    tot = {}
    for case in Z.CASES:
        t, snaps, arena = Z.reference(case)
        assert len(snaps) == case[3]
        for k, v in t.items():
            tot[k] = tot.get(k, 0) + v
        assert t['reuse'] >= 5 and t['invalid'] >= 3 and t['fwd'] + t['bwd'] > 0, (case, t)
    print(tot)
    assert tot['fwd'] >= 20 and tot['bwd'] >= 20 and tot['enter'] >= 20 and tot['exit'] >= 20, tot
    assert tot['ended'] >= 5 and tot['reuse'] >= 5 and tot['dropped_rows'] >= 50 and tot['kept_rows'] >= 50 and tot['invalid'] >= 3, tot
    # the small arena overflows, the empty one drops everything
    assert Z.reference(Z.CASES[2])[1][-1]['astate'][1] > 0 and Z.reference(Z.CASES[1])[1][-1]['astate'].tolist()[0] == 0
    # the scene of variant 1 uses every item and 16-vertex polygons
    c = Z.scene(1)
    assert len(c.lines) == 8 and len(c.regions) == 8 and all(len(p) == 16 for p in c.regions) and {r for r, _ in c.masks} == {0, 1}
