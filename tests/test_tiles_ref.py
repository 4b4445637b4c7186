"""The NumPy restatement of tiled detection (tests/tiles_ref.py) pinned to hand-computed cases, the partition property of the cores on
a sweep of axes, the scale-1 tile pixels against the frame's own slices, and the non-triviality of the cases the GPU kernel tests run.
No GPU and no library call here: tests/test_tiles_abi.py compares the library with this restatement."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cubic_ref            # noqa: E402
import pyramid_ref as P     # noqa: E402
import tiles_ref as R       # noqa: E402

INF, NAN = float('inf'), float('nan')


@pytest.mark.parametrize('L, S, ov, starts, mids', [
    (50, 64, 16, [0], []),                            # L < S: one padded window
    (64, 64, 16, [0], []),                            # L == S
    (65, 64, 16, [0, 1], [65]),                       # L == S + 1: the second window is shifted inward to 1; midpoint of [1, 64) doubled
    (160, 64, 16, [0, 48, 96], [112, 208]),           # the last stride lands on L - S
    (150, 64, 16, [0, 48, 86], [112, 198]),           # an inward-shifted last window: 96 -> 86
    (130, 64, 0, [0, 64, 66], [128, 194]),            # overlap 0: the boundary of touching windows is their common edge, doubled
    (130, 64, 32, [0, 32, 64, 66], [96, 160, 194]),   # 2 * overlap == src
    (3840, 512, 128, [0, 384, 768, 1152, 1536, 1920, 2304, 2688, 3072, 3328], [896, 1664, 2432, 3200, 3968, 4736, 5504, 6272, 6912]),
])
def test_axis_hand_cases(L, S, ov, starts, mids):
    s, lo, hi = R.axis(L, S, ov)
    assert s == starts
    assert lo == [-INF] + [float(m) for m in mids] and hi == [float(m) for m in mids] + [INF]


def test_plan_hand_case_is_row_major_with_clipped_crops():
    p = R.plan(40, 100, 64, 16, frame=3, scale=0.5)
    assert p.shape == (2,) and p.dtype.itemsize == 64
    assert p[0].tolist() == (3, 0, 0, 64, 64, 40, 0.5, -INF, 100.0, -INF, INF)
    assert p[1].tolist() == (3, 36, 0, 64, 64, 40, 0.5, 100.0, INF, -INF, INF)
    q = R.plan(130, 70, 64, 16)
    assert [(t['x0'], t['y0']) for t in q] == [(0, 0), (6, 0), (0, 48), (6, 48), (0, 66), (6, 66)]      # y outer, x inner
    assert len(R.plan(2160, 3840, 512, 128)) == 60 and len(R.plan(2160, 3840, 256, 128)) == 16 * 29


def test_the_cores_partition_every_axis_and_the_windows_stay_inside():
    for L in range(1, 201):
        for S in (8, 32, 64):
            for ov in (0, 8, S // 2):
                if 2 * ov > S:
                    continue
                starts, lo, hi = R.axis(L, S, ov)
                assert all(0 <= s and s + S <= max(L, S) for s in starts) and starts == sorted(set(starts))
                assert starts[0] == 0 and starts[-1] == max(L - S, 0)
                # every doubled-integer coordinate (and well beyond the axis) lies in exactly one core; the core of a window lies inside it
                c2 = np.arange(-2 * S, 2 * max(L, S) + 2 * S)
                inside = np.array([(l <= c2) & (c2 < h) for l, h in zip(lo, hi)])
                assert (inside.sum(axis=0) == 1).all(), (L, S, ov)
                for i, s in enumerate(starts):
                    assert (lo[i] == -INF or lo[i] >= 2 * s) and (hi[i] == INF or hi[i] <= 2 * (s + S)), (L, S, ov, i)


def test_map_and_ownership_hand_cases():
    t0, t1, t2 = R.plan(64, 160, 64, 16)                            # windows at 0, 48, 96; boundaries 112 and 208 (doubled)
    d = np.array([[10.0, 5.0, 30.0, 15.0, 0.9]])
    assert R.map_rows(d, t1).tolist() == [[58.0, 5.0, 78.0, 15.0, 0.9]]
    half = R.plan(64, 160, 32, 8, scale=0.5)[2]                     # src 32 resized to 64: window at 48, tile pixels are half pixels
    assert (half['x0'], half['scale']) == (48, 0.5) and R.map_rows(d, half).tolist() == [[53.0, 2.5, 63.0, 7.5, 0.9]]
    lm = np.arange(13, dtype=np.float64)[None]
    assert R.map_rows(lm, t1)[0].tolist() == [48, 1, 50, 3, 4, 53, 6, 55, 8, 57, 10, 59, 12]
    # a centre exactly on a core boundary belongs to the HIGHER tile: x1 + x2 = 112
    box = np.array([[50.0, 0.0, 62.0, 10.0, 0.5]])
    assert R.marks(box, t0, R.CORE).tolist() == [0] and R.marks(box, t1, R.CORE).tolist() == [1]
    box[0, 2] = 61.75
    assert R.marks(box, t0, R.CORE).tolist() == [1] and R.marks(box, t1, R.CORE).tolist() == [0]
    # the outer cores are unbounded: a box far outside the frame is owned by the border tile
    far = np.array([[-500.0, -500.0, -400.0, -450.0, 0.5], [900.0, 70.0, 950.0, 90.0, 0.5]])
    assert R.marks(far, t0, R.CORE).tolist() == [1, 0] and R.marks(far, t2, R.CORE).tolist() == [0, 1]
    # a NaN box is not owned under CORE, owned under NONE, and passes through the map
    for col in range(4):
        nb = np.array([[50.0, 0.0, 60.0, 10.0, 0.5]])
        nb[0, col] = NAN
        m = R.map_rows(nb, t1)
        assert np.isnan(m[0, col]) and R.marks(m, t1, R.CORE).tolist() == [0] and R.marks(m, t1, R.NONE).tolist() == [1]
    ns = np.array([[50.0, 0.0, 60.0, 10.0, NAN]])                   # a NaN score is no NaN box
    assert R.marks(ns, t0, R.CORE).tolist() == [1]


def test_stitch_packs_in_tile_then_row_order_and_runs_the_pinned_nms():
    table = np.concatenate([R.plan(64, 100, 64, 16, 0), R.plan(50, 40, 64, 16, 1), R.plan(64, 100, 64, 16, 2)])
    assert table['frame'].tolist() == [0, 0, 1, 2, 2] and table['x0'].tolist() == [0, 36, 0, 0, 36]     # boundary at 100 (doubled)
    rows = np.zeros((5, 3, 5))
    rows[0] = [[10, 10, 30, 20, 0.5], [40, 10, 58, 20, 0.9], [41, 10, 59, 20, 0.9]]          # centres 20, 49, 50: the last is tile 1's
    rows[1] = [[4, 10, 22, 20, 0.9], [30, 30, 50, 40, 0.1], [0, 0, 10, 10, 0.7]]             # source x 40..58 (centre 49: tile 0's), 66.., 36..46 (41: tile 0's)
    rows[2] = [[0, 0, 10, 10, 0.3], [0, 0, 10, 10, 0.3], [20, 20, 30, 30, 0.2]]
    stage, out = R.stitch(rows, [3, 3, 2, 0, -1], table, 3, 3, R.CORE, 0.4)
    assert [k.tolist() for _, k in stage] == [[1, 1, 0], [0, 1, 0], [1, 1], [], []]
    d0, keep0, t0 = out[0]
    assert d0[:, :4].tolist() == [[10, 10, 30, 20], [40, 10, 58, 20], [66, 30, 86, 40]] and t0.tolist() == [0, 0, 1]
    assert keep0 == [1, 0, 2]
    d1, keep1, t1 = out[1]
    assert d1.shape == (2, 5) and keep1 == [1] and t1.tolist() == [2, 2]          # equal scores: the higher row first, it suppresses row 0
    assert out[2][0].shape == (0, 5) and out[2][1] == [] and out[2][2].tolist() == []
    assert R.pairs_and_prefix(stage, out).tolist() == [3, 2, 3, 1, 2, 2, 0, 0, 0, 0, 0, 3, 5, 5]
    _, none = R.stitch(rows, [3, 3, 2, 0, -1], table, 3, 3, R.NONE, 0.4)
    assert [r.shape[0] for r, _, _ in none] == [6, 2, 0]
    assert none[0][1] == P.nms_stable(none[0][0], 0.4) and len(none[0][1]) < 6    # the truncated copies meet their originals in the NMS


def test_scale_1_tiles_are_the_frames_own_slices():
    """the cubic weights at fraction 0 are (0, 2048, 0, 0), so a window resized to its own size is the window: the padded slice"""
    assert cubic_ref.cubic_taps(64, 64)[1].tolist() == [[0, 2048, 0, 0]] * 64
    rs = np.random.RandomState(3)
    for h, w in ((96, 160), (64, 64), (40, 50), (130, 70)):
        frame = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        for tile in R.plan(h, w, 64, 16):
            x0, y0 = int(tile['x0']), int(tile['y0'])
            want = np.full((64, 64, 3), 128, np.uint8)
            want[:min(64, h - y0), :min(64, w - x0)] = frame[y0:y0 + 64, x0:x0 + 64]
            assert R.tile_pixels(frame, tile, 64, cubic_ref).tobytes() == want.tobytes(), (h, w, x0, y0)
        assert (h, w) != (40, 50) or (R.tile_pixels(frame, R.plan(h, w, 64, 16)[0], 64, cubic_ref)[40:] == 128).all()


def test_core_hits_prunes_by_core_not_by_window():
    table = R.plan(64, 160, 64, 16)                                  # cores [-inf, 56), [56, 104), [104, inf)
    assert R.core_hits(table, [(0, 0, 56, 10)]).tolist() == [True, False, False]      # x < 56 only: window 1 covers 48..56, its core does not
    assert R.core_hits(table, [(0, 0, 57, 10)]).tolist() == [True, True, False]
    assert R.core_hits(table, [(104, 0, 105, 1)]).tolist() == [False, False, True]
    assert R.core_hits(table, [(60, 0, 61, 1), (150, 0, 160, 5)]).tolist() == [False, True, True]
    assert R.core_hits(table, []).tolist() == [False, False, False]


def test_the_kernel_cases_are_not_trivial_under_the_restatement():
    """what tests/test_hip_tiles.py asserts on the GPU holds for the restatement alone: under CORE rows are dropped and the NMS
    suppresses more, frames have different tile counts, the largest case reaches the 4096-row bound under NONE, and the duplicated
    boundary boxes exist"""
    for case, (per_frame, rpt) in R.CASES.items():
        table = R.case_table(per_frame)
        assert np.bincount(table['frame']).tolist() == list(per_frame)
        for dc in (5, 13):
            rows = R.case_rows(7 * dc + table.shape[0], table, rpt, dc)
            stage, out = R.stitch(rows, None, table, len(per_frame), rpt, R.CORE)
            owned = sum(int(k.sum()) for _, k in stage)
            if table.shape[0] > 1:
                assert 0 < owned < table.shape[0] * rpt and sum(len(k) for _, k, _ in out) < owned
                assert np.isnan(rows[:, :, 4]).any() and np.isnan(rows[:, :, :4]).any()
            _, none = R.stitch(rows, None, table, len(per_frame), rpt, R.NONE)
            assert sum(r.shape[0] for r, _, _ in none) == table.shape[0] * rpt
            assert case != '1x64x64' or none[0][0].shape[0] == 4096
    counts = R.case_counts(14, 9, 10)
    assert counts.min() < 0 and counts.max() > 10 and (counts == 0).any()
