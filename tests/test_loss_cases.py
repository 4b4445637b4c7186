"""Premises of the fused-loss edge cases (tests/loss_cases.py), asserted from the reference alone -- oracle/densebox_oracle.py -- before
tests/test_hip_loss_cases.py launches anything: every named branch of the slice arithmetic is hit by its row, the host's positive count
is the oracle's on the whole table, the tie inputs have the ties they claim, and the tables tell the right reading of the reference's
two easily misread steps (the inclusive end, python's wrap of a negative start) from the wrong one."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_cases as L                                  # noqa: E402
import densebox_amd.labels as LB                        # noqa: E402
from oracle import densebox_oracle as O                 # noqa: E402


@pytest.mark.parametrize('name,box,branch,count', L.BOXES, ids=[b[0] for b in L.BOXES])
def test_box_row_hits_its_branch_and_has_the_stated_positives(name, box, branch, count):
    s = L.spans(box)
    assert L.BRANCH[branch](s), (name, s)
    gt = O.init_score_map(np.asarray([box], np.float32))
    assert int(gt.sum()) == count == (s['core'][0][1] - s['core'][0][0]) * (s['core'][1][1] - s['core'][1][0])


def test_stated_pixel_ranges_and_the_zeroed_block_without_a_core():
    def ones(box):
        ys, xs = np.nonzero(O.init_score_map(np.asarray([box], np.float32))[0, 0])
        return (int(ys.min()), int(ys.max()), int(xs.min()), int(xs.max()))
    assert ones((-3., -3., 3., 3.)) == (0, 2, 0, 2)
    assert ones((50., 50., 70., 70.)) == (57, 59, 57, 59)
    assert ones((55., 55., 64.9, 64.9)) == (58, 59, 58, 59)
    assert ones((-30., -30., 90., 90.)) == (12, 48, 12, 48)
    assert ones((59., 59., 60., 60.)) == (59, 59, 59, 59)
    # (58.5, 0, 61.5, 3): 10 pixels are zeroed (rows 0..4 x columns 58, 59), none re-set; (-10, -6, 8, 4): nothing is touched at all
    m = np.ones((2, 1, 60, 60), np.float32)
    O.mask_gray_zone_cls(m, np.asarray([(58.5, 0., 61.5, 3.), (-10., -6., 8., 4.)], np.float32))
    assert int((m[0] == 0).sum()) == 10 and not m[0, 0, :5, 58:].any() and m[1].all()
    # the all-zero box: positive pixel (0, 0), nothing zeroed, the re-set "core" is pixel (1, 1)
    m = np.zeros((1, 1, 60, 60), np.float32)
    O.mask_gray_zone_cls(m, np.zeros((1, 4), np.float32))
    assert np.argwhere(m[0, 0]).tolist() == [[1, 1]]


def test_interior_fixture_rows_are_in_the_table():
    bb, vt = L.fixture_interior_rows()
    assert len(bb) >= 8 and len(L.box_table()) == len(L.BOXES) + len(bb)
    # pairwise coprime periods: the pairing of box, landmark row and label shifts with every cycle of make_batch
    for kind in L.KINDS:
        a, b, c = len(L.box_table()), len(L.landmark_table(kind)), len(L.LABEL_CYCLE)
        assert np.gcd(a, b) == 1 and np.gcd(a, c) == 1 and np.gcd(b, c) == 1, (kind, a, b, c)


def test_positive_count_equals_the_oracle_on_the_whole_table():
    bt = L.box_table()
    n = len(bt)
    lab = np.asarray(L.LABEL_CYCLE + (2., 0.), np.float32)[np.arange(n) % 7].reshape(n, 1)
    for labels in (None, lab):
        want = O.init_score_map(bt, labels).sum(axis=(1, 2, 3)).astype(np.int64)
        assert np.array_equal(LB.positive_count(bt, labels), want)
        assert np.array_equal(LB.positive_count(torch.from_numpy(bt), None if labels is None else torch.from_numpy(labels)), want)
    assert (lab == 0).any() and int(O.init_score_map(bt, lab).sum()) < int(O.init_score_map(bt).sum())


def test_landmark_table_covers_the_border_rows_and_columns():
    for kind in L.KINDS:
        clamp = kind == 'DenseBoxLMLOC'
        p = L.lm_pixels(L.landmark_table(kind), clamp)
        assert p.min() >= 0 and p.max() <= 59                              # in range after the kind's rounding (and clamp)
        for v in (0, 1, 2, 57, 58, 59):
            assert (p[..., 0] == v).any() and (p[..., 1] == v).any(), (kind, v)
        heat = O.init_lm_heatmap(L.landmark_table(kind), np.ones((len(p), 1), np.float32) if clamp else None)
        ys, xs = np.nonzero(heat.reshape(-1, 60, 60))[1:]
        assert np.array_equal(np.stack([xs, ys], 1).reshape(-1, 4, 2), p)   # lm_pixels restates the oracle's rounding
    raw = L.LANDMARKS
    assert ((raw % 1) == 0.5).any() and (raw < 0).any()
    assert ((L.LANDMARKS_CLAMPED >= 59.5) & (L.LANDMARKS_CLAMPED < 60)).any() and not ((raw + np.float32(0.5)) >= 60).any()
    with pytest.raises(IndexError):                                         # why those rows are DenseBoxLMLOC's only
        O.init_lm_heatmap(L.LANDMARKS_CLAMPED)
    p = L.lm_pixels(raw, False)
    assert any(len({tuple(q) for q in row}) < 4 for row in p.tolist())      # two landmarks of one patch on one pixel
    # empty zero-block by wrap at rows / columns 0 and 1, clipped at 58 and 59, full from 2 to 57
    assert [O._py_slice(v - 2, v + 3) for v in (0, 1, 2, 57, 58, 59)] == [(58, 58), (59, 59), (0, 5), (55, 60), (56, 60), (57, 60)]
    m = np.ones((1, 1, 60, 60), np.float32)
    O.mask_gray_zone_lm(m, np.asarray([[0, 0, 1, 30]]))
    assert m.all()                                                          # row 1: the 5 x 5 block is empty, only the centre is (re-)set
    # inside and outside the box a landmark is paired with, somewhere in a 64-patch batch
    _, bbox, vert, _ = L.make_batch('DenseBoxLM', 64)
    x, y = vert[:, 0::2], vert[:, 1::2]
    inside = (x >= bbox[:, 0:1]) & (x <= bbox[:, 2:3]) & (y >= bbox[:, 1:2]) & (y <= bbox[:, 3:4])
    assert inside.any() and (~inside).any()


def test_check_landmarks_refuses_what_the_kernel_must_not_index():
    ok = L.landmark_table('DenseBoxLMLOC')
    LB.check_landmarks(ok, np.ones((len(ok), 1), np.float32), clamp=True)
    LB.check_landmarks(L.LANDMARKS)
    v = L.LANDMARKS[:3].copy()
    v[1, 2] = 59.5                                                          # x rounds to 60
    with pytest.raises(IndexError, match='landmark index 60 is out of bounds for dimension with size 60'):
        LB.check_landmarks(v)
    LB.check_landmarks(v, np.ones((3, 1), np.float32), clamp=True)          # clamped to 59
    v[1, 2], v[2, 5] = 30., -3.                                             # int(-2.5) = -2: the reference would wrap it
    for lab, clamp in ((None, False), (np.ones((3, 1), np.float32), True), (torch.ones(3, 1), True)):
        with pytest.raises(IndexError, match='landmark index -2 is out of bounds'):
            LB.check_landmarks(torch.from_numpy(v) if torch.is_tensor(lab) else v, lab, clamp=clamp)
    LB.check_landmarks(v, np.asarray([[1.], [1.], [0.]], np.float32), clamp=True)     # the patch is not a valid one
    v[2, 5] = -1.49                                                         # int(-0.99) = 0
    LB.check_landmarks(v)


@pytest.mark.parametrize('k', [1, 11, 47, 48, 49, 130])
def test_tie_inputs_have_ties_across_the_cut(k):
    """Of the K selected losses at least half are shared with an unselected pixel of equal loss (in every patch)."""
    outs, bbox, vert, lab = L.tie_batch()
    gt = O.init_score_map(bbox, lab)
    neg = L.neg_loss(outs[0], gt)
    sel = L.tie_order(neg, k)
    for r in range(neg.shape[0]):
        rest = np.ones(L.NPIX, bool)
        rest[sel[r]] = False
        shared = np.isin(neg[r, sel[r]], neg[r, rest])
        assert 2 * int(shared.sum()) >= k, (r, k, int(shared.sum()))
        v = neg[r, sel[r]]
        assert (np.diff(v) <= 0).all() and all(a < b for a, b, e in zip(sel[r], sel[r, 1:], np.diff(v) == 0) if e)


def test_tie_order_is_the_documented_rule():
    neg = np.asarray([[1., 3., 3., 0., 3., 2., 0.]], np.float32)
    assert L.tie_order(neg, 7).tolist() == [[1, 2, 4, 5, 0, 3, 6]]
    rs = np.random.RandomState(0)
    cont = rs.rand(3, 3600).astype(np.float32)                              # no ties: the rule is torch.topk's order
    assert np.array_equal(L.tie_order(cont, 50), torch.topk(torch.from_numpy(cont), 50, dim=1).indices.numpy())


def test_variant_equals_the_oracle_and_both_misreadings_show():
    bt = L.box_table()
    right = O.init_score_map(bt)
    assert np.array_equal(L.score_map_variant(bt), right)
    names = [b[0] for b in L.BOXES]
    by_end = L.score_map_variant(bt, end_inclusive=False)
    by_clamp = L.score_map_variant(bt, wrap=False)
    differs = lambda a, row: not np.array_equal(a[names.index(row)], right[names.index(row)])   # noqa: E731
    assert differs(by_end, 'last-pixel') and differs(by_end, 'zero-size') and differs(by_end, 'half-ties')
    assert differs(by_clamp, 'left-top-wrap') and not differs(by_clamp, 'below-wrap')
    assert int(by_clamp[names.index('left-top-wrap')].sum()) == 6           # rows 0..1 x columns 0..2 if the start were clamped to 0


def test_loss64_is_the_oracle_loss_to_float32_summation_error():
    for kind in L.KINDS:
        n = 9
        outs, bbox, vert, lab = L.make_batch(kind, n, seed=5)
        rs = np.random.RandomState(1)
        half = O.neg_counts(int(O.init_score_map(bbox, lab if kind == 'DenseBoxLMLOC' else None).sum()), n)[1]
        kw = dict(lambda_loc=2.5, lambda_det=0.7, lambda_lm=0.3)
        res = O.loss_step(kind, tuple(torch.from_numpy(o) for o in outs), bbox, vert, lab, rand_neg=L.draw_rand_neg(rs, n, half),
                          lm_rand_neg=L.draw_lm_rand_neg(rs, n), **kw)
        ref = L.loss64(res, outs, kind, **kw)
        assert abs(float(res['loss']) - ref) <= 2e-6 * ref, kind            # the bar the float32 sum was compared at before
        per = L.loss64(res, outs, kind, per_patch=True, **kw)
        assert per.shape == (n,) and abs(per.sum() - ref) <= 1e-12 * ref
