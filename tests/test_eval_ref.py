"""The evaluation semantics on the CPU: the NumPy restatement (tests/eval_ref.py) on hand-worked frames; the first-claimant formulation
the kernel uses equals the devkit's sequential walk; average precision on curves computed by hand; the package's host functions
(evaluate.average_precision, precision_recall_at) agree with the restatement."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_ref as R  # noqa: E402

from densebox_amd import evaluate as E  # noqa: E402


@pytest.mark.parametrize('case', R.HAND_CASES, ids=[c[0] for c in R.HAND_CASES])
def test_hand_worked_frames(case):
    _, boxes, keep, gt, ign, thr, status, index, iou = case
    s, j, o, err, tally = R.match_frame(R._rows(boxes), keep, gt, ign, None, thr)
    assert s.tolist() == status and j.tolist() == index and err is None
    assert o.tolist() == iou                                      # exact: small integers, one division
    n_gt = len(gt) - (sum(ign) if ign else 0)
    assert tally.tolist() == [len(keep), status.count(1), status.count(0), status.count(-1), n_gt]


def test_lm_err_of_a_true_positive():
    gt = [[0, 0, 9, 9]]
    rows = R._rows([[0, 0, 9, 9], [1, 0, 10, 9]], dc=13)
    rows[0, 5:13] = R.quad_of(gt)[0] + [3, 4, 0, 0, 0, 5, 6, 8]            # corner distances 5, 0, 5, 10
    s, j, _, err, _ = R.match_frame(rows, [0, 1], gt, None, R.quad_of(gt), 0.5)
    assert s.tolist() == [1, 0] and err[0] == 20.0 / 4.0 / 10.0 and np.isnan(err[1])


def test_keep_entry_out_of_range_is_not_counted():
    s, j, o, _, tally = R.match_frame(R._rows([[0, 0, 9, 9]]), [0, 5, -1], [[0, 0, 9, 9]])
    assert s.tolist() == [1, -2, -2] and j.tolist() == [0, -1, -1] and np.isnan(o[1:]).all() and tally.tolist() == [1, 1, 0, 0, 1]


def _first_claim(dets, keep, gt, ign, thr):
    """the kernel's formulation: jmax of every detection on its own, then per GT the lowest claiming position"""
    k = len(keep)
    best = [R.best_gt(R.iou_row(dets[r, :4], gt)) for r in keep]
    matched = [ov > thr for _, ov in best]
    claim = np.full(len(gt), np.iinfo(np.int32).max, np.int64)
    for i in range(k):
        if matched[i] and not ign[best[i][0]]:
            claim[best[i][0]] = min(claim[best[i][0]], i)
    status = np.zeros(k, np.int32)
    index = np.full(k, -1, np.int32)
    for i in range(k):
        if matched[i]:
            jm = best[i][0]
            index[i] = jm
            status[i] = -1 if ign[jm] else int(claim[jm] == i)
    return status, index, np.array([ov for _, ov in best], np.float64)


def test_first_claimant_equals_the_sequential_walk():
    seen = set()
    for seed in range(200):
        rs = np.random.RandomState(seed)
        n, g = rs.randint(0, 13), rs.randint(0, 7)
        def boxes(m):
            xy = rs.randint(0, 80, size=(m, 2)) / 4.0
            wh = rs.randint(4, 48, size=(m, 2)) / 4.0              # quarter-integer coordinates in a small field: many overlaps, exact ties
            return np.concatenate([xy, xy + wh], axis=1)
        dets = R._rows(boxes(n))
        gt = boxes(g)
        if g and n and seed % 3 == 0:
            gt[rs.randint(g)] = dets[rs.randint(n), :4]            # an exact hit
        if g > 1 and seed % 5 == 0:
            gt[1] = gt[0]                                          # twin GTs: a tie for every detection
        ign = rs.rand(g) < 0.25
        keep = rs.permutation(n)[:rs.randint(0, n + 1)].tolist()
        thr = [0.5, 0.3, 0.0][seed % 3]
        s, j, o, _, _ = R.match_frame(dets, keep, gt, ign, None, thr)
        s2, j2, o2 = _first_claim(dets, keep, gt, ign, thr)
        assert np.array_equal(s, s2) and np.array_equal(j, j2) and np.array_equal(o, o2), seed
        seen |= set(s.tolist())
        if len(keep) > 1:
            dup = [(a, b) for a, b in zip(s.tolist(), j.tolist()) if a == 0 and b >= 0]
            seen |= {'dup'} if dup else set()
    assert seen >= {1, 0, -1, 'dup'}


AP_CASES = [          # (scores, status, n_gt, AP)
    ([0.9, 0.8, 0.7], [1, 1, 1], 3, 1.0),                                   # all TP
    ([0.9, 0.8, 0.7], [1, 0, 1], 2, 0.5 * 1.0 + 0.5 * (2.0 / 3.0)),       # the known 3-detection case: 5/6
    ([0.7, 0.9, 0.8], [1, 1, 0], 2, 0.5 * 1.0 + 0.5 * (2.0 / 3.0)),       # the same records in another arrival order
    ([0.5, 0.5], [0, 1], 1, 0.5),                                           # equal scores: arrival order, FP first
    ([0.5, 0.5], [1, 0], 1, 1.0),                                           # ... TP first
    ([0.9, 0.8, 0.7], [1, -1, 1], 2, 1.0),                                  # an ignored record is dropped
    ([0.9], [1], 4, 0.25),                                                  # recall stops at 1/4
    ([], [], 3, 0.0),
    ([0.9, 0.8], [0, 0], 3, 0.0),
]


@pytest.mark.parametrize('case', range(len(AP_CASES)))
def test_average_precision_on_hand_computed_curves(case):
    scores, status, n_gt, want = AP_CASES[case]
    assert R.average_precision(scores, status, n_gt) == pytest.approx(want, abs=1e-15)
    assert E.average_precision(scores, status, n_gt) == pytest.approx(want, abs=1e-15)


def test_average_precision_without_gt_is_nan():
    assert np.isnan(R.average_precision([0.9], [0], 0)) and np.isnan(E.average_precision([0.9], [0], 0))
    assert np.isnan(E.average_precision([], [], 0))


def test_host_curve_functions_agree_with_the_restatement_on_random_records():
    for seed in range(20):
        rs = np.random.RandomState(seed)
        n = rs.randint(1, 200)
        scores = rs.randint(0, 32, size=n) / 32.0                   # many ties
        status = rs.choice([1, 0, 0, -1], size=n)
        n_gt = int((status == 1).sum()) + rs.randint(0, 5)
        if n_gt == 0:
            continue
        assert E.average_precision(scores, status, n_gt) == pytest.approx(R.average_precision(scores, status, n_gt), rel=1e-12, abs=1e-15)
        t = 0.5
        m = (status != -1) & (scores > t)
        p, r = E.precision_recall_at(scores, status, n_gt, t)
        tp = int((status[m] == 1).sum())
        assert r == tp / n_gt and (np.isnan(p) if m.sum() == 0 else p == tp / m.sum())


def test_precision_recall_at_edges():
    p, r = E.precision_recall_at([0.9, 0.5, 0.4], [1, 0, 1], 2, 0.5)         # strict: the record at 0.5 is out
    assert (p, r) == (1.0, 0.5)
    p, r = E.precision_recall_at([0.9], [1], 0, 0.5)
    assert p == 1.0 and np.isnan(r)
    p, r = E.precision_recall_at([], [], 3, 0.5)
    assert np.isnan(p) and r == 0.0
