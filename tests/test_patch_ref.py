"""tests/patch_ref.py, the Python restatement of the patch sampler's plan, against what the reference's own gen_pos_patch /
format_4_vertices / intersect_small returned (tests/golden/patch_plan.npz, recorded by tools/gen_patch_golden.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patch_ref as R                                   # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'patch_plan.npz')


@pytest.fixture(scope='module')
def golden():
    return {k: v for k, v in np.load(GOLDEN).items()}


def test_fixture_populates_every_branch(golden):
    st = golden['pos_status']
    nrand = int(golden['pos_random'])
    assert nrand >= 1500 and len(st) > nrand
    counts = np.bincount(st[:nrand], minlength=4)
    assert counts[0] >= 1000 and counts[1] >= 200, counts          # accepted and rejected by the landmark rule
    hand = np.bincount(st[nrand:], minlength=4)
    assert hand[0] > 0 and hand[1] > 0 and hand[2] >= 4 and hand[3] > 0, hand
    size, verts = golden['pos_size'][nrand:], golden['pos_verts'][nrand:]
    xs, ys = verts[:, 0::2], verts[:, 1::2]
    assert (xs.min(1) == 0).any() and (ys.min(1) == 0).any()       # a plate on each border
    assert (xs.max(1) == size[:, 0] - 1).any() and (ys.max(1) == size[:, 1] - 1).any()
    assert (size.min(1) < 248).any()                               # the source-W/H quirk of the rule
    neg = np.bincount(golden['neg_status'], minlength=7)
    assert neg[0] > 50 and neg[6] > 50 and neg[2] > 0, neg


def test_positive_restatement_equals_the_reference(golden):
    bad = []
    for i in range(len(golden['pos_status'])):
        W, H = (int(v) for v in golden['pos_size'][i])
        st, win, lab = R.positive(W, H, golden['pos_verts'][i], float(golden['pos_draws'][i][0]), float(golden['pos_draws'][i][1]))
        ok = st == golden['pos_status'][i]
        if ok and st == R.ACCEPTED:
            ok = lab == golden['pos_labels'][i].tolist() and (win[3] - win[1], win[2] - win[0]) == tuple(golden['pos_shape'][i])
            ok = ok and 0 <= win[0] and 0 <= win[1] and win[2] <= W and win[3] <= H
        if not ok:
            bad.append(i)
    assert not bad, bad[:10]


def test_negative_restatement_equals_the_reference(golden):
    bad = []
    for i in range(len(golden['neg_status'])):
        W, H = (int(v) for v in golden['neg_size'][i])
        cx, cy = (int(v) for v in golden['neg_centre'][i])
        st, win, _ = R.negative(W, H, golden['neg_plates'][i][:golden['neg_nplates'][i]], float(cx), float(cy), int(golden['neg_th'][i]))
        if st != golden['neg_status'][i] or (st == 0 and win != (cx - 120, cy - 120, cx + 120, cy + 120)):
            bad.append(i)
    assert not bad, bad[:10]


def test_vertex_outside_its_frame_is_refused_before_any_geometry():
    assert R.positive(640, 480, [-1, 200, 60, 200, 60, 230, 0, 230], 0.0, 0.0)[0] == R.OUTSIDE
    assert R.positive(640, 480, [0, 200, 640, 200, 60, 230, 0, 230], 0.0, 0.0)[0] == R.OUTSIDE
    assert R.positive(640, 480, [0, 200, 60, 200, 60, 480, 0, 230], 0.0, 0.0)[0] == R.OUTSIDE


def test_plan_scan_and_capacity():
    sizes = [(480, 640)]
    plates = [[0, 300, 200, 360, 200, 360, 230, 300, 230], [0, 0, 0, 5, 0, 5, 5, 0, 5]]
    cand = [[0, 0], [0, 1], [0, 0], [1, 0], [0, 0]]
    draws = [[0.0, 0.0], [0.0, 0.0], [0.5, 0.5], [300.0, 300.0], [-0.5, 0.5]]
    p = R.plan(sizes, plates, [0, 2], 5, 2, cand=cand, draws=draws)
    assert p['status'].tolist() == [0, 1, 0, 6, 7] and p['slot'].tolist() == [0, -1, 1, -1, 2] and p['count'] == 2
    assert p['tally'].tolist() == [2, 1, 0, 0, 0, 0, 1, 1]
