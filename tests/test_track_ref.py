"""The NumPy restatement of the tracking semantics (tests/track_ref.py) on hand-worked sequences with the expected ids, slots and state
written out, and the seeded sequences of the GPU tests: each must run every branch (match, birth, retirement, a slot freed and taken
again in one frame, an unborn detection), so that no comparison passes vacuously."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_ref as R  # noqa: E402

NAN = float('nan')


def _rows(boxes, scores=None):
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    d = np.zeros((b.shape[0], 5), np.float64)
    d[:, :4] = b
    d[:, 4] = 0.9 - 0.05 * np.arange(b.shape[0]) if scores is None else scores
    return d


def _step(state, boxes, keep=None, scores=None, **params):
    d = _rows(boxes, scores)
    return R.update_batch(state, [(d, list(range(d.shape[0])) if keep is None else keep)], **params)[0]


def test_a_track_followed_over_three_frames():
    st = R.new_state(1, 4)
    tid, slot, hits, ret, tally, _ = _step(st, [[0, 0, 9, 9]], scores=[0.5])
    assert (tid.tolist(), slot.tolist(), hits.tolist(), tally.tolist()) == ([0], [0], [1], [1, 0, 1, 0, 0, 1])
    # frame 1: the box moved by (2, 0); prediction = the old box (vel 0); r = 2: box = p + 0.5 * 2, vel = 0.1 * 2
    tid, slot, hits, ret, tally, _ = _step(st, [[2, 0, 11, 9]], scores=[0.8])
    assert (tid.tolist(), slot.tolist(), hits.tolist(), tally.tolist()) == ([0], [0], [2], [1, 1, 0, 0, 0, 1])
    t = st[1][0, 0]
    assert t['box'].tolist() == [1.0, 0.0, 10.0, 9.0] and t['vel'].tolist() == [0.2, 0.0, 0.2, 0.0]
    assert (t['score'], t['best_score'], t['best_frame'], t['last_frame'], t['first_frame']) == (0.8, 0.8, 1, 1, 0)
    # frame 2: p = (1.2, 0, 10.2, 9); the row is at 3.2: r = 2, box = 2.2, vel = 0.2 + 0.1 * 2; a lower score keeps best_*
    tid, _, hits, _, _, _ = _step(st, [[3.2, 0, 12.2, 9]], scores=[0.6])
    t = st[1][0, 0]
    assert tid.tolist() == [0] and hits.tolist() == [3]
    assert t['box'].tolist() == [1.2 + 0.5 * (3.2 - 1.2), 0.0, 10.2 + 0.5 * (12.2 - 10.2), 9.0]
    assert t['vel'].tolist() == [0.2 + 0.1 * (3.2 - 1.2), 0.0, 0.2 + 0.1 * (12.2 - 10.2), 0.0]
    assert (t['score'], t['best_score'], t['best_frame'], t['last_frame']) == (0.6, 0.8, 1, 2)
    assert st[0][0].tolist() == [3, 1, 0, 0]


def test_a_one_frame_miss_is_bridged_and_a_longer_one_retires():
    st = R.new_state(1, 2)
    p = dict(max_age=1)
    _step(st, [[0, 0, 9, 9]], **p)
    _step(st, [[2, 0, 11, 9]], **p)                                      # vel = (0.2, 0, 0.2, 0), box = (1, 0, 10, 9)
    tid, _, _, ret, tally, _ = _step(st, np.zeros((0, 4)), **p)          # missed: coasts to (1.2, 0, 10.2, 9), age 1
    assert tid.tolist() == [] and len(ret) == 0 and tally.tolist() == [0, 0, 0, 0, 0, 1]
    assert st[1][0, 0]['box'].tolist() == [1.2, 0.0, 10.2, 9.0] and st[1][0, 0]['age'] == 1
    tid, _, hits, _, _, _ = _step(st, [[2, 0, 11, 9]], **p)              # back: the same id, age 0
    assert tid.tolist() == [0] and hits.tolist() == [3] and st[1][0, 0]['age'] == 0
    _step(st, np.zeros((0, 4)), **p)
    tid, _, _, ret, tally, _ = _step(st, np.zeros((0, 4)), **p)          # age 2 > max_age: retired
    assert len(ret) == 1 and ret[0]['id'] == 0 and ret[0]['age'] == 2 and ret[0]['hits'] == 3 and ret[0]['last_frame'] == 3
    assert tally.tolist() == [0, 0, 0, 0, 1, 0] and st[1][0, 0]['id'] == -1
    tid, slot, _, _, _, _ = _step(st, [[2, 0, 11, 9]], **p)              # the same place later is a new track
    assert tid.tolist() == [1] and slot.tolist() == [0]


def test_two_detections_compete_for_one_track():
    st = R.new_state(1, 4)
    _step(st, [[0, 0, 9, 9]])
    # list order decides: [1, 0, 10, 9] (IoU 9/11) is walked first and takes the track although the second row overlaps it fully
    tid, slot, hits, _, tally, _ = _step(st, [[1, 0, 10, 9], [0, 0, 9, 9]])
    assert (tid.tolist(), slot.tolist(), hits.tolist()) == ([0, 1], [0, 1], [2, 1]) and tally.tolist() == [2, 1, 1, 0, 0, 2]
    # and with the keep list reversed on a fresh tracker the other row wins
    st = R.new_state(1, 4)
    _step(st, [[0, 0, 9, 9]])
    tid, slot, _, _, _, _ = _step(st, [[1, 0, 10, 9], [0, 0, 9, 9]], keep=[1, 0])
    assert (tid.tolist(), slot.tolist()) == ([0, 1], [0, 1]) and st[1][0, 0]['box'].tolist() == [0.0, 0.0, 9.0, 9.0]


def test_an_iou_tie_goes_to_the_lowest_slot_and_the_threshold_is_strict():
    st = R.new_state(1, 4)
    _step(st, [[0, 5, 9, 9], [0, 0, 9, 4]])                              # two tracks of area 50 inside [0, 0, 9, 9]: IoU 0.5 each
    tid, slot, _, _, tally, _ = _step(st, [[0, 0, 9, 9]], iou_thresh=0.4)
    assert (tid.tolist(), slot.tolist()) == ([0], [0]) and tally.tolist() == [1, 1, 0, 0, 0, 2]
    st = R.new_state(1, 4)
    _step(st, [[0, 5, 9, 9]])
    tid, slot, _, _, tally, _ = _step(st, [[0, 0, 9, 9]], iou_thresh=0.5)   # ovr == iou_thresh does not match: a birth
    assert (tid.tolist(), slot.tolist()) == ([1], [1]) and tally.tolist() == [1, 0, 1, 0, 0, 2]


def test_a_full_table_counts_unborn_detections():
    st = R.new_state(1, 2)
    tid, slot, hits, _, tally, _ = _step(st, [[0, 0, 9, 9], [100, 0, 109, 9], [200, 0, 209, 9]])
    assert (tid.tolist(), slot.tolist(), hits.tolist()) == ([0, 1, -1], [0, 1, -1], [1, 1, 0])
    assert tally.tolist() == [3, 0, 2, 1, 0, 2] and st[0][0].tolist() == [1, 2, 1, 0]
    tid, _, _, _, tally, _ = _step(st, [[200, 0, 209, 9], [0, 0, 9, 9]], birth_score=0.0)
    assert tid.tolist() == [-1, 0] and tally.tolist() == [2, 1, 0, 1, 0, 2] and st[0][0].tolist() == [2, 2, 2, 0]


def test_a_slot_freed_in_the_update_is_taken_by_a_birth_of_the_same_frame():
    st = R.new_state(1, 2)
    p = dict(max_age=0)
    _step(st, [[0, 0, 9, 9], [100, 0, 109, 9]], **p)
    tid, slot, _, ret, tally, ev = _step(st, [[100, 0, 109, 9], [300, 0, 309, 9]], **p)
    # track 0 (slot 0) is not seen: age 1 > 0, retired; the stranger is born into slot 0 in the same frame
    assert (tid.tolist(), slot.tolist()) == ([1, 2], [1, 0]) and ret['id'].tolist() == [0] and tally.tolist() == [2, 1, 1, 0, 1, 2]
    assert ev['reuse'] == 1 and st[1][0, 0]['id'] == 2 and st[1][0, 0]['first_frame'] == 1


def test_rows_that_may_not_be_born_and_bad_keep_entries():
    st = R.new_state(1, 4)
    tid, slot, hits, _, tally, _ = _step(st, [[0, NAN, 9, 9], [0, 0, 9, 9], [50, 50, np.inf, 59], [80, 80, 89, 89], [90, 90, 99, 99]],
                                        scores=[0.9, 0.8, 0.7, 0.2, NAN], keep=[0, 7, 1, 2, -1, 3, 4], birth_score=0.5)
    assert tid.tolist() == [-1, -2, 0, -1, -2, -1, -1] and slot.tolist() == [-1, -1, 0, -1, -1, -1, -1]
    assert tally.tolist() == [5, 0, 1, 4, 0, 1] and st[0][0].tolist() == [1, 1, 4, 0]
    # a NaN row never matches either: the track coasts
    tid, _, _, _, tally, _ = _step(st, [[0, NAN, 9, 9]], birth_score=0.5)
    assert tid.tolist() == [-1] and tally.tolist() == [1, 0, 0, 1, 0, 1] and st[1][0, 0]['age'] == 1


def test_streams_are_independent_and_append_orders_and_drops():
    st = R.new_state(4, 2)
    p = dict(max_age=0)
    frames = [(_rows([[0, 0, 9, 9], [100, 0, 109, 9]]), [0, 1]), (_rows([[0, 0, 9, 9]]), [0])]
    R.update_batch(st, frames, stream0=1, **p)
    assert st[0][:, 0].tolist() == [0, 1, 1, 0] and st[0][:, 1].tolist() == [0, 2, 1, 0] and (st[1]['id'][[0, 3]] == -1).all()
    res = R.update_batch(st, [(np.zeros((0, 5)), []), (np.zeros((0, 5)), [])], stream0=1, **p)
    astate, records = np.zeros(4, np.int64), []
    R.append(astate, records, 2, res, stream0=1)
    assert astate.tolist() == [2, 1, 3, 0]
    rec = R.as_records(records)
    assert rec['stream'].tolist() == [1, 1] and rec['t']['id'].tolist() == [0, 1] and rec['t']['age'].tolist() == [1, 1]


CASES = [(seed, slots, max_age) for seed in (1, 2, 3) for slots in (1, 65) for max_age in (0, 1, 2)] + [(4, 1024, 1)]


@pytest.mark.parametrize('seed,slots,max_age', CASES)
def test_the_seeded_sequences_run_every_branch(seed, slots, max_age):
    for T in (1, 2, 64):
        st = R.new_state(1, T)
        seen = dict(match=0, birth=0, retire=0, reuse=0, unborn=0)
        for d, k in R.sequence(seed, 8, slots, max_age, crowd=100):
            assert d.shape[0] <= slots and len(k) <= slots
            ev = R.update_batch(st, [(d, k)], max_age=max_age, birth_score=R.BIRTH_SCORE)[0][5]
            for name in seen:
                seen[name] += ev[name]
        assert all(v > 0 for v in seen.values()), (T, seen)
