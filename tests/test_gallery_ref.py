"""The NumPy restatement of the best-shot gallery (tests/gallery_ref.py) on cases whose answers are worked out here: the focus measure on
crops small enough to do by hand; a four-frame script of two tracks (a first shot, a better one, a worse one, the move into the arena at
the tracker's record index); under policy 'score' the shot is the tracker's best_frame / best_score; and the seeded cases the GPU tests
replay reach every branch."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gallery_ref as G  # noqa: E402
import track_ref as R  # noqa: E402


def test_sharpness_on_hand_made_crops():
    one = np.zeros((1, 3, 3, 1), np.uint8)
    one[0, 1, 1, 0] = 3                                       # Y = 12 in the centre: L = 48 at the one interior pixel
    assert G.sharpness(one).tolist() == [48 * 48]
    rgb = np.zeros((1, 3, 3, 3), np.uint8)
    rgb[0, 1, 1] = [1, 2, 3]                                  # Y = 1 + 4 + 3 = 8, L = 32
    rgb[0, 0, 1] = [0, 5, 0]                                  # the pixel above: Y = 10, L = 32 - 10 = 22
    rgb[0, 0, 0] = [255, 255, 255]                            # a corner is no neighbour of the interior pixel
    assert G.sharpness(rgb).tolist() == [22 * 22]
    assert G.sharpness(np.full((2, 2, 5, 3), 200, np.uint8)).tolist() == [0, 0]          # no interior
    assert G.sharpness(np.full((1, 5, 2, 1), 200, np.uint8)).tolist() == [0]
    assert G.sharpness(np.full((1, 4, 6, 3), 77, np.uint8)).tolist() == [0]              # a flat crop
    assert G.sharpness(one).dtype == np.int64


def test_checkerboard_exceeds_32_bits():
    yy, xx = np.mgrid[:128, :128]
    board = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[None, :, :, None], 3, axis=3)
    # Y is 0 or 1020 and every neighbour has the other value: |L| = 4 * 1020 at each of the 126 x 126 interior pixels
    want = 4080 ** 2 * 126 * 126
    assert want > 1 << 32 and G.sharpness(board).tolist() == [want]


def test_one_channel_equals_three_equal_channels():
    rs = np.random.RandomState(5)
    g = rs.randint(0, 256, size=(4, 9, 11, 1)).astype(np.uint8)
    assert G.sharpness(g).tolist() == G.sharpness(np.repeat(g, 3, axis=3)).tolist()      # 4 v == v + 2 v + v
    assert (G.sharpness(g) > 0).all()


def _dot(v):
    """a 3 x 3 x 1 crop of sharpness (16 v)^2"""
    c = np.zeros((3, 3, 1), np.uint8)
    c[1, 1, 0] = v
    return c


def test_four_frame_script():
    """Two objects far apart, max_age 0, two slots.  Slot 0: born with a crop that is not ok, then a first shot, then a worse one.
    Slot 1: a first shot at birth, then a better one, then a worse one.  Frame 3 has no detections: both retire, in slot order."""
    sc = G.Scripted(1, 2, (3, 3), 1, 4, policy=0, max_age=0)
    rows = np.zeros((2, 13))
    rows[0, :5] = [10, 10, 50, 30, 0.9]
    rows[1, :5] = [500, 500, 540, 520, 0.8]
    frame = [(rows, [0, 1])]
    crops = lambda a, b: np.stack([_dot(a), _dot(b)])[None]  # noqa: E731
    sc.step(frame, crops(9, 2), np.array([[0, 1]]))
    s = sc.gal['shots'][0]
    assert s['id'].tolist() == [0, 1] and s['shots'].tolist() == [0, 1] and s['frame'].tolist() == [-1, 0]
    assert s['key'][0] == -np.inf and np.isnan(s['score'][0]) and s['sharpness'].tolist() == [0, 32 * 32]
    assert not sc.gal['crops'][0, 0].any() and np.array_equal(sc.gal['crops'][0, 1], _dot(2))
    sc.step(frame, crops(3, 5), np.array([[1, 1]]))
    s = sc.gal['shots'][0]
    assert s['shots'].tolist() == [1, 2] and s['frame'].tolist() == [1, 1] and s['sharpness'].tolist() == [48 * 48, 80 * 80]
    assert s['key'].tolist() == [48.0 * 48, 80.0 * 80] and s['score'].tolist() == [0.9, 0.8]
    sc.step(frame, crops(2, 5), np.array([[1, 1]]))              # a worse one, and an equal one: strictly greater only
    s = sc.gal['shots'][0]
    assert s['shots'].tolist() == [2, 3] and s['frame'].tolist() == [1, 1] and s['sharpness'].tolist() == [48 * 48, 80 * 80]
    assert np.array_equal(sc.gal['crops'][0, 0], _dot(3)) and np.array_equal(sc.gal['crops'][0, 1], _dot(5))
    assert sc.gal['gstate'].tolist() == [0, 0, 0, 0] and (sc.gal['arena']['shot']['id'] == -1).all()
    sc.step([(np.zeros((0, 13)), [])], np.zeros((1, 1, 3, 3, 1), np.uint8), np.zeros((1, 1), np.int32))
    assert sc.gal['gstate'].tolist() == [2, 2, 0, 0] and (sc.gal['shots'][0]['id'] == -1).all()
    rec = R.as_records(sc.records)
    assert len(rec) == 2 and sc.astate[0] == 2
    a = sc.gal['arena']
    for i in range(2):                                            # the arena index is the tracker's record index
        assert a[i]['stream'] == rec[i]['stream'] == 0 and a[i]['slot'] == i and a[i]['shot']['id'] == rec[i]['t']['id'] == i
    assert a['shot']['frame'][:2].tolist() == [1, 1] and a['shot']['shots'][:2].tolist() == [2, 3] and (a['shot']['id'][2:] == -1).all()
    assert np.array_equal(sc.gal['arena_crops'][0], _dot(3)) and np.array_equal(sc.gal['arena_crops'][1], _dot(5))
    assert sc.events == dict(stored=2, dropped=0, lost=0, adopt=2, reborn=0, coast=0, notok=1, gated=0, first=2, replace=1, keep=2)


def test_commit_false_writes_nothing():
    sc, calls = G.case_script(G.CASES[2])
    for frames, crops, ok, _ in calls[:2]:
        sc.step(frames, crops, ok)
    frames, crops, ok, _ = calls[2]
    res = R.update_batch(sc.state, frames, 0, **sc.params)
    before = {k: v.copy() for k, v in sc.gal.items()}
    ev = G.update(sc.gal, sc.state, res, crops, ok, int(sc.astate[0]), 0, sc.policy, sc.min_score, commit=False)
    assert min(ev['stored'], ev['reborn'], ev['first'], ev['replace']) > 0 and all(np.array_equal(before[k].view(np.uint8), sc.gal[k].view(np.uint8)) for k in before)


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_score_policy_keeps_the_trackers_best_frame(seed):
    slots, max_age = 12, 1
    sc = G.Scripted(2, 16, (4, 3), 3, 64, policy=1, max_age=max_age, birth_score=R.BIRTH_SCORE)
    seqs = [R.sequence(seed + 10 * b, 8, slots, max_age, 13) for b in range(2)]
    rs = np.random.RandomState(seed)
    for step in range(8):
        sc.step([q[step] for q in seqs], rs.randint(0, 256, size=(2, slots, 3, 4, 3)).astype(np.uint8), np.ones((2, slots), np.int32))
    live = 0
    for s in range(2):
        for g, k in zip(sc.gal['shots'][s], sc.state[1][s]):
            assert g['id'] == k['id']
            if k['id'] >= 0:
                assert g['frame'] == k['best_frame'] and g['score'] == k['best_score'] == g['key'] and g['shots'] == k['hits']
                live += 1
    rec = R.as_records(sc.records)
    a = sc.gal['arena'][:len(rec)]
    assert live > 0 and len(rec) > 0 and sc.gal['gstate'].tolist() == [len(rec), len(rec), 0, 0]
    assert a['stream'].tolist() == rec['stream'].tolist() and a['shot']['id'].tolist() == rec['t']['id'].tolist()
    assert a['shot']['frame'].tolist() == rec['t']['best_frame'].tolist() and a['shot']['score'].tolist() == rec['t']['best_score'].tolist()
    assert sc.events['replace'] > 0 and sc.events['keep'] > 0


def test_the_seeded_cases_reach_every_branch():
    """the conditions tests/test_hip_gallery.py asserts on the GPU machine, from the restatement alone"""
    total = dict.fromkeys(G.EVENTS, 0)
    for case in G.CASES:
        sc, calls = G.case_script(case)
        for frames, crops, ok, with_gallery in calls:
            sc.step(frames, crops, ok, stream0=case[4], gallery=with_gallery)
        assert all(sc.events[name] > 0 for name in ('adopt', 'first', 'replace')), (case, sc.events)
        for name in G.EVENTS:
            total[name] += sc.events[name]
    print(total)
    assert all(v > 0 for v in total.values()), total
