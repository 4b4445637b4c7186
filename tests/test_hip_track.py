"""Tracking on the GPU: dbx_track_update_batch == the NumPy restatement (tests/track_ref.py) bit for bit -- every output word and the
whole state of every stream after every step of seeded 8-frame sequences, in dbx_detect_batch's slot layout and
dbx_detect_thresh_batch's packed layout, with clamped counts, bad keep entries and corrupted prefixes (clamps being exercised: the
launch reads and writes nothing outside its buffers); dbx_track_append's records and totals; net.track_batch == detect_batch /
detect_batch_thresh + the restatement on the host; track.update_batch on host results."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import densebox_amd as D
from densebox_amd import _lib, decode as DC, synth, track as T
from densebox_amd.rows import Rows
from densebox_amd._lib import check, ptr, stream_ptr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_ref as R  # noqa: E402
import thresh_ref  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64                     # sentinel elements in front of and behind every output
FILL_I, FILL_B = -777, 0xEE


def _guarded(n, dtype, fill):
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device='cuda')
    return whole, C.c_void_p(whole.data_ptr() + GUARD * whole.element_size())


def _inner(whole, n, fill, name):
    h = whole.cpu().numpy()
    assert (h[:GUARD] == fill).all() and (h[GUARD + n:] == fill).all(), 'words outside %s were written' % name
    return h[GUARD:GUARD + n]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class _Dev:
    """the state of `streams` streams on the device, from a restatement state"""

    def __init__(self, state):
        self.streams, self.T = state[1].shape
        self.headers = torch.from_numpy(state[0].copy()).cuda()
        self.tracks = torch.from_numpy(_bits(state[1]).copy()).cuda()

    def equals(self, state):
        h, t = self.headers.cpu().numpy(), self.tracks.cpu().numpy()
        assert h.tolist() == state[0].tolist(), (h, state[0])
        got = t.view(R.TRACK).reshape(self.streams, self.T)
        for name in R.TRACK.names:
            assert np.array_equal(_bits(got[name]), _bits(state[1][name])), (name, got[name], state[1][name])
        assert np.array_equal(t, _bits(state[1]))


def _launch(dev, dets, keep, prefix, B, slots, stream0, det_rows=None, iou_thresh=0.3, max_age=5, alpha=0.5, beta=0.1, birth_score=-np.inf):
    """dbx_track_update_batch called directly on device tensors; returns numpy (track_id, track_slot, track_hits [B, slots], retired
    TRACK [B, T] with unwritten bytes FILL_B, tally [B, 6]) after the containment checks; unwritten hits hold FILL_I"""
    dc = int(dets.shape[-1])
    det_rows = int(dets.numel() // dc) if det_rows is None else det_rows
    n, Tn = B * slots, dev.T
    ti, p_ti = _guarded(n, torch.int32, FILL_I)
    ts, p_ts = _guarded(n, torch.int32, FILL_I)
    th, p_th = _guarded(n, torch.int32, FILL_I)
    rt, p_rt = _guarded(B * Tn * 104, torch.uint8, FILL_B)
    ta, p_ta = _guarded(B * 6, torch.int32, FILL_I)
    check(_lib.lib().dbx_track_update_batch(ptr(dets), dc, det_rows, ptr(keep), ptr(prefix), B, slots, ptr(dev.headers), ptr(dev.tracks),
                                            dev.streams, stream0, Tn, iou_thresh, max_age, alpha, beta, birth_score, p_ti, p_ts, p_th, p_rt,
                                            p_ta, stream_ptr()))
    torch.cuda.synchronize()
    tid, slot = _inner(ti, n, FILL_I, 'track_id').reshape(B, slots), _inner(ts, n, FILL_I, 'track_slot').reshape(B, slots)
    tally = _inner(ta, B * 6, FILL_I, 'tally').reshape(B, 6)
    assert (tid != FILL_I).all() and (slot != FILL_I).all() and (tally != FILL_I).all()                 # every word is written
    hits = _inner(th, n, FILL_I, 'track_hits').reshape(B, slots)
    retired = _inner(rt, B * Tn * 104, FILL_B, 'retired').reshape(B, Tn * 104)
    return tid, slot, hits, retired, tally


def _check_frame(got, b, want, k):
    """frame b of a launch against the restatement's result for it; k the (clamped) list count: positions past it are -2 / -1 / unwritten"""
    tid, slot, hits, retired, tally = got
    w_id, w_slot, w_hits, w_ret, w_tally, _ = want
    assert len(w_id) == k
    assert tid[b, :k].tolist() == w_id.tolist() and slot[b, :k].tolist() == w_slot.tolist(), (b, tid[b, :k], w_id, slot[b, :k], w_slot)
    assert hits[b, :k].tolist() == w_hits.tolist(), (b, hits[b, :k], w_hits)
    assert (tid[b, k:] == -2).all() and (slot[b, k:] == -1).all() and (hits[b, k:] == FILL_I).all()
    assert tally[b].tolist() == w_tally.tolist(), (b, tally[b], w_tally)
    assert tally[b, 0] == tally[b, 1] + tally[b, 2] + tally[b, 3]
    n = len(w_ret) * 104
    assert np.array_equal(retired[b, :n], _bits(w_ret)), (b, retired[b, :n].view(R.TRACK), w_ret)
    assert (retired[b, n:] == FILL_B).all()


def _slot_inputs(frames, slots, dc):
    """device dets [B * slots, dc] and keep [B, slots + 1] in dbx_detect_batch's layout from per-frame (rows, keep list)"""
    B = len(frames)
    d = np.zeros((B, slots, dc), np.float64)
    k = np.zeros((B, slots + 1), np.int32)
    for b, (r, l) in enumerate(frames):
        d[b, :r.shape[0]] = r
        k[b, 0] = len(l)
        k[b, 1:1 + len(l)] = l
    return torch.from_numpy(d.reshape(B * slots, dc)).cuda(), torch.from_numpy(k).cuda()


def _busy_neighbours(state, stream0, batch):
    """streams outside the launch hold state of their own, which must come back untouched"""
    for s in range(state[0].shape[0]):
        if not stream0 <= s < stream0 + batch:
            state[0][s] = [7 + s, 3, 1, 55]
            t = state[1][s, 0]
            t['id'], t['box'], t['vel'], t['hits'], t['score'] = 2, [2000.0, 2000.0, 2040.0, 2020.0], [1.0, 0.5, 1.0, 0.5], 4, 0.75


# (max_tracks, slots, batch, det_cols, max_age, stream0, streams, seed): the smallest shapes that cross a wave (64 | 65 slots and tracks),
# the workgroup's slot tiling (one to four waves of track threads, list positions beyond one chunk of them) and the LDS bounds (1024, 256)
CASES = [
    (1, 1, 1, 5, 1, 0, 1, 1),
    (2, 65, 3, 13, 1, 2, 6, 2),
    (64, 65, 1, 5, 0, 0, 1, 3),
    (65, 1, 3, 13, 0, 1, 4, 1),
    (65, 1024, 1, 5, 1, 0, 2, 4),
    (256, 65, 3, 5, 2, 0, 3, 2),
    (256, 1024, 3, 13, 1, 1, 5, 4),
    (1, 1024, 1, 13, 0, 3, 4, 3),
]


@pytest.mark.parametrize('T_,slots,batch,dc,max_age,stream0,streams,seed', CASES)
def test_kernel_equals_the_restatement_after_every_step(T_, slots, batch, dc, max_age, stream0, streams, seed):
    seqs = [R.sequence(seed + 10 * b, 8, slots, max_age, dc) for b in range(batch)]
    state = R.new_state(streams, T_)
    _busy_neighbours(state, stream0, batch)
    dev = _Dev(state)
    params = dict(iou_thresh=0.3, max_age=max_age, alpha=0.5, beta=0.1, birth_score=R.BIRTH_SCORE)
    seen = dict(match=0, birth=0, retire=0, reuse=0, unborn=0)
    empty = 0
    for step in range(8):
        frames = [seqs[b][step] for b in range(batch)]
        want = R.update_batch(state, frames, stream0, **params)
        dets, keep = _slot_inputs(frames, slots, dc)
        got = _launch(dev, dets, keep, None, batch, slots, stream0, **params)
        for b in range(batch):
            _check_frame(got, b, want[b], len(frames[b][1]))
            for name in seen:
                seen[name] += want[b][5][name]
            empty += len(frames[b][1]) == 0
        dev.equals(state)                                              # the whole state, the neighbours' included
    assert all(v > 0 for v in seen.values()), seen                     # from the restatement alone: no branch passed vacuously
    assert slots > 1 or max_age == 0 or empty > 0                      # k = 0 frames
    assert slots < 3 or max(len(f[1]) for q in seqs for f in q) == slots                      # and a list that fills every position
    assert state[0][stream0:stream0 + batch, 0].tolist() == [8] * batch


def test_counts_are_clamped_and_bad_keep_entries_are_not_counted():
    rs = np.random.RandomState(3)
    slots, dc, Tn = 8, 13, 4
    xy = rs.randint(0, 400, size=(3, slots, 2)) / 4.0 + np.arange(slots)[None, :, None] * 200
    rows = np.zeros((3, slots, dc))
    rows[:, :, :2], rows[:, :, 2:4], rows[:, :, 4] = xy, xy + 30, 0.5 + rs.rand(3, slots) / 2
    k = np.zeros((3, slots + 1), np.int32)
    k[0] = [0, 5, 4, 3, 2, 1, 0, 7, 6]                   # count 0: the entries behind it are not read as detections
    k[1] = [slots, 7, 6, 5, 4, 3, 2, 1, 0]               # a full list: 8 detections for 4 slots
    k[2] = [100, 1, -1, 3, 8, 5, 1 << 30, 0, 3]          # a count beyond the slots is clamped; entries -1, 8 and 2^30 are outside the rows
    lists = [[], k[1, 1:].tolist(), k[2, 1:].tolist()]
    state = R.new_state(3, Tn)
    dev = _Dev(state)
    dets = torch.from_numpy(rows.reshape(3 * slots, dc)).cuda()
    for step in range(2):
        want = R.update_batch(state, [(rows[b], lists[b]) for b in range(3)], 0, max_age=0)
        got = _launch(dev, dets, torch.from_numpy(k).cuda(), None, 3, slots, 0, max_age=0)
        for b in range(3):
            _check_frame(got, b, want[b], len(lists[b]))
        dev.equals(state)
    assert got[0][2].tolist().count(-2) == 3 and got[4][2, 0] == 5 and got[4][1].tolist() == [8, 4, 0, 4, 0, 4]
    k[1, 0] = -4                                         # a negative count is 0: the four tracks of stream 1 retire (max_age 0)
    want = R.update_batch(state, [(rows[0], []), (rows[1], []), (rows[2], lists[2])], 0, max_age=0)
    got = _launch(dev, dets, torch.from_numpy(k).cuda(), None, 3, slots, 0, max_age=0)
    for b, n in enumerate((0, 0, 8)):
        _check_frame(got, b, want[b], n)
    dev.equals(state)
    assert got[4][1].tolist() == [0, 0, 0, 0, 4, 0]


def _thresh_decode(counts, cap=64):
    """dbx_detect_thresh_batch on crafted 16 x 16 maps, one image per entry of counts: (dets, keep, counts) device tensors and per image
    the host (rows, keep list)"""
    images = [thresh_ref.craft_maps(40 + i, 16, 16, n, 4) for i, n in enumerate(counts)]
    maps = {k: torch.from_numpy(np.ascontiguousarray(np.concatenate([m[k] for m in images]))).cuda() for k in images[0]}
    dets, keep, cnt = DC._run_thresh_batch(maps['score'], maps['loc'], 0.5, cap, maps['lm_heat'], maps['lm_loc'], 0.4, lists_behind_rows=False)
    torch.cuda.synchronize()
    B = len(counts)
    c, d, k = cnt.cpu().numpy(), dets.cpu().numpy(), keep.cpu().numpy()
    prefix = c[2 * B:]
    assert [int(c[2 * b]) for b in range(B)] == list(counts)
    host = []
    for b in range(B):
        p, n = int(prefix[b]), int(c[2 * b])
        l = k[p + b:p + b + n + 1]
        host.append((d[p:p + n].copy(), [int(v) for v in l[1:1 + int(l[0])]]))
    return dets, keep, cnt, host


def test_packed_layout_behind_the_threshold_decode():
    counts, cap, B = (20, 0, 37), 64, 3
    dets, keep, cnt, host = _thresh_decode(counts, cap)
    prefix = cnt[2 * B:]
    state = R.new_state(4, 4)                                           # 4 slots: frames with more kept rows leave some unborn
    dev = _Dev(state)
    p = dict(max_age=1)
    for step in range(2):                                               # births, then every track matched again at IoU 1
        want = R.update_batch(state, host, 1, **p)
        got = _launch(dev, dets, keep, prefix, B, cap, 1, **p)
        for b in range(B):
            _check_frame(got, b, want[b], len(host[b][1]))
        dev.equals(state)
    assert got[4][0, 1] == 4 and got[4][0, 3] > 0 and got[4][1].tolist() == [0] * 6         # matches; unborn rows; the frame without rows
    none = (np.zeros((0, 13)), [])
    # a decreasing prefix: frame 1 has no detections; frame 0 is untouched; frame 2 now points at other rows, all inside the buffers
    bad = torch.tensor([0, 20, 10, 57], dtype=torch.int32, device='cuda')
    d_all, k_all = dets.cpu().numpy(), keep.cpu().numpy()
    l2 = k_all[10 + 2:10 + 2 + 47 + 1]
    k2 = min(max(int(l2[0]), 0), 47)
    odd = (d_all[10:57].copy(), [int(v) for v in l2[1:1 + k2]])
    want = R.update_batch(state, [host[0], none, odd], 1, **p)
    got = _launch(dev, dets, keep, bad, B, cap, 1, **p)
    for b, fr in enumerate((host[0], none, odd)):
        _check_frame(got, b, want[b], len(fr[1]))
    dev.equals(state)
    # a prefix that ends beyond det_rows, and a negative one: those frames' tracks coast (and retire at max_age = 1)
    for bad, frames in (([0, 20, 20, 1 << 20], [host[0], none, none]), ([-5, 20, 20, 57], [none, none, host[2]])):
        want = R.update_batch(state, frames, 1, **p)
        got = _launch(dev, dets, keep, torch.tensor(bad, dtype=torch.int32, device='cuda'), B, cap, 1, **p)
        for b, fr in enumerate(frames):
            _check_frame(got, b, want[b], len(fr[1]))
        dev.equals(state)
    assert state[0][:, 0].tolist() == [0, 5, 5, 5]


def test_append_orders_records_counts_totals_and_drops_beyond_capacity():
    rs = np.random.RandomState(21)
    B, slots, dc = 3, 8, 5
    rows = np.zeros((B, slots, dc))
    xy = rs.randint(0, 400, size=(B, slots, 2)) / 4.0 + np.arange(slots)[None, :, None] * 200
    rows[:, :, :2], rows[:, :, 2:4], rows[:, :, 4] = xy, xy + 30, 0.5 + rs.rand(B, slots) / 2
    first = [(rows[b], l) for b, l in enumerate(([3, 2, 0, 4], [1], [7, 6, 5, 4, 3, 2, 1, 0]))]
    gone = [(rows[b], l) for b, l in enumerate(([3], [], [6, 1]))]                       # 3 + 1 + 6 tracks end (max_age 0)
    big = T.Tracker(5, max_tracks=8, max_age=0, capacity=64)
    small = T.Tracker(5, max_tracks=8, max_age=0, capacity=12)
    state = R.new_state(5, 8)
    astate, records = np.zeros(4, np.int64), []
    for frames in (first, gone, first, gone):
        want = R.update_batch(state, frames, 2, max_age=0)
        R.append(astate, records, 64, want, 2)
        dets, keep = _slot_inputs(frames, slots, dc)
        for tr in (big, small):
            T._launch(tr, Rows(dets, keep, None, B, slots), 2)
    assert astate.tolist() == [20, 0, 20, 0]
    got = big.finished()
    assert got.shape == (20,) and np.array_equal(_bits(got), _bits(R.as_records(records)))
    assert got['stream'].tolist() == [2] * 3 + [3] + [4] * 6 + [2] * 3 + [3] + [4] * 6
    o_app = small._layout()[1]
    assert small._state[o_app:].cpu().numpy().view(np.int64).tolist() == [12, 8, 20, 0]
    assert np.array_equal(small._records.cpu().numpy(), _bits(R.as_records(records)[:12]))
    with pytest.raises(RuntimeError, match='8 records did not fit'):
        small.finished()
    h, t = big._host_state()
    assert h.tolist() == state[0].tolist() and np.array_equal(_bits(t), _bits(state[1]))
    live = big.live()
    assert [l['id'].tolist() for l in live] == [state[1][s]['id'][state[1][s]['id'] >= 0].tolist() for s in range(5)]
    big.reset()
    assert big.finished().shape == (0,) and not big.headers().any() and all(l.shape == (0,) for l in big.live())


def _net(kind, dtype):
    net = getattr(D, kind)(synth.vgg19_standin(seed=0))
    synth.fill_params_(net, 11)
    # The seeded stand-in gives boxes of any shape, most of them with x2 < x1, which overlap nothing.  The last layer of the box head is
    # set so that every pixel's box is 17 x 13 pixels around it, as tests/test_hip_evaluate.py does.
    with torch.no_grad():
        net.conv5_2_loc.weight.zero_()
        net.conv5_2_loc.bias.copy_(torch.tensor([2.0, 1.5, -2.0, -1.5]))
    net = net.cuda().eval()
    net.compute_dtype = dtype
    return net


def _same_results(got, ref, want):
    for (d, keep, tid, hits), (rd, rkeep), w in zip(got, ref, want):
        assert np.array_equal(_bits(d), _bits(rd)) and keep == rkeep
        assert tid.dtype == np.int32 and hits.dtype == np.int32
        assert tid.tolist() == w[0].tolist() and hits.tolist() == w[2].tolist(), (tid, w[0], hits, w[2])


@pytest.mark.parametrize('mode', ['topk', 'thresh'])
@pytest.mark.parametrize('dtype', ['f32', 'f16'])
@pytest.mark.parametrize('kind', ['DenseBox', 'DenseBoxLMLOC'])
def test_track_batch_is_detect_batch_plus_the_restatement(kind, dtype, mode, monkeypatch):
    monkeypatch.delenv('DBX_GRAPH', raising=False)
    net = _net(kind, dtype)
    rs = np.random.RandomState(17)
    X = torch.from_numpy(rs.randint(0, 256, size=(3, 64, 64, 3)).astype(np.uint8)).cuda()
    Y = torch.from_numpy(rs.randint(0, 256, size=(3, 64, 64, 3)).astype(np.uint8)).cuda()
    top = net.detect_batch(X, K=10, max_batch=2)
    if mode == 'topk':
        kw = dict(K=10)
        detect = lambda x: net.detect_batch(x, K=10, max_batch=2)  # noqa: E731
    else:
        best = np.sort(np.concatenate([d[:, 4] for d, _ in top]))[::-1]
        kw = dict(score_thresh=float(np.float32(best[12])), max_dets=64)            # a dozen pixels or more pass, at most 64 per frame
        detect = lambda x: net.detect_batch_thresh(x, kw['score_thresh'], 64, max_batch=2)  # noqa: E731
    refs = [detect(X), detect(X), detect(Y)]
    par = dict(iou_thresh=0.3, max_age=1, alpha=0.5, beta=0.1, birth_score=-np.inf)
    state = R.new_state(5, 64)
    wants = [R.update_batch(state, ref, 1, **par) for ref in refs]
    print(kind, dtype, mode, 'tallies', [[w[4].tolist() for w in ws] for ws in wants])
    for env in (None, '0'):                                                         # the graph, then the same launches without it
        if env is not None:
            monkeypatch.setenv('DBX_GRAPH', env)
        tr = T.Tracker(5, max_tracks=64, max_age=1)
        got = net.track_batch(X, tracker=tr, stream0=1, max_batch=2, **kw)
        assert tr.headers()[:, 0].tolist() == [0, 1, 1, 1, 0]                       # the capture's warm-up runs did not count
        _same_results(got, refs[0], wants[0])
        again = net.track_batch(X, tracker=tr, stream0=1, max_batch=2, **kw)
        _same_results(again, refs[1], wants[1])
        for (_, keep, tid, hits), (_, _, tid0, _) in zip(again, got):               # every kept row matches its own track at IoU 1
            assert tid.tolist() == tid0.tolist() and (tid >= 0).all() and (hits == 2).all()
        assert sum(len(keep) for _, keep, _, _ in again) > 0
        _same_results(net.track_batch(list(Y), tracker=tr, stream0=1, max_batch=2, **kw), refs[2], wants[2])
        h, t = tr._host_state()
        assert h.tolist() == state[0].tolist() and np.array_equal(_bits(t), _bits(state[1]))
        assert [l['id'].tolist() for l in tr.live()] == [state[1][s]['id'][state[1][s]['id'] >= 0].tolist() for s in range(5)]
        if env is None:
            assert sorted(k[0] for k in net._detect_graphs if k[0] == 'track') == ['track'] * 2        # chunks of 2 and 1 frames
    monkeypatch.delenv('DBX_GRAPH')
    # the other entries of the cache are not disturbed
    assert all(np.array_equal(_bits(a), _bits(b)) and ka == kb for (a, ka), (b, kb) in zip(net.detect_batch(X, K=10, max_batch=2), top))


def test_update_batch_on_host_results():
    net = _net('DenseBoxLMLOC', 'f16')
    rs = np.random.RandomState(23)
    x = torch.from_numpy(rs.randint(0, 256, size=(3, 64, 64, 3)).astype(np.uint8)).cuda()
    res = net.detect_batch(x, K=10)
    res.append((np.zeros((0, 13)), []))                                                  # an image without rows
    state = R.new_state(6, 8)
    astate, records = np.zeros(4, np.int64), []
    tr = T.Tracker(6, max_tracks=8, max_age=0)
    for step in range(3):
        frames = res if step != 1 else res[::-1]                                         # other streams' rows: retirements and births
        want = R.update_batch(state, frames, 2, max_age=0)
        R.append(astate, records, tr.capacity, want, 2)
        dets, keeps = [d for d, _ in frames], [k for _, k in frames]
        dets[1] = torch.from_numpy(dets[1]).cuda()                                       # a device result among host ones
        out = T.update_batch(dets, keeps, tracker=tr, stream0=2)
        assert len(out) == 4
        for (tid, hits), w in zip(out, want):
            assert tid.dtype == np.int32 and tid.tolist() == w[0].tolist() and hits.tolist() == w[2].tolist()
    h, t = tr._host_state()
    assert h.tolist() == state[0].tolist() and np.array_equal(_bits(t), _bits(state[1]))
    assert len(records) > 0 and np.array_equal(_bits(tr.finished()), _bits(R.as_records(records)))
