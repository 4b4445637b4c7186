"""Evaluation on the GPU: dbx_match_gt_batch == the NumPy restatement (tests/eval_ref.py), bit for bit in status, gt_index, tally and IoU
and within 1e-12 relative in lm_err (about 20 double operations of at most 1 ulp each; the margin covers fused multiply-adds), in
dbx_detect_batch's slot layout and dbx_detect_thresh_batch's packed layout, with clamped counts, bad keep entries and corrupted prefixes
(clamps being exercised: the launch reads nothing outside its buffers); dbx_eval_append's records and totals; net.evaluate_batch ==
detect_batch / detect_batch_thresh + the restatement on the host; match_batch on host results."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import densebox_amd as D
from densebox_amd import _lib, decode as DC, evaluate as E, synth
from densebox_amd.rows import Rows
from densebox_amd._lib import check, ptr, stream_ptr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_ref as R  # noqa: E402
import thresh_ref  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64                     # sentinel elements in front of and behind every output
FILL_I, FILL_D = -777, 12345.5


def _guarded(n, dtype, fill):
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device='cuda')
    return whole, C.c_void_p(whole.data_ptr() + GUARD * whole.element_size())


def _inner(whole, n, fill, name):
    h = whole.cpu().numpy()
    assert (h[:GUARD] == fill).all() and (h[GUARD + n:] == fill).all(), 'words outside %s were written' % name
    return h[GUARD:GUARD + n]


def _launch(dets, keep, prefix, B, slots, frames, max_gt, gt_cols, thr, det_rows=None, with_err=True):
    """dbx_match_gt_batch called directly on device tensors dets [rows, dc] / keep / prefix (or None); returns numpy (status, gt_index,
    iou, lm_err or None) [B, slots] and tally [B, 5] after the containment checks; unwritten iou / lm_err words hold FILL_D"""
    dc = int(dets.shape[-1])
    det_rows = int(dets.numel() // dc) if det_rows is None else det_rows
    gtbuf = torch.from_numpy(E._pack_gt(frames, max_gt, gt_cols)).cuda()
    o_cnt, o_ign, _ = E._gt_layout(B, max_gt, gt_cols)
    n = B * slots
    st, p_st = _guarded(n, torch.int32, FILL_I)
    ix, p_ix = _guarded(n, torch.int32, FILL_I)
    io, p_io = _guarded(n, torch.float64, FILL_D)
    er, p_er = _guarded(n, torch.float64, FILL_D)
    ta, p_ta = _guarded(B * 5, torch.int32, FILL_I)
    with_err = with_err and dc == 13 and gt_cols == 12
    g = gtbuf.data_ptr()
    check(_lib.lib().dbx_match_gt_batch(ptr(dets), dc, det_rows, ptr(keep), ptr(prefix), B, slots, C.c_void_p(g), gt_cols,
                                        C.c_void_p(g + o_cnt), C.c_void_p(g + o_ign), max_gt, thr, p_st, p_ix, p_io,
                                        p_er if with_err else None, p_ta, stream_ptr()))
    torch.cuda.synchronize()
    status, index = _inner(st, n, FILL_I, 'status').reshape(B, slots), _inner(ix, n, FILL_I, 'gt_index').reshape(B, slots)
    tally = _inner(ta, B * 5, FILL_I, 'tally').reshape(B, 5)
    assert (status != FILL_I).all() and (index != FILL_I).all() and (tally != FILL_I).all()           # every word is written
    iou = _inner(io, n, FILL_D, 'iou').reshape(B, slots)
    err = _inner(er, n, FILL_D, 'lm_err').reshape(B, slots)
    assert with_err or (err == FILL_D).all()
    return status, index, iou, (err if with_err else None), tally


def _same_f64(a, b):
    """equal bits where both are numbers, NaN in the same places"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = np.isnan(a)
    return a.shape == b.shape and np.array_equal(n, np.isnan(b)) and np.array_equal(a[~n].view(np.int64), b[~n].view(np.int64))


def _check_frame(got, b, rows, keep, frame, thr, slots):
    """frame b of a launch's results against the restatement on (rows, keep list); the positions past the list are -2 / -1 / unwritten"""
    status, index, iou, err, tally = got
    boxes, ign, quads = frame
    s, j, o, e, t = R.match_frame(rows, keep, boxes, ign, quads if err is not None else None, thr)
    k = len(keep)
    assert status[b, :k].tolist() == s.tolist() and index[b, :k].tolist() == j.tolist(), (b, status[b, :k], s)
    assert (status[b, k:] == -2).all() and (index[b, k:] == -1).all()
    assert tally[b].tolist() == t.tolist(), (b, tally[b], t)
    assert _same_f64(iou[b, :k], o), (b, iou[b, :k], o)
    assert (iou[b, k:] == FILL_D).all()
    if err is not None:
        assert np.array_equal(np.isnan(err[b, :k]), np.isnan(e)) and (err[b, k:] == FILL_D).all()
        m = ~np.isnan(e)
        assert np.allclose(err[b, :k][m], e[m], rtol=1e-12, atol=0.0), (b, err[b, :k], e)
    return s


def _slot_inputs(frames_rows, lists, slots, dc):
    """device dets [B * slots, dc] and keep [B, slots + 1] in dbx_detect_batch's layout from per-frame rows and keep lists"""
    B = len(frames_rows)
    d = np.zeros((B, slots, dc), np.float64)
    k = np.zeros((B, slots + 1), np.int32)
    for b, (r, l) in enumerate(zip(frames_rows, lists)):
        d[b, :r.shape[0]] = r
        k[b, 0] = len(l)
        k[b, 1:1 + len(l)] = l
    return torch.from_numpy(d.reshape(B * slots, dc)).cuda(), torch.from_numpy(k).cuda()


def _gt_frame(boxes, ign=None, dc=13):
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    return (b, np.zeros(b.shape[0], np.uint8) if ign is None else np.asarray(ign, np.uint8), R.quad_of(b) if dc == 13 else None)


@pytest.mark.parametrize('dc', [5, 13])
def test_hand_worked_frames_in_slot_layout(dc):
    seen = 0
    for thr in sorted({c[5] for c in R.HAND_CASES}):
        cases = [c for c in R.HAND_CASES if c[5] == thr]
        for c0 in range(0, len(cases), 3):
            part = (cases[c0:c0 + 3] + cases * 3)[:3]                       # batch = 3: the last group is filled up from the front
            rows = [R._rows(c[1], dc=dc) for c in part]
            lists = [c[2] for c in part]
            frames = [_gt_frame(c[3], c[4], dc) for c in part]
            dets, keep = _slot_inputs(rows, lists, 8, dc)
            got = _launch(dets, keep, None, 3, 8, frames, 4, 12 if dc == 13 else 4, thr)
            for b, c in enumerate(part):
                s = _check_frame(got, b, rows[b], lists[b], frames[b], thr, 8)
                assert s.tolist() == c[6] and got[1][b, :len(c[7])].tolist() == c[7]           # and the hand-worked values themselves
                seen += 1
    assert seen >= len(R.HAND_CASES)


def test_counts_are_clamped_and_bad_keep_entries_are_not_counted():
    rs = np.random.RandomState(3)
    slots, dc = 8, 13
    xy = rs.randint(0, 40, size=(3, slots, 2)) / 4.0
    boxes = np.concatenate([xy, xy + rs.randint(8, 40, size=(3, slots, 2)) / 4.0], axis=2)
    rows = [R._rows(boxes[b], dc=dc) for b in range(3)]
    frames = [_gt_frame(boxes[b, [1, 3, 5]] + 0.25, [0, 1, 0]) for b in range(3)]
    k = np.zeros((3, slots + 1), np.int32)
    k[0] = [0, 5, 4, 3, 2, 1, 0, 7, 6]                   # count 0: the entries behind it are not read as detections
    k[1] = [slots, 7, 6, 5, 4, 3, 2, 1, 0]               # a full list
    k[2] = [100, 1, -1, 3, 8, 5, 1 << 30, 0, 3]          # a count beyond the slots is clamped; entries -1, 8 and 2^30 are outside the rows
    dets = torch.from_numpy(np.stack(rows).reshape(3 * slots, dc)).cuda()
    got = _launch(dets, torch.from_numpy(k).cuda(), None, 3, slots, frames, 3, 12, 0.5)
    want = [[], k[1, 1:].tolist(), k[2, 1:].tolist()]
    for b in range(3):
        s = _check_frame(got, b, rows[b], want[b], frames[b], 0.5, slots)
    assert s.tolist().count(-2) == 3 and got[4][2, 0] == 5
    k[0, 0] = -4                                         # a negative count is 0
    got = _launch(dets, torch.from_numpy(k).cuda(), None, 3, slots, frames, 3, 12, 0.5)
    _check_frame(got, 0, rows[0], [], frames[0], 0.5, slots)
    short = [(f[0][:n], f[1][:n], f[2][:n]) for f, n in zip(frames, (0, 3, 2))]        # gt_counts 0 and below max_gt
    got = _launch(dets, torch.from_numpy(k).cuda(), None, 3, slots, short, 3, 12, 0.5)
    for b in range(3):
        _check_frame(got, b, rows[b], want[b], short[b], 0.5, slots)


def _quarter_boxes(rs, n, field, lo, hi):
    xy = rs.randint(0, field * 4, size=(n, 2)) / 4.0
    return np.concatenate([xy, xy + rs.randint(lo * 4, hi * 4, size=(n, 2)) / 4.0], axis=1)


def test_random_frames_with_more_than_64_gt_boxes():
    rs = np.random.RandomState(11)
    B, slots, max_gt, dc = 2, 64, 70, 13
    rows = [R._rows(_quarter_boxes(rs, slots, 60, 3, 14), dc=dc) for _ in range(B)]
    frames = []
    for b, g in enumerate((70, 65)):
        gt = _quarter_boxes(rs, g, 60, 3, 14)
        gt[:20] = rows[b][rs.permutation(slots)[:20], :4] + rs.randint(-2, 3, size=(20, 4)) / 4.0      # near hits
        gt[69 if g == 70 else 64] = gt[3]                                                               # a twin beyond lane 63
        frames.append((gt, (rs.rand(g) < 0.2).astype(np.uint8), R.quad_of(gt) + rs.randint(-4, 5, size=(g, 8)) / 4.0))
    lists = [rs.permutation(slots).tolist(), rs.permutation(slots)[:40].tolist()]
    dets, keep = _slot_inputs(rows, lists, slots, dc)
    for thr in (0.5, 0.2):
        got = _launch(dets, keep, None, B, slots, frames, max_gt, 12, thr)
        seen = set()
        for b in range(B):
            s = _check_frame(got, b, rows[b], lists[b], frames[b], thr, slots)
            seen |= set(s.tolist())
        assert seen >= {1, 0, -1}, seen
    assert (got[1] >= 64).any()                              # a GT beyond the first 64 was the best somewhere


def test_one_frame_at_the_limits():
    """slots = 4096, max_gt = 1024: a 32 x 32 grid of 8 x 8 GT boxes and four jittered detections per cell on average, so most GT boxes
    are claimed by several detections"""
    rs = np.random.RandomState(5)
    slots, max_gt = 4096, 1024
    cx, cy = np.meshgrid(np.arange(32) * 8.0, np.arange(32) * 8.0)
    gt = np.stack([cx.ravel(), cy.ravel(), cx.ravel() + 7, cy.ravel() + 7], axis=1)
    cell = rs.randint(0, 1024, size=slots)
    rows = R._rows(gt[cell] + rs.randint(-1, 2, size=(slots, 4)), scores=rs.rand(slots), dc=5)
    frame = (gt, (rs.rand(max_gt) < 0.05).astype(np.uint8), None)
    lst = rs.permutation(slots).tolist()
    dets, keep = _slot_inputs([rows], [lst], slots, 5)
    got = _launch(dets, keep, None, 1, slots, [frame], max_gt, 4, 0.5)
    s = _check_frame(got, 0, rows, lst, frame, 0.5, slots)
    dup = ((s == 0) & (got[1][0] >= 0)).sum()
    assert (s == 1).sum() > 500 and dup > 500 and (s == -1).sum() > 50, ((s == 1).sum(), dup)


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


def _gt_from(rows, keep, rs):
    """GT from a frame's own kept rows: the first ones shifted by a pixel or two (one of them ignored), and one box far away"""
    take = keep[:3]
    boxes = [rows[r, :4] + rs.randint(-2, 3, size=4) for r in take] + [np.array([500.0, 500.0, 540.0, 520.0])]
    ign = [0] * len(boxes)
    if len(take) > 1:
        ign[1] = 1
    quads = [rows[r, 5:13] + 1.0 if rows.shape[1] == 13 else np.zeros(8) for r in take] + [np.zeros(8)]
    return np.array(boxes, np.float64), np.array(ign, np.uint8), np.array(quads, np.float64)


def test_packed_layout_behind_the_threshold_decode():
    counts, cap, B = (20, 0, 37), 64, 3
    dets, keep, cnt, host = _thresh_decode(counts, cap)
    rs = np.random.RandomState(9)
    frames = [_gt_from(r, k, rs) for r, k in host]
    prefix = cnt[2 * B:]
    n_gt = [int((f[1] == 0).sum()) for f in frames]
    got = _launch(dets, keep, prefix, B, cap, frames, 4, 12, 0.5)
    seen = set()
    for b in range(B):
        seen |= set(_check_frame(got, b, host[b][0], host[b][1], frames[b], 0.5, cap).tolist())
    assert seen >= {1, -1} and got[4][1].tolist() == [0, 0, 0, 0, n_gt[1]]          # the image without candidates: only its GT count
    # a decreasing prefix: frame 1 is empty, frame 0 is untouched; frame 2 now points at other rows, all of them inside the buffers
    bad = torch.tensor([0, 20, 10, 57], dtype=torch.int32, device='cuda')
    g2 = _launch(dets, keep, bad, B, cap, frames, 4, 12, 0.5)
    _check_frame(g2, 0, host[0][0], host[0][1], frames[0], 0.5, cap)
    assert (g2[0][1] == -2).all() and g2[4][1].tolist() == [0, 0, 0, 0, n_gt[1]]
    assert set(np.unique(g2[0][2]).tolist()) <= {-2, -1, 0, 1}
    # a prefix that ends beyond det_rows, and a negative one: both frames are empty
    bad = torch.tensor([0, 20, 20, 1 << 20], dtype=torch.int32, device='cuda')
    g3 = _launch(dets, keep, bad, B, cap, frames, 4, 12, 0.5)
    _check_frame(g3, 0, host[0][0], host[0][1], frames[0], 0.5, cap)
    assert (g3[0][2] == -2).all() and g3[4][2].tolist() == [0, 0, 0, 0, n_gt[2]]
    bad = torch.tensor([-5, 20, 20, 57], dtype=torch.int32, device='cuda')
    g4 = _launch(dets, keep, bad, B, cap, frames, 4, 12, 0.5)
    assert (g4[0][0] == -2).all() and g4[4][0].tolist() == [0, 0, 0, 0, n_gt[0]]
    _check_frame(g4, 2, host[2][0], host[2][1], frames[2], 0.5, cap)


def _append(dets, keep, prefix, B, slots, status, err, tally, records, capacity, state):
    dc = int(dets.shape[-1])
    check(_lib.lib().dbx_eval_append(ptr(dets), dc, dets.numel() // dc, ptr(keep), ptr(prefix), B, slots, ptr(status), ptr(err), ptr(tally),
                                     ptr(records), capacity, ptr(state), stream_ptr()))


def _records_equal(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got['score'].view(np.int64), want['score'].view(np.int64))
    assert np.array_equal(got['status'], want['status']) and np.array_equal(got['frame'], want['frame'])
    n = np.isnan(want['lm_err'])
    assert np.array_equal(np.isnan(got['lm_err']), n) and np.allclose(got['lm_err'][~n], want['lm_err'][~n], rtol=1e-12, atol=0.0)


def test_append_orders_records_counts_totals_and_drops_beyond_capacity():
    rs = np.random.RandomState(21)
    B, slots, dc = 3, 8, 13
    rows = [R._rows(_quarter_boxes(rs, slots, 20, 3, 10), scores=rs.rand(slots), dc=dc) for _ in range(B)]
    frames = [_gt_frame(rows[b][[0, 2, 4], :4] + 0.5, [0, 0, 1]) for b in range(B)]
    lists = [[3, 2, 0, 9, 4], [], [7, 6, 5, 4, 3, 2, 1, 0]]                   # a bad entry in frame 0, an empty frame
    dets, keep = _slot_inputs(rows, lists, slots, dc)
    o_cnt, o_ign, _ = E._gt_layout(B, 3, 12)
    gtbuf = torch.from_numpy(E._pack_gt(frames, 3, 12)).cuda()
    status, index, iou, err, tally = E._launch_match(Rows(dets, keep, None, B, slots), gtbuf, 12, 3, 0.5)
    ref = [R.match_frame(rows[b], lists[b], *frames[b], 0.5) for b in range(B)]
    want = R.records([(rows[b], lists[b], ref[b][0], ref[b][3]) for b in range(B)])
    assert len(want) == 12
    ev = E.Evaluator(capacity=64, max_gt=3)
    records, state = ev._buffers(torch.device('cuda'))
    _append(dets, keep, None, B, slots, status, err, tally, records, ev.capacity, state)
    _append(dets, keep, None, B, slots, status, err, tally, records, ev.capacity, state)      # the second call: frames 3..5 behind the first
    s = ev.summary()
    twice = np.concatenate([want, want])
    twice['frame'][12:] += 3
    _records_equal(s['records'], twice)
    sums = 2 * np.sum([r[4] for r in ref], axis=0)
    assert [s['tp'], s['fp'], s['ignored'], s['n_gt'], s['frames']] == [sums[1], sums[2], sums[3], sums[4], 6]
    assert state.cpu().numpy().tolist() == [24, 0, 6, sums[4], sums[1], sums[2], sums[3], 0]
    assert s['ap'] == E.average_precision(twice['score'], twice['status'], int(sums[4]))
    tp_err = twice['lm_err'][twice['status'] == 1]
    assert s['lm_nme'] == pytest.approx(float(tp_err.mean()), rel=1e-12)
    ev.reset()
    assert ev.summary()['frames'] == 0 and ev.summary()['records'].shape == (0,)
    # an arena of 15 records takes the first call whole, 3 records of the second, and counts the other 9
    small = E.Evaluator(capacity=15, max_gt=3)
    rec_s, st_s = small._buffers(torch.device('cuda'))
    rec_s.fill_(0xEE)
    _append(dets, keep, None, B, slots, status, err, tally, rec_s, small.capacity, st_s)
    _append(dets, keep, None, B, slots, status, None, tally, rec_s, small.capacity, st_s)    # lm_err NULL: the records hold NaN
    assert st_s.cpu().numpy()[:3].tolist() == [15, 9, 6]
    got = rec_s.cpu().numpy().view(E.RECORD)
    _records_equal(got[:12], want)
    assert np.array_equal(got['status'][12:], want['status'][:3]) and np.isnan(got['lm_err'][12:]).all() and got['frame'][12:].tolist() == [3] * 3
    with pytest.raises(RuntimeError, match='9 records did not fit'):
        small.summary()


def _net(kind, dtype):
    net = getattr(D, kind)(synth.vgg19_standin(seed=0))
    synth.fill_params_(net, 11)
    # The seeded stand-in gives boxes of any shape, most of them with x2 < x1, which overlap nothing.  The last layer of the box head is
    # set so that every pixel's box is 17 x 13 pixels around it ((x - l) * 4 with l = (2, 1.5, -2, -1.5)): a copy shifted by up to two
    # pixels each way still has IoU >= 165 / 277 = 0.6, so the frames hold true positives, duplicates and ignored matches.
    with torch.no_grad():
        net.conv5_2_loc.weight.zero_()
        net.conv5_2_loc.bias.copy_(torch.tensor([2.0, 1.5, -2.0, -1.5]))
    net = net.cuda().eval()
    net.compute_dtype = dtype
    return net


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


@pytest.mark.parametrize('mode', ['topk', 'thresh'])
@pytest.mark.parametrize('dtype', ['f32', 'f16'])
@pytest.mark.parametrize('kind', ['DenseBox', 'DenseBoxLMLOC'])
def test_evaluate_batch_is_detect_batch_plus_the_restatement(kind, dtype, mode, monkeypatch):
    monkeypatch.delenv('DBX_GRAPH', raising=False)
    net = _net(kind, dtype)
    rs = np.random.RandomState(17)
    x = torch.from_numpy(rs.randint(0, 256, size=(3, 64, 64, 3)).astype(np.uint8)).cuda()
    top = net.detect_batch(x, K=10, max_batch=2)
    if mode == 'topk':
        kw = dict(K=10)
        ref = top
    else:
        best = np.sort(np.concatenate([d[:, 4] for d, _ in top]))[::-1]
        kw = dict(score_thresh=float(np.float32(best[12])), max_dets=64)            # a dozen pixels or more pass, at most 64 per frame
        ref = net.detect_batch_thresh(x, kw['score_thresh'], 64, max_batch=2)
    frames = [_gt_from(d, keep, rs) for d, keep in ref]
    lm = kind != 'DenseBox'
    gkw = dict(gt_ignore=[f[1] for f in frames], gt_quads=[f[2] for f in frames] if lm else None)
    boxes = [f[0] for f in frames]
    host = [R.match_frame(d, keep, f[0], f[1], f[2] if lm else None, 0.5) for (d, keep), f in zip(ref, frames)]
    want = R.records([(d, keep, h[0], h[3]) for (d, keep), h in zip(ref, host)])
    sums = np.sum([h[4] for h in host], axis=0)
    print(kind, dtype, mode, 'records', len(want), 'tally sums', sums.tolist())
    ev = E.Evaluator(capacity=4096, max_gt=8)
    assert net.evaluate_batch(x, boxes, evaluator=ev, max_batch=2, **kw, **gkw) is None
    s = ev.summary()
    _records_equal(s['records'], want)
    assert [s['tp'], s['fp'], s['ignored'], s['n_gt'], s['frames']] == [sums[1], sums[2], sums[3], sums[4], 3]
    assert s['tp'] > 0 and s['ignored'] > 0
    assert s['ap'] == E.average_precision(want['score'], want['status'], int(sums[4]))
    assert s['ap'] == pytest.approx(R.average_precision(want['score'], want['status'], int(sums[4])), rel=1e-12)
    assert (s['lm_nme'] is not None) == lm
    assert sorted(k[0] for k in net._detect_graphs if k[0] == 'evaluate') == ['evaluate'] * 2       # chunks of 2 and 1 frames
    # the same launches without the graph
    monkeypatch.setenv('DBX_GRAPH', '0')
    ev0 = E.Evaluator(capacity=4096, max_gt=8)
    net.evaluate_batch(x, boxes, evaluator=ev0, max_batch=2, **kw, **gkw)
    _records_equal(ev0.summary()['records'], want)
    monkeypatch.delenv('DBX_GRAPH')
    # a second call accumulates behind the first (replays only: no new capture, no warm-up run counted)
    n_graphs = len(net._detect_graphs)
    net.evaluate_batch(x, boxes, evaluator=ev, max_batch=2, **kw, **gkw)
    s2 = ev.summary()
    twice = np.concatenate([want, want])
    twice['frame'][len(want):] += 3
    _records_equal(s2['records'], twice)
    assert s2['frames'] == 6 and s2['tp'] == 2 * s['tp'] and s2['n_gt'] == 2 * s['n_gt'] and len(net._detect_graphs) == n_graphs
    # the other entries of the cache are not disturbed
    again = net.detect_batch(x, K=10, max_batch=2)
    assert all(np.array_equal(_bits(a), _bits(b)) and ka == kb for (a, ka), (b, kb) in zip(again, top))


def test_match_batch_on_host_results():
    net = _net('DenseBoxLMLOC', 'f16')
    rs = np.random.RandomState(23)
    x = torch.from_numpy(rs.randint(0, 256, size=(3, 64, 64, 3)).astype(np.uint8)).cuda()
    res = net.detect_batch(x, K=10)
    res.append((np.zeros((0, 13)), []))                                                  # an image without rows
    frames = [_gt_from(d, keep, rs) for d, keep in res[:2]] + [(np.zeros((0, 4)), np.zeros(0, np.uint8), np.zeros((0, 8)))]
    frames.append(frames[0])
    dets, keeps = [d for d, _ in res], [k for _, k in res]
    dets[1] = torch.from_numpy(dets[1]).cuda()                                            # a device result among host ones
    for quads in (True, False):
        out = E.match_batch(dets, keeps, [f[0] for f in frames], gt_ignore=[f[1] for f in frames],
                            gt_quads=[f[2] for f in frames] if quads else None, iou_thresh=0.5)
        assert len(out) == 4
        for (s, j, o, e), (d, keep), f in zip(out, res, frames):
            ws, wj, wo, we, _ = R.match_frame(d, keep, f[0], f[1], f[2] if quads else None, 0.5)
            assert s.dtype == np.int32 and s.tolist() == ws.tolist() and j.tolist() == wj.tolist() and _same_f64(o, wo)
            assert (e is None) == (not quads)
            if quads:
                m = ~np.isnan(we)
                assert np.array_equal(np.isnan(e), ~m) and np.allclose(e[m], we[m], rtol=1e-12, atol=0.0)
    assert sum(int((s == 1).sum()) for s, _, _, _ in out) > 0
