"""The tile stitch on the GPU: dbx_tile_rows_batch and dbx_tile_nms_batch against tests/tiles_ref.py.  Rows, marks, counts, prefix,
keep lists and tile indices are bitwise the restatement's, the keep lists also dbx_nms_large's on every frame's packed rows, and nothing
is written outside them (sentinels around every buffer and in their unwritten parts)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiles_ref as R                                   # noqa: E402

from densebox_amd import _lib, tiles as T               # noqa: E402
from densebox_amd._lib import check, ptr, stream_ptr    # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 512                    # sentinel bytes in front of and behind every buffer


def _guarded(nbytes):
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    return buf, buf[GUARD:GUARD + nbytes]


def _guards_intact(named):
    for name, g in named.items():
        a = g.cpu().numpy()
        assert (a[:GUARD] == 0xA5).all() and (a[-GUARD:] == 0xA5).all(), name + ': written outside the buffer'


def _up256(v):
    return (v + 255) // 256 * 256


def _keep_list(k):
    return [int(v) for v in k[1:1 + int(k[0])]]


def _nms_large(d, th):
    n, dc = d.shape
    L = _lib.lib()
    t = torch.from_numpy(np.ascontiguousarray(d)).cuda()
    keep = torch.zeros(n + 1, dtype=torch.int32, device='cuda')
    scratch = torch.empty(L.dbx_nms_large_scratch_bytes(n), dtype=torch.uint8, device='cuda')
    check(L.dbx_nms_large(ptr(t), n, dc, th, ptr(keep), ptr(scratch), stream_ptr()))
    return _keep_list(keep.cpu().numpy())


def _stitch_abi(table, rows, counts, frames, rule, chunk, thresh=0.4, behind=False):
    """The two entry points on rows [n, rpt, dc] (tile coordinates) and device count words counts [n] (None: the top-K mode), the rows
    launch issued over `chunk` tiles at a time from ONE reused device buffer (stream order alone keeps a chunk's rows alive), with
    sentinels around every buffer.  Checks the staging area and the outputs against the restatement and returns its per-frame results."""
    n, rpt, dc = rows.shape
    table = np.ascontiguousarray(table.astype(T.TILE_DTYPE))
    L = _lib.lib()
    tdev = torch.from_numpy(table.view(np.uint8).copy()).cuda()
    ns = L.dbx_tile_stage_bytes(n, rpt, dc)
    assert ns == _up256(n * 8) + _up256(n * rpt * 4) + _up256(n * rpt * dc * 8)
    g_s, stage = _guarded(ns)
    g_r, rbuf = _guarded(chunk * rpt * dc * 8)
    g_c, cbuf = _guarded(chunk * 8)
    for t0 in range(0, n, chunk):
        k = min(chunk, n - t0)
        rbuf[:k * rpt * dc * 8].copy_(torch.from_numpy(rows[t0:t0 + k].reshape(-1).view(np.uint8).copy()))
        if counts is not None:
            pair = np.stack([counts[t0:t0 + k], counts[t0:t0 + k] + 11], axis=1).astype(np.int32)
            cbuf[:k * 8].copy_(torch.from_numpy(pair.reshape(-1).view(np.uint8).copy()))
        check(L.dbx_tile_rows_batch(ptr(rbuf), ptr(cbuf) if counts is not None else None, table.ctypes.data, ptr(tdev), n, t0, k, rpt, dc,
                                    rule, ptr(stage), stream_ptr()))
    max_tiles = int(np.bincount(table['frame'], minlength=frames).max())
    nws = L.dbx_tile_nms_batch_workspace_bytes(frames, max_tiles, rpt)
    nmax = max_tiles * rpt
    assert nws == frames * (_up256(nmax * 4) + _up256(nmax * ((nmax + 63) // 64) * 8))
    g_w, ws = _guarded(nws)
    nrow = n * rpt
    g_d, od = _guarded(nrow * dc * 8 + ((nrow + frames) * 4 if behind else 0))
    g_k, ok = _guarded((nrow + frames) * 4)
    g_t, ot = _guarded(nrow * 4)
    g_n, oc = _guarded((2 * n + frames + 1) * 4)
    check(L.dbx_tile_nms_batch(table.ctypes.data, ptr(tdev), n, frames, rpt, dc, thresh, ptr(stage), ptr(od), ptr(od if behind else ok),
                               ptr(ot), ptr(oc), ptr(ws), stream_ptr()))
    torch.cuda.synchronize()
    _guards_intact(dict(stage=g_s, rows=g_r, counts=g_c, workspace=g_w, out_dets=g_d, out_keep=g_k, out_tile=g_t, out_counts=g_n))
    assert tdev.cpu().numpy().tobytes() == table.tobytes(), 'the device table was written'

    want_stage, want = R.stitch(rows, counts, table, frames, rpt, rule, thresh)
    # ---- the staging area: pairs, marks and rows of the delivered slots, sentinels in the others
    s = stage.cpu().numpy()
    o_m, o_r = _up256(n * 8), _up256(n * 8) + _up256(n * rpt * 4)
    pairs = s[:n * 8].view(np.int32).reshape(n, 2)
    marks = s[o_m:o_m + n * rpt * 4].reshape(n, rpt * 4)
    srows = s[o_r:o_r + n * rpt * dc * 8].reshape(n, rpt * dc * 8)
    for t, (m, k) in enumerate(want_stage):
        cnt = m.shape[0]
        assert pairs[t].tolist() == [cnt, int(k.sum())], (t, pairs[t], cnt, int(k.sum()))
        assert marks[t, :cnt * 4].view(np.int32).tolist() == k.tolist(), (t, 'marks')
        assert srows[t, :cnt * dc * 8].tobytes() == m.tobytes(), (t, 'mapped rows')
        assert (marks[t, cnt * 4:] == 0xA5).all() and (srows[t, cnt * dc * 8:] == 0xA5).all(), (t, 'written beyond the delivered rows')
    # ---- the outputs
    c = oc.cpu().numpy().view(np.int32)
    assert c.tolist() == R.pairs_and_prefix(want_stage, want).tolist()
    prefix = c[2 * n:]
    total = int(prefix[frames])
    d = od.cpu().numpy()
    kb = d[total * dc * 8:] if behind else ok.cpu().numpy()
    assert (kb[(total + frames) * 4:] == 0xA5).all(), 'out_keep: written behind the lists'
    if behind:
        assert (ok.cpu().numpy() == 0xA5).all()
    else:
        assert (d[total * dc * 8:] == 0xA5).all(), 'out_dets: written behind the packed rows'
    tl = ot.cpu().numpy()
    assert (tl[total * 4:] == 0xA5).all(), 'out_tile: written behind the packed rows'
    got_rows = d[:total * dc * 8].view(np.float64).reshape(total, dc)
    lists = kb[:(total + frames) * 4].view(np.int32)
    tile_of = tl[:total * 4].view(np.int32)
    for b, (wr, wk, wt) in enumerate(want):
        p, m = int(prefix[b]), wr.shape[0]
        assert got_rows[p:p + m].tobytes() == wr.tobytes(), (b, 'packed rows')
        assert tile_of[p:p + m].tolist() == wt.tolist(), (b, 'tile indices')
        keep = _keep_list(lists[p + b:p + b + m + 1])
        assert lists[p + b] == len(wk) and keep == wk, (b, 'keep list', keep[:8], wk[:8])
        if m:
            assert keep == _nms_large(wr, thresh), (b, 'dbx_nms_large')
    return want_stage, want


def _shares(name, stage, want):
    delivered = sum(m.shape[0] for m, _ in stage)
    owned = sum(int(k.sum()) for _, k in stage)
    kept = sum(len(k) for _, k, _ in want)
    print('%s: %d rows delivered, %d owned, %d dropped, %d kept by the NMS' % (name, delivered, owned, delivered - owned, kept))
    return delivered, owned, kept


@pytest.mark.parametrize('dc', [5, 13])
@pytest.mark.parametrize('case', sorted(R.CASES))
def test_topk_mode_both_rules_and_every_chunking(case, dc):
    per_frame, rpt = R.CASES[case]
    table = R.case_table(per_frame)
    n = table.shape[0]
    rows = R.case_rows(7 * dc + n, table, rpt, dc)
    for rule in (R.CORE, R.NONE):
        first = None
        for chunk in sorted({1, min(4, n), n}):
            stage, want = _stitch_abi(table, rows, None, len(per_frame), rule, chunk, behind=(chunk == n))
            sig = [(r.tobytes(), k) for r, k, _ in want]
            assert first is None or sig == first
            first = sig
        delivered, owned, kept = _shares('%s dc %d rule %d' % (case, dc, rule), stage, want)
        assert delivered == n * rpt
        if rule == R.NONE:
            assert owned == delivered
            if case == '1x64x64':
                assert want[0][0].shape[0] == 4096                   # the NMS's bound
        elif n > 1:
            assert 0 < owned < delivered and kept < owned            # rows are dropped by the rule and suppressed by the NMS


@pytest.mark.parametrize('dc', [5, 13])
def test_a_box_on_a_core_boundary_survives_once(dc):
    """the same source box delivered by two neighbouring tiles, its centre exactly on their boundary: under CORE only the right-hand
    tile's copy is packed (the core is half-open: the boundary belongs to the higher tile); under NONE both are, and the NMS keeps one"""
    table = R.case_table((6,))
    rows = R.case_rows(3, table, 10, dc, nan=False)
    pair = (0, 1)                                                     # tiles 0 and 1 of the first tile row: row 0 and row 1
    box = R.map_rows(rows[0, 0:1], table[0])
    assert box.tobytes() == R.map_rows(rows[1, 1:2], table[1]).tobytes() and box[0, 0] + box[0, 2] == table[0]['hi2x']
    for rule, copies in ((R.CORE, 1), (R.NONE, 2)):
        _, want = _stitch_abi(table, rows, None, 1, rule, 4)
        packed, keep, tile_of = want[0]
        at = [i for i in range(packed.shape[0]) if packed[i].tobytes() == box[0].tobytes()]
        assert len(at) == copies and [int(tile_of[i]) for i in at] == list(pair)[-copies:]
        assert len([i for i in at if i in keep]) == 1


@pytest.mark.parametrize('dc', [5, 13])
@pytest.mark.parametrize('case', sorted(R.CASES))
def test_threshold_mode_clamps_the_device_counts(case, dc):
    per_frame, rpt = R.CASES[case]
    table = R.case_table(per_frame, scale=0.5)                        # magnified windows: tile coordinates are halved
    n = table.shape[0]
    rows = R.case_rows(11 * dc + n, table, rpt, dc)
    counts = R.case_counts(n + dc, n, rpt)
    assert counts.min() <= 0 and (n < 3 or (counts.min() < 0 and counts.max() > rpt))
    for rule in (R.CORE, R.NONE):
        for chunk in sorted({1, min(4, n), n}):
            stage, want = _stitch_abi(table, rows, counts, len(per_frame), rule, chunk, thresh=0.3, behind=(chunk == 1))
        _shares('%s dc %d rule %d threshold mode' % (case, dc, rule), stage, want)
        assert [m.shape[0] for m, _ in stage] == [R.clamp(c, rpt) for c in counts]


def test_a_call_without_an_owned_row_writes_counts_and_empty_lists():
    table = R.case_table((1, 6, 2))
    rows = R.case_rows(5, table, 10, 5)
    _, want = _stitch_abi(table, rows, np.zeros(9, np.int32), 3, R.CORE, 4)
    assert all(r.shape[0] == 0 and k == [] for r, k, _ in want)
    rows[:, :, 0] = np.nan                                            # every box NaN: delivered, none owned
    stage, want = _stitch_abi(table, rows, None, 3, R.CORE, 9)
    assert all(m.shape[0] == 10 and k.sum() == 0 for m, k in stage) and all(r.shape[0] == 0 for r, _, _ in want)
    _, want = _stitch_abi(table, rows, None, 3, R.NONE, 9)            # ... and all of them under NONE, NaN passing through the map
    assert [r.shape[0] for r, _, _ in want] == [10, 60, 20]


def test_merge_host_results_is_the_restatement():
    table = R.case_table((1, 6, 2)).astype(T.TILE_DTYPE)
    rows = R.case_rows(9, table, 10, 13)
    counts = [10, 0, 3, 10, 7, 1, 10, 2, 9]
    res = [rows[t, :c] for t, c in enumerate(counts)]
    got = T.merge_host_results(res, table, 3, rule='core', nms_thresh=0.4, with_tiles=True)
    _, want = R.stitch(rows, counts, table, 3, 10, R.CORE, 0.4)
    first = [0, 1, 7]
    for b, ((gd, gk, gt, gp), (wd, wk, wt)) in enumerate(zip(got, want)):
        assert gd.tobytes() == wd.tobytes() and gk == wk and (gt + first[b]).tolist() == wt.tolist()
        assert gp.tobytes() == table[table['frame'] == b].tobytes()
