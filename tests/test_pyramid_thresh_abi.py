"""CPU-side checks of the threshold pyramid: dbx_thresh_rows_batch and dbx_merge_nms_thresh_batch are exported, declared and bound at ABI
version 13 and refuse every bad argument on the host, before anything is launched; their size functions; detect_pyramid's new argument
checks (no device work); the fetch-size helper; the NumPy restatement the GPU tests use against pyramid_ref on equal counts, and the
non-triviality of the cases the kernel tests run."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from densebox_amd import _lib
from densebox_amd._lib import MergeXform

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyramid_ref as P             # noqa: E402
import pyramid_thresh_ref as PT     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float('inf'), float('nan')
NEW = ['dbx_thresh_rows_batch', 'dbx_thresh_rows_batch_scratch_bytes', 'dbx_merge_nms_thresh_batch',
       'dbx_merge_nms_thresh_batch_workspace_bytes']


def test_new_entry_points_are_exported_declared_and_bound_at_version_13():
    L = _lib.lib()
    src = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, code), name + ' is not declared'
        assert name in _lib.SIGNATURES and name not in _lib.MISSING, name
        assert callable(getattr(L, name))
    assert int(re.search(r'#define\s+DBX_ABI_VERSION\s+(\d+)', src).group(1)) == L.dbx_version() == _lib.ABI_VERSION == 13
    assert re.search(r'\b13\s+additions only', src)
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert all(name in doc for name in NEW)


def _rows(L, score=0x1000, loc=0x2000, lm_heat=None, lm_loc=None, batch=2, rows=60, cols=60, t=0.5, max_dets=1024, dets=0x3000,
          det_cols=5, topk=0x4000, counts=0x7000, scratch=0x6000):
    vp = lambda a: None if a is None else C.c_void_p(a)       # noqa: E731
    return L.dbx_thresh_rows_batch(vp(score), vp(loc), vp(lm_heat), vp(lm_loc), batch, rows, cols, t, max_dets, vp(dets), det_cols,
                                   vp(topk), vp(counts), vp(scratch), None)


@pytest.mark.parametrize('bad', [
    dict(score=None), dict(loc=None), dict(dets=None), dict(topk=None), dict(counts=None), dict(scratch=None),
    dict(batch=0), dict(batch=-3),
    dict(rows=0), dict(cols=-1), dict(rows=65536, cols=65536),
    dict(max_dets=0), dict(max_dets=-1), dict(max_dets=4097),
    dict(t=NAN),
    dict(det_cols=4), dict(det_cols=6), dict(det_cols=13), dict(det_cols=12, lm_heat=0x8000),
])
def test_thresh_rows_batch_rejects_bad_arguments_without_touching_the_gpu(bad):
    L = _lib.lib()
    rc = _rows(L, **bad)
    assert rc == -1, bad
    assert b'thresh_rows_batch' in L.dbx_last_error()
    with pytest.raises(RuntimeError, match='thresh_rows_batch'):
        _lib.check(rc)


def _merge(L, levels=2, batch=3, max_dets=100, det_cols=5, nms=0.4, dets='ok', cnts='ok', xf='ok', out_dets=0x3000, out_keep=0x4000,
           out_counts=0x6000, ws=0x5000, scale=None, off_x=None, off_y=None, null_dets=None, null_counts=None):
    vp = lambda a: None if a is None else C.c_void_p(a)       # noqa: E731
    nl, nb = max(1, levels), max(1, batch)
    if dets == 'ok':
        dets = (C.c_void_p * nl)(*[0x10000 * (l + 1) for l in range(nl)])
        if null_dets is not None:
            dets[null_dets] = None
    if cnts == 'ok':
        cnts = (C.c_void_p * nl)(*[0x100000 * (l + 1) for l in range(nl)])
        if null_counts is not None:
            cnts[null_counts] = None
    if xf == 'ok':
        xf = (MergeXform * (nl * nb))()
        for t in xf:
            t.scale, t.off_x, t.off_y = 1920 / 720, 0.0, 420.0
        last = xf[nl * nb - 1]
        if scale is not None:
            last.scale = scale
        if off_x is not None:
            last.off_x = off_x
        if off_y is not None:
            last.off_y = off_y
    return L.dbx_merge_nms_thresh_batch(dets, cnts, xf, levels, batch, max_dets, det_cols, nms, vp(out_dets), vp(out_keep),
                                        vp(out_counts), vp(ws), None)


@pytest.mark.parametrize('bad', [
    dict(levels=0), dict(levels=-2), dict(batch=0), dict(batch=-1),
    dict(max_dets=0), dict(max_dets=-5), dict(max_dets=4097), dict(levels=1, max_dets=2 ** 30),
    dict(levels=5, max_dets=1000), dict(levels=4, max_dets=1025), dict(levels=2, max_dets=2049), dict(levels=4097, max_dets=1),
    dict(det_cols=4), dict(det_cols=6), dict(det_cols=12), dict(det_cols=0),
    dict(dets=None), dict(cnts=None), dict(xf=None), dict(out_dets=None), dict(out_keep=None), dict(out_counts=None), dict(ws=None),
    dict(null_dets=0), dict(null_dets=1), dict(null_counts=0), dict(null_counts=1), dict(levels=4, null_dets=3),
    dict(levels=4, null_counts=3),
    dict(scale=0.0), dict(scale=-1.5), dict(scale=INF), dict(scale=NAN),
    dict(off_x=INF), dict(off_x=NAN), dict(off_y=-INF), dict(off_y=NAN),
    dict(nms=NAN), dict(nms=-0.1),
])
def test_merge_nms_thresh_batch_rejects_bad_arguments_without_touching_the_gpu(bad):
    L = _lib.lib()
    rc = _merge(L, **bad)
    assert rc == -1, bad
    assert b'merge_nms_thresh_batch' in L.dbx_last_error()
    with pytest.raises(RuntimeError, match='merge_nms_thresh_batch'):
        _lib.check(rc)


def test_size_functions():
    L = _lib.lib()
    f = L.dbx_thresh_rows_batch_scratch_bytes
    for ok in ((1, 60, 60, 1), (32, 270, 480, 1024), (5, 25, 33, 4096)):
        assert f(*ok) > 0
    for bad in ((0, 60, 60, 10), (1, 0, 60, 10), (1, 60, -1, 10), (1, 60, 60, 0), (1, 60, 60, 4097)):
        assert f(*bad) == -1, bad
    g = L.dbx_merge_nms_thresh_batch_workspace_bytes
    for levels, batch, cap in ((1, 1, 1), (3, 32, 1024), (4, 5, 1024), (1, 3, 4096), (2, 2, 2048), (4, 1, 300), (4096, 1, 1)):
        n = levels * cap
        got = g(levels, batch, cap)
        assert got > 0 and got % 256 == 0
        # the device records, and per frame the NMS order and the n x ceil(n / 64)-word suppression matrix
        need = levels * 16 + levels * batch * 24 + batch * (4 * n + n * ((n + 63) // 64) * 8)
        assert got >= need, (levels, batch, cap, got, need)
        assert g(levels, batch + 1, cap) > got
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (5, 1, 1000), (1, 1, 4097), (-1, 1, 1), (2, 1, 2049), (1, -1, 10)):
        assert g(*bad) == -1, bad


def test_detect_pyramid_threshold_argument_checks_fail_before_any_device_work():
    import densebox_amd as D
    from densebox_amd import decode as DC, synth
    net = D.DenseBoxLMLOC(synth.vgg19_standin(seed=0)).eval()
    frames = [np.zeros((48, 64, 3), np.uint8), np.zeros((64, 40, 3), np.uint8)]
    for bad in (NAN, INF, -INF, '0.5', True, np.bool_(False), [0.5]):
        with pytest.raises(RuntimeError, match='detect_pyramid: score_thresh'):
            net.detect_pyramid(frames, sizes=(64,), score_thresh=bad)
    for bad in (0, -1, 4097, 10.0, '10', True, None):
        with pytest.raises(RuntimeError, match='detect_pyramid: max_dets'):
            DC.detect_pyramid(net, frames, sizes=(64,), score_thresh=0.5, max_dets=bad)
    for sizes, cap in (((64, 128, 192, 256), 1025), ((64, 128), 2049), ((64, 128, 192), 4096)):
        with pytest.raises(RuntimeError, match=r'detect_pyramid: len\(sizes\)=%d levels x max_dets=%d' % (len(sizes), cap)):
            net.detect_pyramid(frames, sizes=sizes, score_thresh=0.5, max_dets=cap)
    with pytest.raises(RuntimeError, match='detect_pyramid: K=7 and score_thresh'):
        net.detect_pyramid(frames, sizes=(64,), K=7, score_thresh=0.5)
    # the other checks still come first or hold alike
    with pytest.raises(RuntimeError, match='detect_pyramid: sizes'):
        net.detect_pyramid(frames, sizes=(66,), score_thresh=0.5)
    with pytest.raises(RuntimeError, match='detect_pyramid: max_batch'):
        net.detect_pyramid(frames, sizes=(64,), max_batch=0, score_thresh=0.5)
    with pytest.raises(RuntimeError, match='detect_pyramid.*uint8'):
        net.detect_pyramid([frames[0].astype(np.float32)], sizes=(64,), score_thresh=0.5)


def _counts_words(pairs):
    """the merge's count words for hand-made pairs[b][l] = (n, pixels above the threshold)"""
    pairs = np.asarray(pairs, np.int32)
    m = pairs[:, :, 0].sum(axis=1)
    return np.concatenate([pairs.reshape(-1), [0], np.cumsum(m)]).astype(np.int32)


def test_fetch_bytes_and_unpack_on_hand_made_counts():
    from densebox_amd import decode as DC
    for dc in (5, 13):
        for pairs in ([[(3, 9), (0, 0)], [(0, 0), (0, 0)], [(2, 2), (4, 5000)]],          # an empty frame between two others
                      [[(0, 0)] * 3],                                                      # a call without a row
                      [[(0, 1)], [(0, 0)]],
                      [[(1024, 1024)] * 4, [(1, 1), (0, 0), (1024, 90000), (7, 7)]]):
            c = _counts_words(pairs)
            b, levels = len(pairs), len(pairs[0])
            assert c.shape[0] == DC._pyramid_counts_words(b, levels)
            m = [sum(n for n, _ in fr) for fr in pairs]
            total = sum(m)
            nbytes = DC._pyramid_thresh_fetch_bytes(c, levels, dc)
            assert nbytes == total * dc * 8 + (total + b) * 4
            # an arena as the kernel packs it: row r of the call holds r in every column; list of frame i: count 1, row m_i - 1
            rows = np.repeat(np.arange(total, dtype=np.float64)[:, None], dc, axis=1)
            lists, at = np.zeros(total + b, np.int32), 0
            for i, mi in enumerate(m):
                if mi:
                    lists[at], lists[at + 1] = 1, mi - 1
                at += mi + 1
            arena = np.concatenate([rows.view(np.uint8).reshape(-1), lists.view(np.uint8)])
            assert arena.shape[0] == nbytes
            got = DC._unpack_pyramid_thresh(c, arena, levels, dc, True)
            assert len(got) == b
            first = 0
            for (d, keep, lv), mi, fr in zip(got, m, pairs):
                assert d.shape == (mi, dc) and d.dtype == np.float64
                assert d[:, 0].tolist() == list(range(first, first + mi))
                assert keep == ([mi - 1] if mi else [])
                assert lv.tolist() == [n for n, _ in fr]
                first += mi
            assert all(len(r) == 2 for r in DC._unpack_pyramid_thresh(c, arena, levels, dc, False))


@pytest.mark.parametrize('dc', [5, 13])
def test_restatement_is_pyramid_ref_when_all_counts_are_equal(dc):
    rs = np.random.RandomState(dc)
    for levels, K in ((1, 10), (2, 64), (3, 100), (4, 33)):
        for kind in range(4):
            frame = PT.frame_levels(rs, kind, levels, K, dc)
            xf = PT.frame_xforms(kind, 1, levels)
            union, keep = PT.merge_nms(frame, [K] * levels, xf, K)
            want = P.merge(frame, xf)
            assert union.tobytes() == want.tobytes() and union.shape == (levels * K, dc)
            assert keep == P.nms_stable(want, 0.4)
            # fewer rows: the first n of every level, as if the levels had been cut before the merge; counts are clamped
            counts = [K + 5, 0, K // 2, -3][:levels]
            union, keep = PT.merge_nms(frame, counts, xf, K, 0.7)
            cut = [f[:PT.clamp(n, K)] for f, n in zip(frame, counts)]
            assert union.tobytes() == P.merge(cut, xf).tobytes() and keep == P.nms_stable(P.merge(cut, xf), 0.7)
    union, keep = PT.merge_nms(PT.frame_levels(rs, 0, 3, 10, dc), [0, 0, 0], PT.frame_xforms(0, 0, 3), 10)
    assert union.shape == (0, dc) and keep == []


def test_the_kernel_cases_are_not_trivial_under_the_restatement():
    """what tests/test_hip_pyramid_thresh.py asserts on the GPU holds for the NumPy restatement alone: in every case rows of two levels
    meet (where there are two levels), a row is suppressed and more than one is kept"""
    for dc in (5, 13):
        for batch in (1, 3, 5):
            for levels in (1, 2, 3, 4):
                frames, counts, xforms = PT.grid_case(levels, batch, dc)
                two, nms = PT.non_trivial(frames, counts, xforms, 100)
                assert nms and (two or levels == 1), (dc, batch, levels)
                if batch >= 3:
                    assert counts[1] == [0] * levels and sum(counts[0]) > 0 and sum(counts[2]) > 0      # empty between non-empty
    for which in (0, 1):
        frames, counts, xforms, cap = PT.full_case(which)
        assert sum(counts[0]) == 4096
        two, nms = PT.non_trivial(frames, counts, xforms, cap)
        assert nms and (two or which == 1)
