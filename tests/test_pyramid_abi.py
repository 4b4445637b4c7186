"""CPU-side checks of pyramid detection: the NumPy restatement tests/pyramid_ref.py (the oracle of the GPU tests) against
oracle.densebox_oracle.nms and on hand-made merges; dbx_merge_nms_batch refuses every bad argument on the host, with an error code and a
message naming the entry point, before anything is launched; detect_pyramid's argument checks and the level transform."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyramid_ref as P                                 # noqa: E402

from densebox_amd import _lib, resize                   # noqa: E402
from densebox_amd._lib import MergeXform                # noqa: E402
from oracle import densebox_oracle as O                 # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('dc', [5, 13])
def test_nms_stable_is_the_oracle_nms_on_every_random_case(dc):
    """Scores come from a continuous distribution and the generator asserts they are pairwise distinct, so the sort kind cannot
    matter and no case is left out."""
    cases = 0
    for seed in range(40):
        rs = np.random.RandomState(seed)
        n = int(rs.choice([1, 2, 7, 10, 30, 64, 65, 200, 500]))
        d = P.random_frame(rs, n, dc, span=float(rs.choice([240, 720, 1920])))
        assert len(set(d[:, 4].tolist())) == n
        for th in (0.0, 0.4, 0.7):
            assert P.nms_stable(d, th) == O.nms(d, th), (seed, n, th)
            cases += 1
    assert cases == 120


def test_nms_stable_tie_order_is_higher_row_index_first():
    far = lambda i: [1000.0 * i, 0.0, 1000.0 * i + 50, 20.0]          # noqa: E731  boxes that never overlap
    d = np.array([far(0) + [0.5], far(1) + [0.9], far(2) + [0.5], far(3) + [0.5], far(4) + [0.1]])
    assert P.nms_stable(d, 0.4) == [1, 3, 2, 0, 4]
    # two identical boxes with the same score: the higher row wins and suppresses the lower one
    d = np.array([[10.0, 10, 110, 50, 0.7], [500.0, 10, 600, 50, 0.2], [10.0, 10, 110, 50, 0.7]])
    assert P.nms_stable(d, 0.4) == [2, 1]
    # a tie between an overlapping pair decides WHICH survives
    d = np.array([[0.0, 0, 100, 40, 0.3], [5.0, 0, 105, 40, 0.3]])
    assert P.nms_stable(d, 0.4) == [1]
    # NaN scores sort last in NumPy, so they come first after [::-1], higher row first
    d = np.array([far(0) + [0.5], far(1) + [np.nan], far(2) + [0.9], far(3) + [np.nan]])
    assert P.nms_stable(d, 0.4) == [3, 1, 2, 0]


def test_merge_is_two_float64_operations_per_coordinate():
    rs = np.random.RandomState(3)
    a, b = P.random_frame(rs, 10, 13, span=720.0), P.random_frame(rs, 10, 13, span=480.0)
    xf = [(1920 / 720, 0.0, 420.0), (1920 / 480, 7.0, 0.0)]
    m = P.merge([a, b], xf)
    assert m.shape == (20, 13) and m.dtype == np.float64
    for l, (d, (s, ox, oy)) in enumerate(zip((a, b), xf)):
        for r in range(10):
            for col in range(13):
                want = d[r, col] if col == 4 else d[r, col] * s - (ox if col in (0, 2, 5, 7, 9, 11) else oy)
                assert m[l * 10 + r, col] == want, (l, r, col)
    assert np.array_equal(a[:, 4], m[:10, 4]) and np.array_equal(b[:, 4], m[10:, 4])


def test_hand_made_merges():
    """A 1080 x 1920 frame seen at 480 and at 720.  (a) One plate, found at both levels: after the map back the two boxes nearly
    coincide (IoU far above 0.4) and only the higher score survives.  (b) Boxes with IDENTICAL resized-frame coordinates at the two
    levels are different source boxes (4x and 2.67x the coordinates): both survive."""
    xf = [resize.level_xform(1080, 1920, 480), resize.level_xform(1080, 1920, 720)]
    assert xf[0] == (4.0, 0.0, 420.0) and xf[1] == (1920 / 720, 0.0, 420.0)
    plate = np.array([800.0, 500.0, 1000.0, 560.0])                       # source-frame box
    lv = []
    for (s, ox, oy), score, jitter in zip(xf, (0.6, 0.8), (1.0, -1.5)):
        box = (plate + np.array([ox, oy, ox, oy])) / s + jitter              # where that level sees it
        lv.append(np.array([list(box) + [score]]))
    m = P.merge(lv, xf)
    assert np.abs(m[:, :4] - plate).max() < 8.0
    assert P.nms_stable(m, 0.4) == [1]                                      # row 1 = level 1 (score 0.8); level 0's copy is suppressed
    same = np.array([[100.0, 150.0, 160.0, 170.0, 0.5]])
    m = P.merge([same, same], xf)
    assert not np.array_equal(m[0, :4], m[1, :4])
    assert P.nms_stable(m, 0.4) == [1, 0]                                   # equal scores: the higher row first; neither is suppressed


# ------------------------------------------------------------------------------------------------------------------- C ABI
def _call(L, levels=2, batch=3, K=10, det_cols=5, ptrs='ok', xf='ok', out_dets=0x3000, out_keep=0x4000, ws=0x5000, scale=None,
          off_x=None, off_y=None, null_level=None):
    vp = lambda a: None if a is None else C.c_void_p(a)       # noqa: E731
    nl, nb = max(1, levels), max(1, batch)
    if ptrs == 'ok':
        ptrs = (C.c_void_p * nl)(*[0x10000 * (l + 1) for l in range(nl)])
        if null_level is not None:
            ptrs[null_level] = None
    if xf == 'ok':
        xf = (MergeXform * (nl * nb))()
        for t in xf:
            t.scale, t.off_x, t.off_y = 1920 / 720, 0.0, 420.0
        bad = xf[nl * nb - 1]
        if scale is not None:
            bad.scale = scale
        if off_x is not None:
            bad.off_x = off_x
        if off_y is not None:
            bad.off_y = off_y
    return L.dbx_merge_nms_batch(ptrs, xf, levels, batch, K, det_cols, 0.4, vp(out_dets), vp(out_keep), vp(ws), None)


INF, NAN = float('inf'), float('nan')


@pytest.mark.parametrize('bad', [
    dict(levels=0), dict(levels=-2), dict(batch=0), dict(batch=-1), dict(K=0), dict(K=-5),
    dict(det_cols=4), dict(det_cols=6), dict(det_cols=12), dict(det_cols=0),
    dict(ptrs=None), dict(xf=None), dict(out_dets=None), dict(out_keep=None), dict(ws=None),
    dict(null_level=0), dict(null_level=1), dict(levels=4, null_level=3),
    dict(scale=0.0), dict(scale=-1.5), dict(scale=INF), dict(scale=NAN),
    dict(off_x=INF), dict(off_x=NAN), dict(off_y=-INF), dict(off_y=NAN),
    dict(levels=5, K=1000), dict(levels=4, K=1025), dict(levels=1, K=4097), dict(levels=3, K=2 ** 30),
])
def test_merge_nms_batch_rejects_bad_arguments_without_touching_the_gpu(bad):
    L = _lib.lib()
    rc = _call(L, **bad)
    assert rc == -1, bad
    msg = L.dbx_last_error()
    assert b'merge_nms_batch' in msg, msg
    with pytest.raises(RuntimeError, match='merge_nms_batch'):
        _lib.check(rc)


def test_merge_nms_batch_workspace_size():
    L = _lib.lib()
    f = L.dbx_merge_nms_batch_workspace_bytes
    for levels, batch, K in ((1, 1, 1), (3, 32, 10), (4, 5, 256), (1, 3, 1000), (4, 2, 1024), (4, 1, 300)):
        n = levels * K
        got = f(levels, batch, K)
        assert got > 0 and got % 256 == 0
        # the device records, and per frame: order (int32), suppression flags, 16 words per row on the LDS path
        need = levels * 8 + levels * batch * 24 + batch * (5 * n + (128 * n if n <= 1024 else 0))
        assert got >= need, (levels, batch, K, got, need)
        assert f(levels, batch + 1, K) > got
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (5, 1, 1000), (1, 1, 4097), (-1, 1, 1)):
        assert f(*bad) < 0, bad


def test_merge_xform_struct_matches_the_header_and_the_integration_doc():
    assert C.sizeof(MergeXform) == 24 and [(n, t) for n, t in MergeXform._fields_] == [('scale', C.c_double), ('off_x', C.c_double),
                                                                                          ('off_y', C.c_double)]
    src = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    m = re.search(r'typedef struct dbx_merge_xform \{\s*double (.*?);\s*\} dbx_merge_xform;', src)
    assert m and [s.strip() for s in m.group(1).split(',')] == ['scale', 'off_x', 'off_y']
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    m = re.search(r'class MergeXform\(C\.Structure\):.*?_fields_ = \[(.*?)\]\n', doc, re.S)
    assert m, 'INTEGRATION.md does not show MergeXform'
    names = re.findall(r"\('(\w+)', C\.(\w+)\)", m.group(1))
    assert [n for n, _ in names] == [f[0] for f in MergeXform._fields_] and all(getattr(C, t) is C.c_double for _, t in names)
    assert 'dbx_merge_nms_batch' in doc


# ------------------------------------------------------------------------------------------------- Python argument checks
def test_detect_pyramid_python_argument_checks():
    """Refused with a RuntimeError naming detect_pyramid before any device work (this test runs without a GPU)."""
    import densebox_amd as D
    from densebox_amd import decode as DC, synth
    net = D.DenseBoxLMLOC(synth.vgg19_standin(seed=0)).eval()
    frames = [np.zeros((48, 64, 3), np.uint8), np.zeros((64, 40, 3), np.uint8)]
    for sizes in ((), [], (64, 128, 192, 256, 320), (64, 64), (64, 128, 64), (66,), (64, 30), (0,), (-64,), (True,), True, 720,
                  (64.0,), ('64',), None, (np.bool_(True), 64)):
        with pytest.raises(RuntimeError, match='detect_pyramid: sizes'):
            net.detect_pyramid(frames, sizes=sizes)
    for mb in (0, -1, 2.5, True):
        with pytest.raises(RuntimeError, match='detect_pyramid: max_batch'):
            net.detect_pyramid(frames, sizes=(64,), max_batch=mb)
    for K in (0, -1, 1025, 2.0):
        with pytest.raises(RuntimeError, match='detect_pyramid: K'):
            DC.detect_pyramid(net, frames, sizes=(64, 128, 192, 256), K=K)
    with pytest.raises(RuntimeError, match='detect_pyramid.*uint8'):
        net.detect_pyramid(torch.zeros(2, 3, 64, 64))
    with pytest.raises(RuntimeError, match='detect_pyramid.*uint8'):
        DC.detect_pyramid(net, [torch.zeros(64, 64, 3)])
    with pytest.raises(RuntimeError, match='detect_pyramid.*uint8'):
        net.detect_pyramid([frames[0].astype(np.float32)])
    with pytest.raises(RuntimeError, match='detect_pyramid.*channels'):
        net.detect_pyramid(torch.zeros(2, 64, 64, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='detect_pyramid.*no images'):
        net.detect_pyramid([])
    for kind in ('DenseBox', 'DenseBoxLM', 'DenseBoxLMLOC'):
        assert callable(getattr(getattr(D, kind), 'detect_pyramid'))


@pytest.mark.parametrize('hw', [(1080, 1920), (1920, 1080), (333, 333), (97, 240), (240, 97), (301, 500), (500, 301), (1, 6), (7, 2)])
def test_level_xform_is_pad_geometrys_formula(hw):
    h, w = hw
    side, pad_x, pad_y = resize.pad_geometry(h, w)
    lu = abs(h - w) // 2
    assert (side, pad_x, pad_y) == (max(h, w), lu if h > w else 0, lu if h <= w else 0)
    for size in (160, 240, 480, 720, 1080):
        scale, ox, oy = resize.level_xform(h, w, size)
        assert isinstance(scale, float) and isinstance(ox, float) and isinstance(oy, float)
        assert scale == max(h, w) / size and (ox, oy) == (float(pad_x), float(pad_y))
        # a point of the frame, through pad_img + resize and back (the resize maps pixel centres; the map back is the documented
        # plain scaling the reference's viz applies, so only the scaling and the offsets are checked here)
        x, y = 0.3 * w, 0.8 * h
        xr, yr = (x + pad_x) / scale, (y + pad_y) / scale
        assert abs(xr * scale - ox - x) < 1e-9 and abs(yr * scale - oy - y) < 1e-9
