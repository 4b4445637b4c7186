"""CPU-side checks of the evaluation entry points (dbx_match_gt_batch, dbx_eval_append, densebox_amd.evaluate): the new symbols are
declared, bound and exported without an ABI bump; dbx_eval_record has the documented layout; every bad argument is refused on the host,
with an error code and a message naming the entry point, before anything is launched; the Python argument checks run before the device
is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from densebox_amd import _lib, evaluate as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['dbx_match_gt_batch', 'dbx_eval_append']
NAN = float('nan')


def test_new_entry_points_are_exported_declared_and_bound_without_a_bump():
    L = _lib.lib()
    src = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, code), name + ' is not declared'
        assert name in _lib.SIGNATURES and name not in _lib.MISSING, name
        assert callable(getattr(L, name))
    assert re.search(r'\bdbx_eval_record\b', code)
    assert int(re.search(r'#define\s+DBX_ABI_VERSION\s+(\d+)', src).group(1)) == L.dbx_version() == _lib.ABI_VERSION == 13
    assert re.search(r'without a bump: dbx_eval_record, dbx_match_gt_batch, dbx_eval_append', src)
    assert re.search(r'without a bump: dbx_crop_frame, dbx_plate_crops_batch', src)          # the earlier sentence stays
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert all(name in doc for name in NEW + ['dbx_eval_record'])


def test_eval_record_layout_matches_the_header():
    R = _lib.EvalRecord
    assert C.sizeof(R) == 24
    assert (R.score.offset, R.lm_err.offset, R.status.offset, R.frame.offset) == (0, 8, 16, 20)
    assert E.RECORD.itemsize == 24 and [E.RECORD.fields[n][1] for n in ('score', 'lm_err', 'status', 'frame')] == [0, 8, 16, 20]
    src = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    m = re.search(r'typedef struct dbx_eval_record \{(.*?)\} dbx_eval_record;', src, re.S)
    body = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
    assert re.findall(r'(\w+)\s+(\w+);', body) == [('double', 'score'), ('double', 'lm_err'), ('int32_t', 'status'), ('int32_t', 'frame')]


def _vp(a):
    return None if a is None else C.c_void_p(a)


def _match(L, dets=0x1000, det_cols=13, det_rows=80, keep=0x2000, prefix=None, batch=2, slots=8, gt=0x3000, gt_cols=12, gt_counts=0x4000,
           gt_ignore=0x5000, max_gt=4, iou_thresh=0.5, status=0x6000, gt_index=0x7000, iou=0x8000, lm_err=0x9000, tally=0xa000):
    return L.dbx_match_gt_batch(_vp(dets), det_cols, det_rows, _vp(keep), _vp(prefix), batch, slots, _vp(gt), gt_cols, _vp(gt_counts),
                                _vp(gt_ignore), max_gt, iou_thresh, _vp(status), _vp(gt_index), _vp(iou), _vp(lm_err), _vp(tally), None)


def _append(L, dets=0x1000, det_cols=13, det_rows=80, keep=0x2000, prefix=None, batch=2, slots=8, status=0x6000, lm_err=0x9000,
            tally=0xa000, records=0xb000, capacity=100, state=0xc000):
    return L.dbx_eval_append(_vp(dets), det_cols, det_rows, _vp(keep), _vp(prefix), batch, slots, _vp(status), _vp(lm_err), _vp(tally),
                             _vp(records), capacity, _vp(state), None)


@pytest.mark.parametrize('bad', [
    dict(dets=None), dict(keep=None), dict(gt=None), dict(gt_counts=None), dict(status=None), dict(gt_index=None), dict(iou=None),
    dict(tally=None),
    dict(det_cols=4, lm_err=None), dict(det_cols=12, lm_err=None), dict(det_cols=0, lm_err=None),
    dict(gt_cols=5, lm_err=None), dict(gt_cols=8, lm_err=None), dict(gt_cols=0, lm_err=None),
    dict(det_cols=5), dict(gt_cols=4), dict(det_cols=5, gt_cols=4),                    # lm_err without 13 / 12
    dict(slots=0), dict(slots=4097), dict(slots=-1),
    dict(max_gt=0), dict(max_gt=1025), dict(max_gt=-4),
    dict(batch=-1),
    dict(iou_thresh=NAN),
    dict(det_rows=15), dict(det_rows=-1), dict(det_rows=-1, prefix=0xd000),          # slot layout needs batch * slots rows
])
def test_match_gt_batch_rejects_bad_arguments_without_touching_the_gpu(bad):
    L = _lib.lib()
    rc = _match(L, **bad)
    assert rc == -1, bad
    msg = L.dbx_last_error()
    assert b'match_gt_batch' in msg, msg
    with pytest.raises(RuntimeError, match='match_gt_batch'):
        _lib.check(rc)


@pytest.mark.parametrize('bad', [
    dict(dets=None), dict(keep=None), dict(status=None), dict(tally=None), dict(records=None), dict(state=None),
    dict(det_cols=4), dict(det_cols=14),
    dict(slots=0), dict(slots=4097),
    dict(batch=-1),
    dict(capacity=-1),
    dict(det_rows=15), dict(det_rows=-1),
])
def test_eval_append_rejects_bad_arguments_without_touching_the_gpu(bad):
    L = _lib.lib()
    rc = _append(L, **bad)
    assert rc == -1, bad
    msg = L.dbx_last_error()
    assert b'eval_append' in msg, msg
    with pytest.raises(RuntimeError, match='eval_append'):
        _lib.check(rc)


def test_empty_calls_are_no_ops():
    L = _lib.lib()
    none = dict(dets=None, keep=None, status=None, tally=None)
    assert _match(L, batch=0, det_rows=0, gt=None, gt_counts=None, gt_ignore=None, gt_index=None, iou=None, lm_err=None, **none) == 0
    assert _match(L, batch=0) == 0
    assert _append(L, batch=0, det_rows=0, lm_err=None, records=None, state=None, **none) == 0
    assert _append(L, batch=0) == 0


def test_evaluator_argument_checks():
    for bad in (0, -5, 1.5, True, None):
        with pytest.raises(RuntimeError, match='capacity'):
            E.Evaluator(capacity=bad)
    for bad in (0, 1025, 2.0, True):
        with pytest.raises(RuntimeError, match='max_gt'):
            E.Evaluator(max_gt=bad)
    for bad in (NAN, 'half', None, True):
        with pytest.raises(RuntimeError, match='iou_thresh'):
            E.Evaluator(iou_thresh=bad)
    ev = E.Evaluator(capacity=10, iou_thresh=0.3, max_gt=1024)
    assert (ev.capacity, ev.iou_thresh, ev.max_gt) == (10, 0.3, 1024) and ev._state is None          # nothing allocated yet
    ev.reset()
    s = ev.summary()                                                                                # an unused evaluator: all zero, AP NaN
    assert s['frames'] == s['tp'] == s['fp'] == s['ignored'] == s['n_gt'] == 0 and np.isnan(s['ap']) and s['lm_nme'] is None
    assert s['scores'].shape == s['precision'].shape == s['recall'].shape == (0,)
    assert E.Evaluator().serial != E.Evaluator().serial


def test_match_batch_python_argument_checks():
    d5, d13 = np.zeros((2, 5)), np.zeros((2, 13))
    gt = [np.zeros((1, 4))]
    with pytest.raises(RuntimeError, match='one entry per image'):
        E.match_batch([d5], [[0], [1]], gt)
    with pytest.raises(RuntimeError, match='one entry per image'):
        E.match_batch([], [], [])
    with pytest.raises(RuntimeError, match='gt_boxes'):
        E.match_batch([d5], [[0]], [gt[0], gt[0]])
    with pytest.raises(RuntimeError, match=r'gt_boxes\[0\]'):
        E.match_batch([d5], [[0]], [np.zeros((1, 5))])
    with pytest.raises(RuntimeError, match='more than max_gt'):
        E.match_batch([d5], [[0]], [np.zeros((1025, 4))])
    with pytest.raises(RuntimeError, match='gt_ignore'):
        E.match_batch([d5], [[0]], gt, gt_ignore=[[0, 1]])
    with pytest.raises(RuntimeError, match='gt_quads'):
        E.match_batch([d13], [[0]], gt, gt_quads=[np.zeros((1, 7))])
    with pytest.raises(RuntimeError, match='13-column'):
        E.match_batch([d5], [[0]], gt, gt_quads=[np.zeros((1, 8))])
    with pytest.raises(RuntimeError, match='all alike'):
        E.match_batch([d5, d13], [[0], [0]], gt * 2)
    with pytest.raises(RuntimeError, match='all alike'):
        E.match_batch([np.zeros((2, 6))], [[0]], gt)
    with pytest.raises(RuntimeError, match='outside'):
        E.match_batch([d5], [[2]], gt)
    with pytest.raises(RuntimeError, match='outside'):
        E.match_batch([d5], [[-1]], gt)
    with pytest.raises(RuntimeError, match='exceed'):
        E.match_batch([np.zeros((4097, 5))], [[0]], gt)
    with pytest.raises(RuntimeError, match='iou_thresh'):
        E.match_batch([d5], [[0]], gt, iou_thresh=NAN)


def test_evaluate_batch_python_argument_checks():
    """Everything is refused before the device is touched: this machine has none."""
    import densebox_amd as D
    from densebox_amd import synth
    box = D.DenseBox(synth.vgg19_standin(seed=0)).eval()
    lm = D.DenseBoxLMLOC(synth.vgg19_standin(seed=0)).eval()
    frames = torch.zeros(2, 64, 64, 3, dtype=torch.uint8)
    gt = [np.zeros((1, 4)), np.zeros((0, 4))]
    ev = E.Evaluator(capacity=16, max_gt=2)
    with pytest.raises(TypeError, match='evaluator'):                      # keyword-only, no default
        box.evaluate_batch(frames, gt)
    with pytest.raises(RuntimeError, match='evaluator'):
        box.evaluate_batch(frames, gt, evaluator=None)
    with pytest.raises(RuntimeError, match='both given'):
        box.evaluate_batch(frames, gt, evaluator=ev, K=20, score_thresh=0.5)
    with pytest.raises(RuntimeError, match='score_thresh'):
        box.evaluate_batch(frames, gt, evaluator=ev, score_thresh=NAN)
    with pytest.raises(RuntimeError, match='max_dets'):
        box.evaluate_batch(frames, gt, evaluator=ev, score_thresh=0.5, max_dets=4097)
    for bad in (0, 4097, 2.5, True):
        with pytest.raises(RuntimeError, match='K='):
            box.evaluate_batch(frames, gt, evaluator=ev, K=bad)
    with pytest.raises(RuntimeError, match='no landmarks'):
        box.evaluate_batch(frames, gt, evaluator=ev, gt_quads=[np.zeros((1, 8)), np.zeros((0, 8))])
    with pytest.raises(RuntimeError, match='gt_boxes'):
        lm.evaluate_batch(frames, gt[:1], evaluator=ev)
    with pytest.raises(RuntimeError, match='more than max_gt=2'):
        lm.evaluate_batch(frames, [np.zeros((3, 4)), gt[1]], evaluator=ev)
    with pytest.raises(RuntimeError, match='gt_ignore'):
        lm.evaluate_batch(frames, gt, evaluator=ev, gt_ignore=[[0], [1]])
    with pytest.raises(RuntimeError, match='gt_quads'):
        lm.evaluate_batch(frames, gt, evaluator=ev, gt_quads=[np.zeros((2, 8)), np.zeros((0, 8))])
    with pytest.raises(RuntimeError, match='uint8'):
        lm.evaluate_batch(torch.zeros(2, 64, 64, 4, dtype=torch.uint8), gt, evaluator=ev)
    with pytest.raises(RuntimeError, match='max_batch'):
        lm.evaluate_batch(frames, gt, evaluator=ev, max_batch=0)
    assert ev._state is None                                               # no check above reached the device


def test_gt_packing_layout():
    frames = E._gt_frames('t', 2, [np.array([[1, 2, 3, 4], [5, 6, 7, 8.5]]), []], [[0, 1], []], [np.arange(16).reshape(2, 8), np.zeros((0, 8))], 3)
    buf = E._pack_gt(frames, 3, 12)
    o_cnt, o_ign, size = E._gt_layout(2, 3, 12)
    assert (o_cnt, o_ign, size) == (2 * 3 * 12 * 8, 2 * 3 * 12 * 8 + 8, 2 * 3 * 12 * 8 + 8 + 8) and buf.shape == (size,)
    gt = buf[:o_cnt].view(np.float64).reshape(2, 3, 12)
    assert gt[0, 1].tolist() == [5, 6, 7, 8.5] + list(range(8, 16)) and not gt[0, 2].any() and not gt[1].any()
    assert buf[o_cnt:o_ign].view(np.int32).tolist() == [2, 0] and buf[o_ign:o_ign + 6].tolist() == [0, 1, 0, 0, 0, 0]
