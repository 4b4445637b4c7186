"""Evaluation against labelled data on the GPU: the kept detections of any detect_* call matched to ground-truth boxes
(dbx_match_gt_batch) and the (score, TP / FP) records of a whole labelled set accumulated in a device arena (dbx_eval_append), so that
precision, recall and average precision at EVERY score threshold come from one pass at a low one.

Semantics, per frame (the PASCAL VOC devkit's matching with the +1-pixel IoU of the reference's NMS, DenseBox.py:3398-3443; the
reference itself has no evaluator).  The detections are the kept rows in keep-list order, i = 0..k-1.  For detection i, jmax is the GT
box of the largest IoU (the lowest index on ties, a NaN IoU never wins) and the detection is matched when that IoU is > iou_thresh,
strictly.  status 0 (false positive), gt_index -1: not matched.  status -1 (ignored, neither TP nor FP): matched to a GT that carries the
ignore flag.  status 1 (true positive): the first detection in list order matched to jmax; a later one is a duplicate, status 0 with
gt_index jmax.  lm_err (13-column rows with GT quads): for a TP the mean distance of the four landmarks (columns 5..12) to the GT quad's
corners over sqrt((x2 - x1 + 1) * (y2 - y1 + 1)) of the GT box, NaN otherwise."""
import ctypes as C
import itertools

import numpy as np
import torch

from . import _lib, decode as DC, rows as R
from ._lib import check, ptr, stream_ptr
from .decode import _host, _integer

MAX_SLOTS = 4096             # dbx_match_gt_batch's bound on the list positions of a frame
MAX_GT = 1024                # ... and on the GT boxes of a frame (they live in LDS)
RECORD = np.dtype([('score', '<f8'), ('lm_err', '<f8'), ('status', '<i4'), ('frame', '<i4')])       # dbx_eval_record
assert RECORD.itemsize == C.sizeof(_lib.EvalRecord) == 24


# ------------------------------------------------------------------------------------------------------------ host: the curves
def _curve(scores, status, n_gt):
    """(scores, precision, recall) along the ranking: ignored records dropped, stable descending sort (ties keep arrival order)"""
    scores, status = np.asarray(scores, np.float64).reshape(-1), np.asarray(status).reshape(-1)
    if scores.shape != status.shape:
        raise RuntimeError('evaluate: %d scores for %d status values' % (scores.size, status.size))
    m = status != -1
    scores, status = scores[m], status[m]
    order = np.argsort(-scores, kind='stable')
    tp, fp = np.cumsum(status[order] == 1), np.cumsum(status[order] != 1)
    rec = tp / n_gt if n_gt > 0 else np.full(tp.shape, np.nan)
    return scores[order], tp / np.maximum(tp + fp, 1), rec


def average_precision(scores, status, n_gt):
    """VOC all-point average precision of records (score, status 1 TP / 0 FP / -1 ignored) against n_gt GT boxes: the envelope of the
    precision (made monotone from the right) summed over the steps of the recall.  NaN when n_gt == 0."""
    if n_gt <= 0:
        return float('nan')
    _, prec, rec = _curve(scores, status, n_gt)
    mrec, mpre = np.concatenate(([0.0], rec, [1.0])), np.concatenate(([0.0], prec, [0.0]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    i = np.nonzero(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))


def precision_recall_at(scores, status, n_gt, score_thresh):
    """(precision, recall) of the records whose score is > score_thresh (strictly, as the threshold decode compares); ignored records
    dropped.  precision is NaN without such a record, recall NaN when n_gt == 0."""
    scores, status = np.asarray(scores, np.float64).reshape(-1), np.asarray(status).reshape(-1)
    m = (status != -1) & (scores > score_thresh)
    n, tp = int(m.sum()), int((status[m] == 1).sum())
    return (tp / n if n else float('nan')), (tp / n_gt if n_gt > 0 else float('nan'))


# ------------------------------------------------------------------------------------------------------------ host: ground truth
def _gt_frames(fn, n, gt_boxes, gt_ignore, gt_quads, max_gt):
    """per image (boxes float64 [g, 4], ignore uint8 [g], quads float64 [g, 8] or None), or RuntimeError"""
    for name, v in (('gt_boxes', gt_boxes), ('gt_ignore', gt_ignore), ('gt_quads', gt_quads)):
        if v is None and name != 'gt_boxes':
            continue
        if not isinstance(v, (list, tuple)) or len(v) != n:
            raise RuntimeError('%s: %s must be a list with one entry per image (%d), got %s' %
                               (fn, name, n, len(v) if isinstance(v, (list, tuple)) else type(v).__name__))
    out = []
    for i in range(n):
        b = _host(gt_boxes[i]).astype(np.float64)
        if b.size == 0:
            b = b.reshape(0, 4)
        if b.ndim != 2 or b.shape[1] != 4:
            raise RuntimeError('%s: gt_boxes[%d] must be [g, 4] (x1, y1, x2, y2), got %s' % (fn, i, list(b.shape)))
        g = b.shape[0]
        if g > max_gt:
            raise RuntimeError('%s: gt_boxes[%d] holds %d boxes, more than max_gt=%d' % (fn, i, g, max_gt))
        ig = np.zeros(g, np.uint8)
        if gt_ignore is not None:
            ig = (_host(gt_ignore[i]).reshape(-1) != 0).astype(np.uint8)
            if ig.shape[0] != g:
                raise RuntimeError('%s: gt_ignore[%d] holds %d flags for %d boxes' % (fn, i, ig.shape[0], g))
        q = None
        if gt_quads is not None:
            q = _host(gt_quads[i]).astype(np.float64)
            if q.size != g * 8:
                raise RuntimeError('%s: gt_quads[%d] must hold 8 numbers per box (%d boxes), got %s' % (fn, i, g, list(q.shape)))
            q = q.reshape(g, 8)
        out.append((b, ig, q))
    return out


def _gt_layout(B, max_gt, gt_cols):
    """byte offsets of (gt float64 [B][max_gt][gt_cols], counts int32 [B], ignore uint8 [B][max_gt]) in one buffer, and its size"""
    o_cnt = B * max_gt * gt_cols * 8
    o_ign = o_cnt + B * 4
    return o_cnt, o_ign, (o_ign + B * max_gt + 7) // 8 * 8


def _pack_gt(frames, max_gt, gt_cols):
    """the uint8 host image of one chunk's ground truth in _gt_layout"""
    B = len(frames)
    o_cnt, o_ign, size = _gt_layout(B, max_gt, gt_cols)
    buf = np.zeros(size, np.uint8)
    gt = buf[:o_cnt].view(np.float64).reshape(B, max_gt, gt_cols)
    cnt = buf[o_cnt:o_ign].view(np.int32)
    ign = buf[o_ign:o_ign + B * max_gt].reshape(B, max_gt)
    for i, (b, ig, q) in enumerate(frames):
        g = b.shape[0]
        cnt[i] = g
        gt[i, :g, :4] = b
        ign[i, :g] = ig
        if gt_cols == 12:
            gt[i, :g, 4:] = q
    return buf


# ------------------------------------------------------------------------------------------------------------ the launches
def _launch_match(rows, gtbuf, gt_cols, max_gt, iou_thresh):
    """dbx_match_gt_batch on the device rows `rows` (rows.Rows), the ground truth in a device buffer of _gt_layout: (status, gt_index
    int32 [B, slots], iou, lm_err (or None) float64 [B, slots], tally int32 [B, 5]) device tensors"""
    dev, B, slots = rows.dets.device, rows.B, rows.slots
    o_cnt, o_ign, _ = _gt_layout(B, max_gt, gt_cols)
    status = torch.empty((B, slots), dtype=torch.int32, device=dev)
    index = torch.empty((B, slots), dtype=torch.int32, device=dev)
    iou = torch.empty((B, slots), dtype=torch.float64, device=dev)
    err = torch.empty((B, slots), dtype=torch.float64, device=dev) if (rows.dc == 13 and gt_cols == 12) else None
    tally = torch.empty((B, 5), dtype=torch.int32, device=dev)
    g = gtbuf.data_ptr()
    check(_lib.lib().dbx_match_gt_batch(*rows.args(), C.c_void_p(g), gt_cols, C.c_void_p(g + o_cnt), C.c_void_p(g + o_ign), max_gt,
                                        float(iou_thresh), ptr(status), ptr(index), ptr(iou), ptr(err), ptr(tally), stream_ptr()))
    return status, index, iou, err, tally


def match_batch(dets, keeps, gt_boxes, gt_ignore=None, gt_quads=None, iou_thresh=0.5):
    """The results of any detect_* call matched to ground truth with ONE upload, ONE dbx_match_gt_batch launch and one copy back.

    dets, keeps: per image the float64 rows [n, 5|13] (numpy arrays or tensors, host or device) and the keep list, as detect_batch,
    detect_batch_thresh, detect_batch_resized and detect_pyramid return them; an image may have no rows and an empty list.
    gt_boxes: per image [g, 4] boxes (x1, y1, x2, y2) in the rows' coordinates, g may be 0 (at most 1024).  gt_ignore: per image [g]
    flags, or None.  gt_quads: per image [g, 8] landmark corners in the order of row columns 5..12, or None; they need 13-column rows.

    Returns, per image, (status int32 [k], gt_index int32 [k], iou float64 [k], lm_err float64 [k] or None) for the k entries of its keep
    list in order (the module docstring has the semantics)."""
    fn = 'match_batch'
    p = R.pack_host(fn, dets, keeps, max_slots=MAX_SLOTS)
    if isinstance(iou_thresh, bool) or not isinstance(iou_thresh, (int, float, np.integer, np.floating)) or np.isnan(iou_thresh):
        raise RuntimeError('%s: iou_thresh=%r must be a number' % (fn, iou_thresh))
    B, slots, lists = p.B, p.slots, p.lists
    frames = _gt_frames(fn, B, gt_boxes, gt_ignore, gt_quads, MAX_GT)
    if gt_quads is not None and p.dc != 13:
        raise RuntimeError('%s: gt_quads need 13-column rows (DenseBoxLM / DenseBoxLMLOC), got %d columns' % (fn, p.dc))
    max_gt = max(1, max(f[0].shape[0] for f in frames))
    gt_cols = 12 if gt_quads is not None else 4
    gt = _pack_gt(frames, max_gt, gt_cols)
    o_gt = p.nd + (p.nk + 7) // 8 * 8                                                  # the ground truth behind the lists, 8-byte padded
    host = np.zeros(o_gt + gt.size, np.uint8)
    p.write(host, 0, p.nd)
    host[o_gt:] = gt
    buf = torch.from_numpy(host).cuda()                                               # the one upload
    status, index, iou, err, _ = _launch_match(p.on(buf, 0, p.nd), buf[o_gt:], gt_cols, max_gt, iou_thresh)
    parts = [status.view(torch.uint8).reshape(-1), index.view(torch.uint8).reshape(-1), iou.view(torch.uint8).reshape(-1)]
    if err is not None:
        parts.append(err.view(torch.uint8).reshape(-1))
    h = torch.cat(parts).cpu().numpy()                                                 # the one copy back
    n4, n8 = B * slots * 4, B * slots * 8
    status, index = (h[i * n4:(i + 1) * n4].view(np.int32).reshape(B, slots) for i in range(2))
    iou = h[2 * n4:2 * n4 + n8].view(np.float64).reshape(B, slots)
    err = h[2 * n4 + n8:].view(np.float64).reshape(B, slots) if err is not None else None
    return [(status[i, :k.size].copy(), index[i, :k.size].copy(), iou[i, :k.size].copy(), None if err is None else err[i, :k.size].copy())
            for i, k in enumerate(lists)]


# ------------------------------------------------------------------------------------------------------------ the evaluator
class Evaluator:
    """The device side of an evaluation pass: an arena of `capacity` dbx_eval_record (24 bytes each) and the running totals, filled by
    net.evaluate_batch() without a copy to the host per batch, read once by summary().  iou_thresh: a detection is matched when its
    best IoU is strictly above it.  max_gt: the most GT boxes one frame may carry (1..1024).  The buffers are allocated on `device`
    (the current CUDA device by default) at the first use."""
    _serials = itertools.count()

    def __init__(self, capacity=1 << 20, iou_thresh=0.5, max_gt=64, device=None):
        if not _integer(capacity) or capacity < 1:
            raise RuntimeError('Evaluator: capacity=%r must be a positive integer' % (capacity,))
        if not _integer(max_gt) or not 1 <= max_gt <= MAX_GT:
            raise RuntimeError('Evaluator: max_gt=%r must be an integer in 1..%d' % (max_gt, MAX_GT))
        if isinstance(iou_thresh, bool) or not isinstance(iou_thresh, (int, float, np.integer, np.floating)) or np.isnan(iou_thresh):
            raise RuntimeError('Evaluator: iou_thresh=%r must be a number' % (iou_thresh,))
        self.capacity, self.iou_thresh, self.max_gt = int(capacity), float(iou_thresh), int(max_gt)
        self.device = None if device is None else torch.device(device)
        self.serial = next(Evaluator._serials)      # part of the graph keys: a new evaluator never replays another one's graphs
        self._records = self._state = self._dry = None
        self._gt = {}

    def _buffers(self, dev):
        """(records uint8 [capacity * 24], state int64 [8]) on the device, allocated once"""
        if self._state is None:
            dev = self.device if self.device is not None else dev
            self._records = torch.empty(self.capacity * RECORD.itemsize, dtype=torch.uint8, device=dev)
            self._state = torch.zeros(8, dtype=torch.int64, device=dev)
            self._dry = torch.zeros(8, dtype=torch.int64, device=dev)     # the state a graph's warm-up runs count into
        return self._records, self._state

    def _gt_static(self, B, gt_cols):
        """the static device buffer (_gt_layout) the launches of chunks of B frames read their ground truth from"""
        buf = self._gt.get((B, gt_cols))
        if buf is None:
            buf = self._gt[(B, gt_cols)] = torch.zeros(_gt_layout(B, self.max_gt, gt_cols)[2], dtype=torch.uint8, device=self._state.device)
        return buf

    def reset(self):
        """forget every record and total; the buffers (and the graphs captured on them) stay"""
        if self._state is not None:
            self._state.zero_()

    def summary(self):
        """One copy of the state, then one copy of exactly the records written.  Returns a dict: ap (VOC all-point), scores / precision /
        recall (arrays along the ranking, ignored records dropped), tp, fp, ignored, n_gt, frames, lm_nme (the mean lm_err over the true
        positives that have one, or None), records (the structured array, in frame order then list order).  Raises when records were
        dropped because the arena was full."""
        st = np.zeros(8, np.int64) if self._state is None else self._state.cpu().numpy()
        cursor, dropped, frames, n_gt, tp, fp, ign = (int(v) for v in st[:7])
        if dropped > 0:
            raise RuntimeError('Evaluator: %d records did not fit the arena of capacity=%d; evaluate with a larger capacity'
                               % (dropped, self.capacity))
        rec = np.zeros(0, RECORD) if cursor == 0 else self._records[:cursor * RECORD.itemsize].cpu().numpy().view(RECORD)
        scores, prec, recall = _curve(rec['score'], rec['status'], n_gt)
        e = rec['lm_err'][(rec['status'] == 1) & ~np.isnan(rec['lm_err'])]
        return dict(ap=average_precision(rec['score'], rec['status'], n_gt), scores=scores, precision=prec, recall=recall, tp=tp, fp=fp,
                    ignored=ign, n_gt=n_gt, frames=frames, lm_nme=float(e.mean()) if e.size else None, records=rec)


# ------------------------------------------------------------------------------------------------------------ net.evaluate_batch
def _eval_eager(ev, gtbuf, gt_cols, K, thresh, nms_thresh, dry_outside_capture):
    """The eager function of evaluate_batch's chunks: forward, decode (+ NMS), dbx_match_gt_batch, dbx_eval_append.  thresh: None for
    the top-K decode of K rows, or (score_thresh, max_dets).  Under _graph_replay the function also runs twice as a warm-up before the
    capture: with dry_outside_capture those runs append into a scratch state with capacity 0, so only replays count.  Returns (tally,
    every tensor the launches read or wrote): a graph entry keeps both, which pins the buffers its replays use."""
    def eager(net, images):
        s, l, hm, ll = DC._forward_maps(net, images)
        B = int(images.size(0))
        rows, _ = R.decode_rows(s, l, hm, ll, B, K, thresh, nms_thresh)
        status, index, iou, err, tally = _launch_match(rows, gtbuf, gt_cols, ev.max_gt, ev.iou_thresh)
        records, state = ev._buffers(images.device)
        dry = dry_outside_capture and not torch.cuda.is_current_stream_capturing()
        check(_lib.lib().dbx_eval_append(*rows.args(), ptr(status), ptr(err), ptr(tally), None if dry else ptr(records),
                                         0 if dry else ev.capacity, ptr(ev._dry if dry else state), stream_ptr()))
        return tally, (rows.dets, rows.keep, rows.prefix, status, index, iou, err, records, state, gtbuf)
    return eager


def evaluate_batch(net, images, gt_boxes, *, evaluator, K=10, score_thresh=None, max_dets=1024, nms_thresh=0.4, max_batch=32,
                   gt_ignore=None, gt_quads=None):
    """Detection and its scoring against ground truth in one go, with nothing returned to the host: per chunk of at most `max_batch`
    same-shape frames the forward, dbx_detect_batch (top-K) or dbx_detect_thresh_batch (score_thresh given: every pixel above it, at
    most max_dets per frame; a non-default K together with it raises), dbx_match_gt_batch on the rows and keep lists where the decode
    left them, and dbx_eval_append into `evaluator`.  evaluator.summary() reads the totals and the curve afterwards.

    images, max_batch, chunking and list grouping: detect_batch's (frames of other sizes go through detect_batch_resized /
    detect_pyramid and match_batch).  gt_boxes: per image [g, 4] boxes in input pixels, g <= evaluator.max_gt; gt_ignore, gt_quads: per
    image [g] flags / [g, 8] corners or None; quads need a landmark net.  Frames are numbered in the order the chunks run (input order
    for a batch tensor; a list of mixed shapes runs shape by shape).

    Eval mode replays ONE hipGraph per chunk from the cache detect() uses, under a tag of its own, keyed by (batch shape, dtype, (decode
    mode and its sizes, the evaluator and its buffers, iou_thresh, max_gt, GT columns), nms_thresh, compute dtype); the chunk's ground
    truth is uploaded into a static device buffer of the evaluator that the captured launches read.  Train mode and DBX_GRAPH=0 run the
    same launches eagerly."""
    fn = 'evaluate_batch'
    if not isinstance(evaluator, Evaluator):
        raise RuntimeError('%s: evaluator must be an evaluate.Evaluator, got %s' % (fn, type(evaluator).__name__))
    tc = DC._thresh_or_topk(fn, K, score_thresh, max_dets)
    if tc is None:
        R._check_K(fn, K, MAX_SLOTS)
    if gt_quads is not None:
        DC._require_landmarks(fn, net, 'compare gt_quads with')
    frames = _gt_frames(fn, DC._frame_count(fn, images), gt_boxes, gt_ignore, gt_quads, evaluator.max_gt)
    gt_cols = 12 if gt_quads is not None else 4
    mode = ('topk', int(K)) if tc is None else ('thresh', tc[1], tc[0])
    dry = DC._use_graph(net)

    def chunk(x, idx):
        records, state = evaluator._buffers(x.device)
        gtbuf = evaluator._gt_static(len(idx), gt_cols)
        gtbuf.copy_(torch.from_numpy(_pack_gt([frames[i] for i in idx], evaluator.max_gt, gt_cols)))      # the chunk's one upload
        key = (mode + (evaluator.serial, records.data_ptr(), state.data_ptr(), gtbuf.data_ptr(), evaluator.iou_thresh, evaluator.max_gt,
                       gt_cols), float(nms_thresh))
        DC._run_chunk(net, 'evaluate', x, key, _eval_eager(evaluator, gtbuf, gt_cols, int(K), tc, nms_thresh, dry), (False, False))
        return [None] * len(idx)
    DC._detect_many(fn, images, max_batch, chunk, with_index=True)
