"""NumPy restatement of the evaluation semantics (dbx_match_gt_batch, dbx_eval_append, densebox_amd.evaluate) for the tests: the PASCAL
VOC devkit's matching written as its sequential loop over the detections in list order, with the +1-pixel IoU of the reference's NMS
(DenseBox.py:3398-3443), the landmark error of a true positive, and VOC all-point average precision.  The reference has no evaluator, so
these definitions are the project's own; tests/test_eval_ref.py pins them on hand-worked cases.  Not collected."""
import numpy as np


def iou_row(box, gt):
    """float64 [g]: the NMS's overlap of one box with every GT box -- areas (x2 - x1 + 1) * (y2 - y1 + 1), intersection sides
    max(0, min(x2) - max(x1) + 1), inter / (area_d + area_g - inter).  A NaN coordinate gives a NaN overlap (the areas carry it)."""
    box = np.asarray(box, np.float64)
    gt = np.asarray(gt, np.float64).reshape(-1, 4)
    with np.errstate(all='ignore'):
        ad = (box[2] - box[0] + 1) * (box[3] - box[1] + 1)
        ag = (gt[:, 2] - gt[:, 0] + 1) * (gt[:, 3] - gt[:, 1] + 1)
        xx1, yy1 = np.maximum(box[0], gt[:, 0]), np.maximum(box[1], gt[:, 1])
        xx2, yy2 = np.minimum(box[2], gt[:, 2]), np.minimum(box[3], gt[:, 3])
        w, h = np.maximum(0.0, xx2 - xx1 + 1), np.maximum(0.0, yy2 - yy1 + 1)
        inter = w * h
        return inter / (ad + ag - inter)


def best_gt(ovr):
    """(jmax, ovmax): the largest overlap, the lowest index on ties, a NaN never wins; (-1, -inf) without a winner"""
    v = np.where(np.isnan(ovr), -np.inf, np.asarray(ovr, np.float64))
    if v.size == 0:
        return -1, -np.inf
    j = int(np.argmax(v))                                  # the first of equal maxima
    return (j, float(v[j])) if v[j] > -np.inf else (-1, -np.inf)


def lm_error(row, gt_box, gt_quad):
    """mean corner distance between the row's landmarks (columns 5..12) and the GT quad, over sqrt of the GT box's +1 area"""
    d = (np.asarray(row, np.float64)[5:13] - np.asarray(gt_quad, np.float64)).reshape(4, 2)
    s = 0.0
    for c in range(4):
        s += np.sqrt(d[c, 0] * d[c, 0] + d[c, 1] * d[c, 1])
    with np.errstate(all='ignore'):
        return s / 4.0 / np.sqrt((gt_box[2] - gt_box[0] + 1) * (gt_box[3] - gt_box[1] + 1))


def match_frame(dets, keep, gt_boxes, gt_ignore=None, gt_quads=None, iou_thresh=0.5):
    """One frame, the devkit's walk: the detections are rows dets[keep[i]] for i = 0..k-1 in that order.  A keep entry outside the rows
    gives its position status -2 (gt_index -1, iou NaN) and is not counted.  Returns (status int32 [k], gt_index int32 [k], iou float64
    [k], lm_err float64 [k] or None, tally int32 [5] = (counted, TP, FP, ignored, GT without the ignore flag))."""
    dets = np.asarray(dets, np.float64)
    dets = dets.reshape(-1, dets.shape[-1] if dets.ndim == 2 else 5)
    gt = np.asarray(gt_boxes, np.float64).reshape(-1, 4)
    g = gt.shape[0]
    ign = np.zeros(g, bool) if gt_ignore is None else np.asarray(gt_ignore).reshape(-1).astype(bool)
    quads = None if gt_quads is None else np.asarray(gt_quads, np.float64).reshape(g, 8)
    k = len(keep)
    status, index = np.zeros(k, np.int32), np.full(k, -1, np.int32)
    iou = np.full(k, np.nan, np.float64)
    err = None if quads is None else np.full(k, np.nan, np.float64)
    taken = np.zeros(g, bool)
    for i, r in enumerate(keep):
        if not 0 <= r < dets.shape[0]:
            status[i] = -2
            continue
        jmax, ovmax = best_gt(iou_row(dets[r, :4], gt))
        iou[i] = ovmax
        if not ovmax > iou_thresh:
            continue                                   # FP, gt_index -1
        index[i] = jmax
        if ign[jmax]:
            status[i] = -1
        elif not taken[jmax]:
            taken[jmax] = True
            status[i] = 1
            if err is not None:
                err[i] = lm_error(dets[r], gt[jmax], quads[jmax])
        # else: the GT is taken, a duplicate FP with its gt_index
    tally = np.array([(status != -2).sum(), (status == 1).sum(), (status == 0).sum(), (status == -1).sum(), (~ign).sum()], np.int32)
    return status, index, iou, err, tally


def records(results):
    """the records dbx_eval_append leaves for a sequence of frames: per frame (dets, keep, status, lm_err or None) -> structured array
    (score, lm_err, status, frame) of the counted positions, in frame order then list order"""
    out = []
    for f, (dets, keep, status, err) in enumerate(results):
        for i, r in enumerate(keep):
            if status[i] != -2:
                out.append((dets[r, 4], np.nan if err is None else err[i], status[i], f))
    return np.array(out, dtype=[('score', '<f8'), ('lm_err', '<f8'), ('status', '<i4'), ('frame', '<i4')])


def average_precision(scores, status, n_gt):
    """VOC all-point AP: ignored records (status -1) dropped, a stable descending sort by score (ties in arrival order), precision made
    monotone from the right, summed over the recall steps.  NaN when there is no GT."""
    scores, status = np.asarray(scores, np.float64), np.asarray(status)
    if n_gt <= 0:
        return float('nan')
    m = status != -1
    scores, status = scores[m], status[m]
    order = sorted(range(len(scores)), key=lambda i: -scores[i])          # sorted() is stable
    tp = fp = 0
    rec, prec = [0.0], [0.0]
    for i in order:
        tp += int(status[i] == 1)
        fp += int(status[i] != 1)
        rec.append(tp / n_gt)
        prec.append(tp / (tp + fp))
    rec.append(1.0)
    prec.append(0.0)
    for i in range(len(prec) - 2, -1, -1):
        prec[i] = max(prec[i], prec[i + 1])
    return float(sum((rec[i + 1] - rec[i]) * prec[i + 1] for i in range(len(rec) - 1) if rec[i + 1] != rec[i]))


NAN = float('nan')


def _rows(boxes, scores=None, dc=5):
    """rows [n, dc] from boxes, scores descending from 0.9 by default, landmarks (dc 13) the box corners shifted by (0.5, 0.25)"""
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    d = np.zeros((b.shape[0], dc), np.float64)
    d[:, :4] = b
    d[:, 4] = 0.9 - 0.05 * np.arange(b.shape[0]) if scores is None else scores
    if dc == 13:
        d[:, 5:13] = quad_of(b) + np.tile([0.5, 0.25], 4)
    return d


def quad_of(boxes):
    """the corners (left-up, right-up, right-down, left-down) of boxes [g, 4] as quads [g, 8]"""
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    return np.stack([b[:, 0], b[:, 1], b[:, 2], b[:, 1], b[:, 2], b[:, 3], b[:, 0], b[:, 3]], axis=1)


# Hand-worked frames: (name, boxes of the rows, keep list, GT boxes, ignore flags or None, iou_thresh, expected status, gt_index, iou).
# [0,0,9,9] has area 100; [0,0,9,4] and [0,5,9,9] have area 50 and lie inside it: IoU exactly 0.5 each.  [1,0,10,9] against [0,0,9,9]:
# inter 90, union 110, IoU 9/11.
HAND_CASES = [
    ('two detections on one GT: TP then duplicate FP', [[0, 0, 9, 9], [1, 0, 10, 9], [50, 50, 59, 59]], [0, 1, 2], [[0, 0, 9, 9]], None, 0.5,
     [1, 0, 0], [0, 0, -1], [1.0, 9.0 / 11.0, 0.0]),
    ('list order decides, not row order', [[1, 0, 10, 9], [0, 0, 9, 9]], [1, 0], [[0, 0, 9, 9]], None, 0.5, [1, 0], [0, 0], [1.0, 9.0 / 11.0]),
    ('IoU equal to the threshold is a FP', [[0, 0, 9, 9]], [0], [[0, 0, 9, 4]], None, 0.5, [0], [-1], [0.5]),
    ('a tie between two GTs: the lowest index', [[0, 0, 9, 9]], [0], [[0, 5, 9, 9], [0, 0, 9, 4]], None, 0.4, [1], [0], [0.5]),
    ('an ignore GT: neither TP nor FP, never taken', [[0, 0, 9, 9], [1, 0, 10, 9]], [0, 1], [[0, 0, 9, 9]], [1], 0.5, [-1, -1], [0, 0],
     [1.0, 9.0 / 11.0]),
    ('no GT', [[0, 0, 9, 9]], [0], [], None, 0.5, [0], [-1], [-np.inf]),
    ('no detections', [[0, 0, 9, 9]], [], [[0, 0, 9, 9], [20, 20, 29, 29]], [0, 1], 0.5, [], [], []),
    ('NaN coordinates never match', [[0, NAN, 9, 9], [0, 0, 9, 9]], [0, 1], [[NAN, 0, 9, 9], [0, 0, 9, 9]], None, 0.5, [0, 1], [-1, 1],
     [-np.inf, 1.0]),
]
