"""NumPy float64 restatement of the tracking semantics (dbx_track_update_batch, dbx_track_append, densebox_amd.track) for the tests,
written from the contract in include/densebox_hip.h as its sequential walk: predict, greedy IoU association in list order, alpha-beta
update, retirement, births.  Every float64 result is one IEEE operation per written operation, in the written order, so the kernel must
give the same bits.  tests/test_track_ref.py pins it on hand-worked sequences.  Also the seeded detection sequences the GPU tests replay.
Not collected."""
import numpy as np

TRACK = np.dtype([('box', '<f8', (4,)), ('vel', '<f8', (4,)), ('score', '<f8'), ('best_score', '<f8'), ('id', '<i4'), ('hits', '<i4'),
                  ('age', '<i4'), ('first_frame', '<i4'), ('last_frame', '<i4'), ('best_frame', '<i4')])
RECORD = np.dtype([('stream', '<i4'), ('reserved', '<i4'), ('t', TRACK)])
assert TRACK.itemsize == 104 and RECORD.itemsize == 112


def new_state(streams, max_tracks):
    """(headers int32 [streams, 4] = (frame, next_id, unborn, reserved), tracks TRACK [streams, max_tracks]): all zero, every id -1"""
    tracks = np.zeros((streams, max_tracks), TRACK)
    tracks['id'] = -1
    return np.zeros((streams, 4), np.int32), tracks


def overlaps(p, box):
    """float64 [t]: the NMS's overlap of predicted boxes p [t, 4] with one row's box -- areas (x2 - x1 + 1) * (y2 - y1 + 1), intersection
    sides max(0, min(x2) - max(x1) + 1), inter / (area_t + area_d - inter), the product rounded before the subtraction"""
    p = np.asarray(p, np.float64).reshape(-1, 4)
    box = np.asarray(box, np.float64)
    with np.errstate(all='ignore'):
        at = (p[:, 2] - p[:, 0] + 1) * (p[:, 3] - p[:, 1] + 1)
        ad = (box[2] - box[0] + 1) * (box[3] - box[1] + 1)
        xx1, yy1 = np.maximum(p[:, 0], box[0]), np.maximum(p[:, 1], box[1])
        xx2, yy2 = np.minimum(p[:, 2], box[2]), np.minimum(p[:, 3], box[3])
        w, h = np.maximum(0.0, xx2 - xx1 + 1), np.maximum(0.0, yy2 - yy1 + 1)
        inter = w * h
        return inter / (at + ad - inter)


def update_frame(header, table, dets, keep, iou_thresh=0.3, max_age=5, alpha=0.5, beta=0.1, birth_score=-np.inf):
    """One frame of one stream, in place on header int32 [4] and table TRACK [max_tracks].  The detections are rows dets[keep[i]] for
    i = 0..k-1 in that order; a keep entry outside the rows is not counted (track_id -2).  Returns (track_id, track_slot, track_hits
    int32 [k], retired TRACK [n], tally int32 [6] = (counted, matched, born, unborn, retired, live after), events) where events counts
    the slots freed in C and taken again in D in this frame under 'reuse'."""
    dets = np.asarray(dets, np.float64)
    dets = dets.reshape(-1, dets.shape[-1] if dets.ndim == 2 else 5)
    T, k, f = table.shape[0], len(keep), int(header[0])
    alpha, beta = np.float64(alpha), np.float64(beta)
    track_id, track_slot, track_hits = np.full(k, -1, np.int32), np.full(k, -1, np.int32), np.zeros(k, np.int32)
    counted = [0 <= r < dets.shape[0] for r in keep]
    live = table['id'] >= 0
    with np.errstate(all='ignore'):
        p = table['box'] + table['vel']                                     # A (only the live rows are used)
    claimed_by = np.full(T, -1, np.int64)
    slot_of = np.full(k, -1, np.int64)
    for i, r in enumerate(keep):                                            # B
        if not counted[i]:
            track_id[i] = -2
            continue
        cand = np.nonzero(live & (claimed_by < 0))[0]
        if cand.size == 0:
            continue
        o = overlaps(p[cand], dets[r, :4])
        o = np.where(np.isnan(o), -np.inf, o)
        j = int(np.argmax(o))                                               # the first of equal maxima: the lowest slot
        if o[j] > -np.inf and o[j] > iou_thresh:
            claimed_by[cand[j]] = i
            slot_of[i] = cand[j]
    retired, freed = [], set()
    for t in range(T):                                                      # C
        if not live[t]:
            continue
        tr = table[t]
        i = int(claimed_by[t])
        if i >= 0:
            row = dets[keep[i]]
            with np.errstate(all='ignore'):
                res = row[:4] - p[t]
                tr['box'] = p[t] + alpha * res
                tr['vel'] = tr['vel'] + beta * res
            tr['score'] = row[4]
            if row[4] > tr['best_score']:
                tr['best_score'], tr['best_frame'] = row[4], f
            tr['hits'] += 1
            tr['age'] = 0
            tr['last_frame'] = f
        else:
            tr['box'] = p[t]
            tr['age'] += 1
            if tr['age'] > max_age:
                retired.append(tr.copy())
                tr['id'] = -1
                freed.add(t)
    born = unborn = reuse = 0
    for i, r in enumerate(keep):                                            # D
        if not counted[i] or slot_of[i] >= 0:
            continue
        row = dets[r]
        free = np.nonzero(table['id'] < 0)[0]
        if np.isfinite(row[:4]).all() and row[4] >= birth_score and free.size:
            t = int(free[0])
            tr = table[t]
            tr['id'] = header[1]
            header[1] += 1
            tr['box'], tr['vel'] = row[:4], 0.0
            tr['score'] = tr['best_score'] = row[4]
            tr['hits'], tr['age'] = 1, 0
            tr['first_frame'] = tr['last_frame'] = tr['best_frame'] = f
            slot_of[i] = t
            born += 1
            reuse += t in freed
        else:
            unborn += 1
    header[2] += unborn
    header[0] = f + 1                                                       # E
    for i in range(k):
        if slot_of[i] >= 0:
            t = int(slot_of[i])
            track_id[i], track_slot[i], track_hits[i] = table['id'][t], t, table['hits'][t]
    matched = int((claimed_by >= 0).sum())
    tally = np.array([sum(counted), matched, born, unborn, len(retired), int((table['id'] >= 0).sum())], np.int32)
    ret = np.array(retired, TRACK) if retired else np.zeros(0, TRACK)
    return track_id, track_slot, track_hits, ret, tally, dict(match=matched, birth=born, retire=len(retired), reuse=reuse, unborn=unborn)


def update_batch(state, frames, stream0=0, **params):
    """frames: per frame of the launch (dets, keep); frame b updates stream stream0 + b of state = (headers, tracks), in place.
    Returns the per-frame results of update_frame."""
    headers, tracks = state
    assert 0 <= stream0 and stream0 + len(frames) <= headers.shape[0]
    return [update_frame(headers[stream0 + b], tracks[stream0 + b], d, k, **params) for b, (d, k) in enumerate(frames)]


def append(astate, records, capacity, results, stream0=0):
    """dbx_track_append: astate int64 [4] = (cursor, dropped, retired_total, reserved) in place; records a python list that grows up to
    `capacity` entries (stream, TRACK record), frame order then `retired` order"""
    cur = int(astate[0])
    start = cur
    for b, res in enumerate(results):
        for tr in res[3]:
            if cur < capacity:
                records.append((stream0 + b, tr.copy()))
            cur += 1
    kept = min(cur, capacity)
    astate[0] = kept
    astate[1] += cur - kept
    astate[2] += cur - start


def as_records(records):
    out = np.zeros(len(records), RECORD)
    for i, (s, tr) in enumerate(records):
        out[i]['stream'], out[i]['t'] = s, tr
    return out


# ------------------------------------------------------------------------------------------------------------ seeded sequences
BIRTH_SCORE = 0.3            # the generated objects score 0.5..1, the junk rows 0.1


def sequence(seed, steps, slots, max_age, dc=5, crowd=None):
    """`steps` frames of one camera: per frame (dets float64 [n, dc], keep list), n <= slots.  A crowd of objects drifts by a few
    pixels per frame with jitter, dropouts and newcomers.  Three things are scripted, far from the crowd, so that every branch runs
    whatever the sizes: object 0 is first in the list in frames 0 and 1 (born into slot 0, then matched) and gone afterwards, so slot 0
    retires in frame 2 + max_age; a newcomer is first in the list of exactly that frame, and is born into the slot just freed; junk rows
    (a NaN coordinate, a score below BIRTH_SCORE) that must never be born come where there is room, and alone in frame 4 + max_age.
    With slots == 1 the frames between hold no detection at all.  Without `crowd` the crowd is slots - 3 objects, all of them seen in
    frame 1, whose list then has exactly `slots` entries."""
    rs = np.random.RandomState(seed)
    fr = 2 + max_age
    assert steps > fr + 2
    n_crowd = max(0, slots - 3 if crowd is None else min(slots - 3, crowd))
    pos = rs.randint(0, 600 * 4, size=(n_crowd, 2)) / 4.0
    size = rs.randint(10 * 4, 40 * 4, size=(n_crowd, 2)) / 4.0
    vel = rs.randint(-3 * 4, 3 * 4 + 1, size=(n_crowd, 2)) / 4.0
    start = rs.randint(0, steps - 2, size=n_crowd) * (rs.rand(n_crowd) < 0.4)
    out = []
    for f in range(steps):
        boxes, scores = [], []
        if f < 2:
            boxes.append([2000.0 + 3 * f, 2000.0 + 2 * f, 2040.0 + 3 * f, 2020.0 + 2 * f])
            scores.append(0.9 - 0.1 * f)
        elif f >= fr and f != fr + 2:
            g = f - fr
            boxes.append([3000.0 - 2 * g, 100.0 + g, 3030.0 - 2 * g, 125.0 + g])
            scores.append(0.7 + 0.05 * g)
        if f != fr + 2:
            seen = (start <= f) & (rs.rand(n_crowd) > 0.15)
            if f == 1:
                seen[:] = True                                         # one frame whose list fills every position
            c = pos + vel * f + rs.randint(-4, 5, size=(n_crowd, 2)) / 4.0
            for j in np.nonzero(seen)[0]:
                boxes.append([c[j, 0], c[j, 1], c[j, 0] + size[j, 0], c[j, 1] + size[j, 1]])
                scores.append(0.5 + 0.5 * rs.rand())
        head = len(boxes) and (f < 2 or f >= fr)                      # the scripted row stays first; the crowd comes in random order
        order = list(range(len(boxes)))
        tail = order[1:] if head else order
        tail = [tail[i] for i in rs.permutation(len(tail))]
        order = (order[:1] if head else []) + tail
        junk = []
        if f == fr + 2 or (slots >= 3 and f % 2 == 1):
            junk.append(([50.0, np.nan, 90.0, 80.0], 0.95))
            junk.append(([700.0, 700.0, 730.0, 720.0], 0.1))
        rows = [(boxes[i], scores[i]) for i in order][:max(0, slots - len(junk))] + junk
        rows = rows[:slots]
        d = np.zeros((len(rows), dc), np.float64)
        for i, (b, s) in enumerate(rows):
            d[i, :4], d[i, 4] = b, s
        if dc == 13:
            d[:, 5:] = rs.randint(0, 2400, size=(len(rows), 8)) / 4.0
        # rows are stored in another order than the list walks them, as behind an NMS
        perm = rs.permutation(len(rows))
        store = np.zeros_like(d)
        store[perm] = d
        out.append((store, [int(v) for v in perm]))
    return out
