"""NumPy restatement of the best-shot gallery (dbx_crop_sharpness, dbx_track_gallery_update, densebox_amd.gallery) for the tests,
written from the contract in include/densebox_hip.h as a loop over (frame, slot) in steps 1-3.  It builds on tests/track_ref.py: the
tracks, the track_slot lists, the retired records and the tallies are that restatement's.  Every result is an integer, a copied word or
a comparison of such, so the kernel must give the same bits.  tests/test_gallery_ref.py pins it on hand-worked cases.  Not collected."""
import numpy as np

import track_ref

SHOT = np.dtype([('key', '<f8'), ('score', '<f8'), ('sharpness', '<i8'), ('id', '<i4'), ('frame', '<i4'), ('shots', '<i4'),
                 ('reserved', '<i4')])
SHOT_RECORD = np.dtype([('stream', '<i4'), ('slot', '<i4'), ('shot', SHOT)])
assert SHOT.itemsize == 40 and SHOT_RECORD.itemsize == 48
EVENTS = ('stored', 'dropped', 'lost', 'adopt', 'reborn', 'coast', 'notok', 'gated', 'first', 'replace', 'keep')


def sharpness(crops):
    """int64 [n]: the sum over the interior pixels of the squared 5-point Laplacian of the integer luma of uint8 crops [n, oh, ow, c],
    c 1 or 3: Y = 4 * v or c0 + 2 * c1 + c2; 0 when oh < 3 or ow < 3"""
    crops = np.asarray(crops)
    assert crops.dtype == np.uint8 and crops.ndim == 4 and crops.shape[3] in (1, 3)
    v = crops.astype(np.int64)
    y = 4 * v[..., 0] if crops.shape[3] == 1 else v[..., 0] + 2 * v[..., 1] + v[..., 2]
    if y.shape[1] < 3 or y.shape[2] < 3:
        return np.zeros(y.shape[0], np.int64)
    lap = 4 * y[:, 1:-1, 1:-1] - y[:, :-2, 1:-1] - y[:, 2:, 1:-1] - y[:, 1:-1, :-2] - y[:, 1:-1, 2:]
    return (lap * lap).sum(axis=(1, 2))


def fresh(track_id):
    g = np.zeros((), SHOT)
    g['key'], g['score'], g['id'], g['frame'] = -np.inf, np.nan, track_id, -1
    return g


def new_gallery(streams, max_tracks, oh, ow, c, capacity):
    """shots SHOT [streams, max_tracks] and arena SHOT_RECORD [capacity], every id -1 and everything else zero; the two crop stores
    zero; gstate int64 [4] = (ended, stored, lost, dropped)"""
    shots = np.zeros((streams, max_tracks), SHOT)
    shots['id'] = -1
    arena = np.zeros(capacity, SHOT_RECORD)
    arena['shot']['id'] = -1
    return dict(shots=shots, crops=np.zeros((streams, max_tracks, oh, ow, c), np.uint8), arena=arena,
                arena_crops=np.zeros((capacity, oh, ow, c), np.uint8), gstate=np.zeros(4, np.int64))


def update(gal, state, results, crops, ok, cursor, stream0=0, policy=0, min_score=-np.inf, commit=True):
    """dbx_track_gallery_update, in place on gal.  state = (headers, tracks) and results = what track_ref.update_batch left and returned
    for these frames; crops[b] uint8 [slots_b, oh, ow, c] and ok[b] [slots_b] by list position; cursor = word 0 of the append state
    BEFORE track_ref.append of the same results.  Returns the events of the call; with commit False nothing is written (the events are
    still counted)."""
    headers, tracks = state
    T = tracks.shape[1]
    capacity = gal['arena'].shape[0]
    ev = dict.fromkeys(EVENTS, 0)
    counts = [min(max(int(res[4][4]), 0), T) for res in results]
    for b, res in enumerate(results):
        s = stream0 + b
        slot, retired = res[1], res[3][:counts[b]]
        f = int(headers[s][0]) - 1
        for t in range(T):
            g, k = gal['shots'][s, t].copy(), tracks[s, t]
            crop = gal['crops'][s, t].copy()
            ended = g['id'] >= 0 and k['id'] != g['id']
            if ended:                                                       # 1
                hit = np.nonzero(retired['id'] == g['id'])[0]
                outcome = 'lost'
                if hit.size:
                    i = cursor + sum(counts[:b]) + int(hit[0])
                    outcome = 'stored' if cursor >= 0 and i < capacity else 'dropped'
                ev[outcome] += 1
                if commit:
                    if outcome == 'stored':
                        gal['arena'][i] = (s, t, g)
                        gal['arena_crops'][i] = crop
                    gal['gstate'][0] += 1
                    gal['gstate'][('stored', 'lost', 'dropped').index(outcome) + 1] += 1
                g['id'] = -1
            if k['id'] >= 0 and g['id'] != k['id']:                          # 2
                g, crop = fresh(k['id']), np.zeros_like(crop)
                ev['adopt'] += 1
                ev['reborn'] += bool(ended)
            if k['id'] >= 0:                                                 # 3
                js = np.nonzero(np.asarray(slot) == t)[0]
                if js.size == 0:
                    ev['coast'] += 1
                elif not ok[b][js[0]]:
                    ev['notok'] += 1
                elif not k['score'] >= min_score:
                    ev['gated'] += 1
                else:
                    j = int(js[0])
                    sh = int(sharpness(crops[b][j][None])[0])
                    key = np.float64(sh) if policy == 0 else k['score']
                    first = g['shots'] == 0
                    g['shots'] += 1
                    if first or key > g['key']:
                        g['key'], g['score'], g['sharpness'], g['frame'] = key, k['score'], sh, f
                        crop = crops[b][j].copy()
                        ev['first' if first else 'replace'] += 1
                    else:
                        ev['keep'] += 1
            if commit:
                gal['shots'][s, t], gal['crops'][s, t] = g, crop
    return ev


def live(gal):
    """per stream (shots, crops) of the slots with id >= 0, in slot order: what PlateGallery.live() returns"""
    return [(gal['shots'][s][gal['shots'][s]['id'] >= 0].copy(), gal['crops'][s][gal['shots'][s]['id'] >= 0].copy())
            for s in range(gal['shots'].shape[0])]


class Scripted:
    """A tracker restatement and a gallery restatement advanced together: step(frames, crops, ok) is one gallery.update_batch /
    net.track_plate_crops call; gallery=False advances the tracker alone (update + append), as track.update_batch does."""

    def __init__(self, streams, max_tracks, size, c, capacity, policy=0, min_score=-np.inf, track_capacity=1 << 16, **params):
        self.state = track_ref.new_state(streams, max_tracks)
        self.astate, self.records = np.zeros(4, np.int64), []
        self.gal = new_gallery(streams, max_tracks, size[1], size[0], c, capacity)
        self.policy, self.min_score, self.params, self.track_capacity = policy, min_score, params, track_capacity
        self.events = dict.fromkeys(EVENTS, 0)

    def step(self, frames, crops=None, ok=None, stream0=0, gallery=True):
        res = track_ref.update_batch(self.state, frames, stream0, **self.params)
        if gallery:
            ev = update(self.gal, self.state, res, crops, ok, int(self.astate[0]), stream0, self.policy, self.min_score)
            for name in EVENTS:
                self.events[name] += ev[name]
        track_ref.append(self.astate, self.records, self.track_capacity, res, stream0)
        return res


# ------------------------------------------------------------------------------------------------------------ seeded cases
# (max_tracks, slots, batch, max_age, stream0, streams, seed, policy): the smallest shapes that cross a wave of track slots and of list
# positions, the bounds (256 slots of tracks), launches inside a larger tracker, both policies
CASES = [
    (1, 1, 1, 1, 0, 1, 1, 0),
    (2, 65, 3, 1, 2, 6, 2, 1),
    (64, 65, 1, 0, 0, 1, 3, 0),
    (65, 1, 3, 0, 1, 4, 1, 1),
    (256, 65, 3, 2, 0, 3, 2, 0),
    (65, 10, 2, 1, 1, 4, 4, 1),
]
MIN_SCORE = 0.6              # the generated objects score 0.5..1: about a fifth of the crowd's rows are gated
STEPS = 8


def case_script(case, size=(7, 5), c=3):
    """The Scripted pair of one case -- capacity 2, or 1 with one list position; the streams outside the launch hold tracks and shots
    of their own -- and its STEPS calls: per call (frames, crops uint8 [batch, slots, oh, ow, c], ok int32 [batch, slots] with about a
    fifth of the positions not ok, whether the gallery takes part: in the even-seed cases call 3 advances the tracker alone)."""
    T, slots, batch, max_age, stream0, streams, seed, policy = case
    sc = Scripted(streams, T, size, c, 1 if slots == 1 else 2, policy, MIN_SCORE, iou_thresh=0.3, max_age=max_age, alpha=0.5, beta=0.1,
                  birth_score=track_ref.BIRTH_SCORE)
    rs = np.random.RandomState(1000 + seed)
    for s in range(streams):
        if not stream0 <= s < stream0 + batch:
            sc.state[0][s] = [7 + s, 3, 1, 55]
            t = sc.state[1][s, 0]
            t['id'], t['box'], t['vel'], t['hits'], t['score'] = 2, [2000.0, 2000.0, 2040.0, 2020.0], [1.0, 0.5, 1.0, 0.5], 4, 0.75
            sc.gal['shots'][s, 0] = (123.0, 0.75, 123, 2, 5 + s, 3, 0)
            sc.gal['crops'][s, 0] = rs.randint(0, 256, size=sc.gal['crops'].shape[2:])
    seqs = [track_ref.sequence(seed + 10 * b, STEPS, slots, max_age, 13) for b in range(batch)]
    calls = []
    for step in range(STEPS):
        crops = rs.randint(0, 256, size=(batch, slots, size[1], size[0], c)).astype(np.uint8)
        ok = (rs.rand(batch, slots) >= 0.2).astype(np.int32)
        calls.append(([seqs[b][step] for b in range(batch)], crops, ok, not (seed % 2 == 0 and step == 3)))
    return sc, calls
