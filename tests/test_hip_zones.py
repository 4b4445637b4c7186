"""Zones on the GPU, bit for bit against the restatement (tests/zones_ref.py): dbx_zone_filter_keep in both layouts with clamped counts,
bad keep entries and corrupted prefixes; the filter, dbx_zone_update_batch and dbx_zone_append after every step of the seeded sequences (state,
counters, staging, arena, cursor, dropped), the neighbouring streams untouched, commit = 0 writing nothing; Zones.set_stream between
two replays; net.watch_batch == detect_batch / detect_batch_thresh + the restated filter + tests/track_ref.py + the restated update;
zones.update_batch and zones.filter_keep on host results."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import densebox_amd as D
from densebox_amd import _lib, synth, track as T, zones as ZN
from densebox_amd._lib import check, ptr, stream_ptr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_ref as TR  # noqa: E402
import zones_ref as Z  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64                     # sentinel elements in front of and behind every output (a multiple of 16 bytes for every dtype used)
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


def _table_bytes(cfg):
    """the dbx_zone_config of a restatement Config, as uint8 [2320]"""
    c = np.zeros((), ZN.CONFIG)
    c['n_lines'], c['n_regions'], c['n_masks'] = len(cfg.lines), len(cfg.regions), len(cfg.masks)
    for i, l in enumerate(cfg.lines):
        c['lines'][i] = l
    for name, polys in (('regions', [(0, p) for p in cfg.regions]), ('masks', cfg.masks)):
        for i, (role, p) in enumerate(polys):
            c[name][i]['n'], c[name][i]['role'] = len(p), role
            c[name][i]['xy'][:2 * len(p)] = np.asarray(p, np.int32).reshape(-1)
    buf = _bits(c).copy()
    check(_lib.lib().dbx_zone_check_config(C.cast(buf.ctypes.data, C.POINTER(_lib.ZoneConfig))))
    return buf


def _tables(cfgs):
    return torch.from_numpy(np.concatenate([_table_bytes(c) for c in cfgs])).cuda()


# ------------------------------------------------------------------------------------------------------------ the filter
def _frame(keep, prefix, b, slots, det_rows):
    """det_frame's reading rule on host arrays: (first row, rows, the list's word offset in keep, clamped count, prefix pair good)"""
    if prefix is not None:
        p0, p1 = int(prefix[b]), int(prefix[b + 1])
        ok = p0 >= 0 and p1 >= p0 and p1 <= det_rows
        r0, n, at = (p0, p1 - p0, p0 + b) if ok else (0, 0, 0)
    else:
        ok, r0, n, at = True, b * slots, slots, b * (slots + 1)
    lim = min(n, slots)
    c = int(keep[at]) if lim > 0 else 0
    return r0, n, at, max(0, min(c, lim)), ok


def _filter_case(cfgs, dets, keep, prefix, B, slots, stream0, kind, det_rows=None):
    """dbx_zone_filter_keep called directly; checks every word of keep_out and stats against the restatement and the guards"""
    dc = dets.shape[-1]
    det_rows = dets.size // dc if det_rows is None else det_rows
    d_dets, d_keep = torch.from_numpy(dets).cuda(), torch.from_numpy(keep).cuda()
    d_prefix = None if prefix is None else torch.from_numpy(np.asarray(prefix, np.int32)).cuda()
    out, p_out = _guarded(keep.size, torch.int32, FILL_I)
    st, p_st = _guarded(2 * B, torch.int32, FILL_I)
    check(_lib.lib().dbx_zone_filter_keep(ptr(d_dets), dc, det_rows, ptr(d_keep), ptr(d_prefix), B, slots, ptr(_tables(cfgs)), len(cfgs),
                                          stream0, ZN.ANCHORS[kind], p_out, p_st, stream_ptr()))
    torch.cuda.synchronize()
    got, stats = _inner(out, keep.size, FILL_I, 'keep_out'), _inner(st, 2 * B, FILL_I, 'stats').reshape(B, 2)
    want = np.full(keep.size, FILL_I, np.int32)
    rows = dets.reshape(-1, dc)
    tot = [0, 0]
    for b in range(B):
        r0, n, at, k, ok = _frame(keep, prefix, b, slots, det_rows)
        kept = Z.filter_keep(cfgs[stream0 + b], rows[r0:r0 + n], [int(v) for v in keep[at + 1:at + 1 + k]], kind)
        assert stats[b].tolist() == [k, len(kept)], (b, stats[b], k, len(kept))
        if ok:
            want[at], want[at + 1:at + 1 + len(kept)], want[at + 1 + len(kept):at + 1 + min(n, slots)] = len(kept), kept, 0
        tot[0] += len(kept)
        tot[1] += k - len(kept)
    assert np.array_equal(got, want), (got, want)
    return tot


def _mask_cfgs(streams):
    """stream 0 and every third one has no mask polygon; the others an include polygon with a concave notch and an exclude square"""
    inc = [(40, 40), (600, 40), (600, 440), (320, 300), (40, 440)]
    masked = Z.from_pixels(include=[inc], exclude=[[(200, 100), (260, 100), (260, 160), (200, 160)]])
    return [Z.Config() if s % 3 == 0 else masked for s in range(streams)]


def _rows(rs, n, dc):
    d = np.zeros((n, dc))
    c = np.stack([rs.randint(0, 640 * 4, size=n), rs.randint(0, 480 * 4, size=n)], 1) / 4.0
    d[:, 0], d[:, 1], d[:, 2], d[:, 3], d[:, 4] = c[:, 0] - 15, c[:, 1] - 10, c[:, 0] + 15, c[:, 1] + 10, rs.rand(n)
    d[rs.rand(n) < 0.05, rs.randint(0, 4)] = np.nan
    return d


@pytest.mark.parametrize('slots,dc,kind', [(1, 5, 'centre'), (7, 13, 'bottom'), (1024, 5, 'centre')])
def test_filter_in_the_slot_layout(slots, dc, kind):
    rs = np.random.RandomState(slots)
    B, streams, stream0 = 4, 6, 1                                       # streams 1, 2, 4 are masked, 3 is copied
    dets = _rows(rs, B * slots, dc)
    keep = np.zeros((B, slots + 1), np.int32)
    for b in range(B):
        keep[b, 1:] = rs.permutation(slots)
        keep[b, 0] = slots
    if slots > 1:
        keep[0, 0] = slots + 100                                        # a count beyond the slots is clamped
        keep[1, 0] = slots // 2
        keep[1, 1 + slots // 2:] = 5                                    # entries behind the count are not read; the output has zeros there
        keep[2, 1:4] = [-1, slots, 1 << 30]                             # entries outside the rows: copied on the stream without a mask
        keep[3, 2:4] = [-7, slots + 3]                                  # ... and dropped on a masked one
    else:
        keep[1, 0] = -3                                                 # a negative count is 0
    tot = _filter_case(_mask_cfgs(streams), dets, keep.reshape(-1), None, B, slots, stream0, kind)
    assert slots == 1 or (tot[0] > 0 and tot[1] > 0), tot


def test_filter_in_the_packed_layout_with_corrupted_prefixes():
    rs = np.random.RandomState(9)
    counts, cap, dc = (20, 0, 37, 64), 64, 13
    B, total = len(counts), sum(counts)
    prefix = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    dets = _rows(rs, B * cap, dc)                                       # the buffers have the decode's sizes: cap rows and cap + 1 words a frame
    keep = rs.randint(0, 5, size=B * (cap + 1)).astype(np.int32)
    for b, n in enumerate(counts):
        at = prefix[b] + b
        keep[at] = n - (3 if b == 0 else 0)
        keep[at + 1:at + 1 + n] = rs.permutation(n)
    keep[prefix[2] + 2 + 5] = 37                                        # an entry outside the frame's rows
    cfgs = _mask_cfgs(6)
    tot = _filter_case(cfgs, dets, keep, prefix, B, cap, 1, 'centre')
    assert tot[0] > 20 and tot[1] > 20, tot
    _filter_case(cfgs, dets, keep, prefix, B, cap, 0, 'bottom')         # frame 0 on a stream without a mask: copied
    _filter_case(cfgs, dets, keep, prefix, B, 16, 1, 'centre')          # fewer slots than rows: the counts are clamped to 16
    # a decreasing pair, a pair that ends beyond det_rows, a negative one: those frames have no list and nothing is written for them
    # (the pairs of the other frames do not overlap: frames whose rows overlap would write overlapping lists)
    for bad in ([30, 20, 20, 57, 121], [0, 20, 20, 1 << 20, 121], [-5, 20, 20, 57, 121], [0, 20, 20, 57, 257]):
        _filter_case(cfgs, dets, keep, np.asarray(bad, np.int32), B, cap, 1, 'centre')
    _filter_case(cfgs, dets, keep, prefix, B, cap, 1, 'centre', det_rows=100)            # det_rows below the last prefix


# ------------------------------------------------------------------------------------------------------------ update and append
class _ZDev:
    """zone state, counters, append state and arena on the device, with guards around each"""

    def __init__(self, streams, Tn, capacity, busy):
        self.streams, self.T, self.capacity = streams, Tn, capacity
        st, lines, regions = Z.new_state(streams, Tn)
        for s in busy:                                                   # streams outside the launch hold state of their own
            st[s]['owner_id'], st[s]['inside'], st[s]['px'], lines[s], regions[s] = 3, 5, 77, 7 + s, 9 + s
        self.busy = {s: (st[s].copy(), lines[s].copy(), regions[s].copy()) for s in busy}
        self.sizes = (st.size * 32, lines.size, regions.size, 4, capacity * 32)
        self.bufs = []
        for a, dt in ((_bits(st), torch.uint8), (lines.reshape(-1), torch.int64), (regions.reshape(-1), torch.int64),
                      (np.zeros(4, np.int64), torch.int64), (np.full(capacity * 32, FILL_B, np.uint8), torch.uint8)):
            whole, p = _guarded(a.size, dt, FILL_B if dt == torch.uint8 else FILL_I)
            whole[GUARD:GUARD + a.size] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            self.bufs.append((whole, p))

    def read(self):
        """(state STATE [streams, T], lines, regions, append state, arena bytes) after the containment checks"""
        out = [_inner(w, n, FILL_B if w.dtype == torch.uint8 else FILL_I, 'zone buffer %d' % i) for i, ((w, _), n) in
               enumerate(zip(self.bufs, self.sizes))]
        return (out[0].view(Z.STATE).reshape(self.streams, self.T), out[1].reshape(self.streams, 8, 2), out[2].reshape(self.streams, 8, 3),
                out[3], out[4])

    def snapshot(self):
        return [w.clone() for w, _ in self.bufs]


def _update(dev, tables, headers, tracks, B, stream0, min_hits, kind, commit=1, staged=None):
    """dbx_zone_update_batch called directly: (staged bytes [B, T * 24 * 32], counts [B]) with unwritten words FILL"""
    n = B * dev.T * 24 * 32
    stg, p_stg = _guarded(n, torch.uint8, FILL_B)
    cnt, p_cnt = _guarded(B, torch.int32, FILL_I)
    check(_lib.lib().dbx_zone_update_batch(ptr(tracks), ptr(headers), ptr(tables), dev.bufs[0][1], dev.bufs[1][1], dev.bufs[2][1], B,
                                           dev.streams, stream0, dev.T, min_hits, ZN.ANCHORS[kind], p_stg, p_cnt, commit, stream_ptr()))
    torch.cuda.synchronize()
    return _inner(stg, n, FILL_B, 'staged').reshape(B, -1), _inner(cnt, B, FILL_I, 'staged_count'), (stg, p_stg, cnt, p_cnt)


@pytest.mark.parametrize('case', Z.CASES, ids=lambda c: 'T%d-%s-min%d-cap%d' % (c[0], c[6], c[7], c[8]))
def test_update_and_append_equal_the_restatement_after_every_step(case):
    Tn, slots, objects, steps, B, variant, kind, min_hits, capacity = case
    tot, snaps, arena = Z.reference(case)
    cfgs, _ = Z.case_inputs(case)
    tables = _tables(cfgs)
    busy = [s for s in range(Z.STREAMS) if not Z.STREAM0 <= s < Z.STREAM0 + B]
    dev = _ZDev(Z.STREAMS, Tn, capacity, busy)
    L = _lib.lib()
    for step, snap in enumerate(snaps):
        headers = torch.from_numpy(snap['headers']).cuda()
        tracks = torch.from_numpy(_bits(snap['tracks']).copy()).cuda()
        if step in (0, 7, steps - 1):                                    # commit = 0 reads everything and leaves every buffer bit-identical
            before = dev.snapshot()
            stg, cnt, _ = _update(dev, tables, headers, tracks, B, Z.STREAM0, min_hits, kind, commit=0)
            assert (stg == FILL_B).all() and (cnt == FILL_I).all()
            assert all(torch.equal(a, w) for a, (w, _) in zip(before, dev.bufs))
        # the filter on the step's frames, in the slot layout: the lists the restated tracker was fed
        d = np.zeros((B, slots, 5))
        k = np.zeros((B, slots + 1), np.int32)
        for b, (r, l) in enumerate(snap['frames']):
            d[b, :r.shape[0]], k[b, 0], k[b, 1:1 + len(l)] = r, len(l), l
        kept = _filter_case(cfgs, d.reshape(B * slots, 5), k.reshape(-1), None, B, slots, Z.STREAM0, kind)
        assert kept[0] == sum(len(q) for q in snap['kept'])
        stg, cnt, raw = _update(dev, tables, headers, tracks, B, Z.STREAM0, min_hits, kind)
        for b in range(B):
            ev = snap['events'][b]
            assert cnt[b] == len(ev), (step, b, cnt[b], len(ev))
            assert np.array_equal(stg[b, :len(ev) * 32], _bits(ev)), (step, b, stg[b, :len(ev) * 32].view(Z.EVENT), ev)
            assert (stg[b, len(ev) * 32:] == FILL_B).all()
        check(L.dbx_zone_append(raw[1], raw[3], B, Tn, dev.bufs[4][1], capacity, dev.bufs[3][1], stream_ptr()))
        torch.cuda.synchronize()
        st, lines, regions, astate, ar = dev.read()
        assert np.array_equal(_bits(st[Z.STREAM0:Z.STREAM0 + B]), _bits(snap['zstate'][Z.STREAM0:Z.STREAM0 + B])), step
        assert np.array_equal(lines[Z.STREAM0:Z.STREAM0 + B], snap['lines'][Z.STREAM0:Z.STREAM0 + B]), step
        assert np.array_equal(regions[Z.STREAM0:Z.STREAM0 + B], snap['regions'][Z.STREAM0:Z.STREAM0 + B]), step
        for s in busy:                                                   # the neighbours' state and counters are untouched
            assert np.array_equal(_bits(st[s]), _bits(dev.busy[s][0])) and np.array_equal(lines[s], dev.busy[s][1])
            assert np.array_equal(regions[s], dev.busy[s][2])
        assert astate.tolist() == snap['astate'].tolist(), (step, astate, snap['astate'])
        n = snap['stored'] * 32
        assert np.array_equal(ar[:n], _bits(arena[:snap['stored']])) and (ar[n:] == FILL_B).all(), step
    assert snaps[-1]['astate'][2] == tot['fwd'] + tot['bwd'] + tot['enter'] + tot['exit'] + tot['ended'] > 0
    assert capacity >= 1 << 12 or snaps[-1]['astate'][1] > 0            # the small arenas dropped events, and the count is exact


# ------------------------------------------------------------------------------------------------------------ the front end
def _net(kind, dtype):
    net = getattr(D, kind)(synth.vgg19_standin(seed=0))
    synth.fill_params_(net, 11)
    # every pixel's box is 17 x 13 pixels around it, as in tests/test_hip_track.py
    with torch.no_grad():
        net.conv5_2_loc.weight.zero_()
        net.conv5_2_loc.bias.copy_(torch.tensor([2.0, 1.5, -2.0, -1.5]))
    net = net.cuda().eval()
    net.compute_dtype = dtype
    return net


def _scene_for(refs, kind='centre'):
    """A table made from the reference detections alone: the include polygon is the half plane left of the median anchor of the kept
    rows (so some rows stay and some go), a line runs along its edge and a region covers its upper part.  Pixels."""
    xs = sorted(Z.anchor(d[r], kind)[0] for ref in refs for d, keep in ref for r in keep)
    m = xs[len(xs) // 2] / 4.0 + 0.125
    half = [(-200, -200), (m, -200), (m, 400), (-200, 400)]
    return dict(lines=[((m - 8, -200), (m - 8, 400)), ((-200, 30), (400, 34))], regions=[[(-200, -200), (m, -200), (m, 32), (-200, 30)], half],
                include=[half], exclude=[[(2, 2), (6, 2), (6, 6), (2, 6)]])


class _Chain:
    """detect results -> restated filter -> tests/track_ref.py -> restated zone update and append, for streams stream0.. of `streams`"""

    def __init__(self, streams, Tn, scene, stream0, par, kind='centre', min_hits=1, capacity=1 << 16):
        self.cfgs = [Z.from_pixels(**scene) for _ in range(streams)]
        self.t, self.z = TR.new_state(streams, Tn), Z.new_state(streams, Tn)
        self.astate, self.arena = np.zeros(4, np.int64), []
        self.stream0, self.par, self.kind, self.min_hits, self.capacity = stream0, par, kind, min_hits, capacity
        self.kept = self.dropped = 0

    def step(self, ref):
        kept = [Z.filter_keep(self.cfgs[self.stream0 + b], d, k, self.kind) for b, (d, k) in enumerate(ref)]
        self.kept += sum(len(k) for k in kept)
        self.dropped += sum(len(k) for _, k in ref) - sum(len(k) for k in kept)
        res = TR.update_batch(self.t, [(d, kk) for (d, _), kk in zip(ref, kept)], self.stream0, **self.par)
        evs = Z.update_batch(self.cfgs, self.z, self.t, len(ref), self.stream0, self.min_hits, self.kind)
        Z.append(self.astate, self.arena, self.capacity, evs)
        return [(d, kk, r[0], r[2]) for (d, _), kk, r in zip(ref, kept, res)]

    def check(self, tr, zn):
        h, t = tr._host_state()
        assert h.tolist() == self.t[0].tolist() and np.array_equal(_bits(t), _bits(self.t[1]))
        st, lines, regions, astate = zn._host_state()
        assert np.array_equal(_bits(st), _bits(self.z[0])), (st, self.z[0])
        assert np.array_equal(lines, self.z[1]) and np.array_equal(regions, self.z[2]), (lines, self.z[1], regions, self.z[2])
        assert astate.tolist() == self.astate.tolist()
        got = zn.events()
        assert got.dtype == ZN.EVENT and np.array_equal(_bits(got), _bits(Z.as_events(self.arena)))
        c = zn.counts()
        assert np.array_equal(c[0], self.z[1]) and np.array_equal(c[1], self.z[2])


def _same(got, want):
    assert len(got) == len(want)
    for (d, keep, tid, hits), (wd, wkeep, wid, whits) in zip(got, want):
        assert np.array_equal(_bits(d), _bits(wd)) and list(keep) == list(wkeep), (keep, wkeep)
        assert tid.dtype == np.int32 and tid.tolist() == wid.tolist() and hits.tolist() == whits.tolist(), (tid, wid, hits, whits)


@pytest.mark.parametrize('mode', ['topk', 'thresh'])
@pytest.mark.parametrize('dtype', ['f32', 'f16'])
@pytest.mark.parametrize('kind', ['DenseBox', 'DenseBoxLMLOC'])
def test_watch_batch_is_detect_batch_plus_the_restated_chain(kind, dtype, mode, monkeypatch):
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
        kw = dict(score_thresh=float(np.float32(best[12])), max_dets=64)
        detect = lambda x: net.detect_batch_thresh(x, kw['score_thresh'], 64, max_batch=2)  # noqa: E731
    refs = [detect(X), detect(Y), detect(X)]
    scene = _scene_for(refs)
    par = dict(iou_thresh=0.3, max_age=1, alpha=0.5, beta=0.1, birth_score=-np.inf)
    plain = T.Tracker(5, max_tracks=64, max_age=1)
    before = net.track_batch(X, tracker=plain, stream0=1, max_batch=2, **kw)
    for env in (None, '0'):                                              # the graph, then the same launches without it
        if env is not None:
            monkeypatch.setenv('DBX_GRAPH', env)
        chain = _Chain(5, 64, scene, 1, par)
        tr = T.Tracker(5, max_tracks=64, max_age=1)
        zn = ZN.Zones(tr)
        for s in range(5):
            zn.set_stream(s, **scene)
        for x, ref in zip((X, list(Y), X), refs):
            _same(net.watch_batch(x, tracker=tr, zones=zn, stream0=1, max_batch=2, **kw), chain.step(ref))
            assert tr.headers()[:, 0].max() <= 3                         # the capture's warm-up runs did not count
            chain.check(tr, zn)
        print(kind, dtype, mode, env, 'kept', chain.kept, 'dropped', chain.dropped, 'events', chain.astate.tolist(),
              'kinds', np.bincount(Z.as_events(chain.arena)['kind'], minlength=5).tolist())
        assert chain.kept > 0 and chain.dropped > 0 and chain.astate[2] > 0          # from the restatement alone
        if env is None:
            assert sorted(k[0] for k in net._detect_graphs if k[0] == 'watch') == ['watch'] * 2          # chunks of 2 and 1 frames
    monkeypatch.delenv('DBX_GRAPH')
    # track_batch on the same net is what it was, and the other entries of the cache are not disturbed
    after = net.track_batch(X, tracker=T.Tracker(5, max_tracks=64, max_age=1), stream0=1, max_batch=2, **kw)
    for a, b in zip(before, after):
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and a[1] == b[1] and a[2].tolist() == b[2].tolist() and a[3].tolist() == b[3].tolist()
    assert all(np.array_equal(_bits(a), _bits(b)) and ka == kb for (a, ka), (b, kb) in zip(net.detect_batch(X, K=10, max_batch=2), top))


def test_set_stream_between_two_replays_needs_no_recapture(monkeypatch):
    monkeypatch.delenv('DBX_GRAPH', raising=False)
    net = _net('DenseBoxLMLOC', 'f16')
    rs = np.random.RandomState(29)
    X = torch.from_numpy(rs.randint(0, 256, size=(2, 64, 64, 3)).astype(np.uint8)).cuda()
    ref = net.detect_batch(X, K=10)
    scene = _scene_for([ref], 'bottom')
    par = dict(iou_thresh=0.3, max_age=1, alpha=0.5, beta=0.1, birth_score=-np.inf)
    chain = _Chain(2, 16, dict(), 0, par, kind='bottom')                # no table at first: nothing filtered, no events
    tr = T.Tracker(2, max_tracks=16, max_age=1)
    zn = ZN.Zones(tr, anchor='bottom')
    _same(net.watch_batch(X, tracker=tr, zones=zn), chain.step(ref))
    chain.check(tr, zn)
    assert chain.dropped == 0 and chain.astate[2] == 0
    graphs = [id(v[1]) for k, v in net._detect_graphs.items() if k[0] == 'watch']
    assert len(graphs) == 1
    zn.set_stream(1, **scene)                                            # stream 1 gets a table; stream 0 stays without
    chain.cfgs[1] = Z.from_pixels(**scene)
    _same(net.watch_batch(X, tracker=tr, zones=zn), chain.step(ref))
    chain.check(tr, zn)
    assert chain.dropped > 0 and chain.astate[2] > 0 and (zn.events()['stream'] == 1).all()
    assert [id(v[1]) for k, v in net._detect_graphs.items() if k[0] == 'watch'] == graphs          # the same graph replayed
    zn.reset()
    assert zn.events().shape == (0,) and not zn.counts()[1].any() and zn.table(1)['n_masks'] == 2


def test_update_batch_and_filter_keep_on_host_results():
    net = _net('DenseBoxLMLOC', 'f16')
    rs = np.random.RandomState(23)
    x = torch.from_numpy(rs.randint(0, 256, size=(3, 64, 64, 3)).astype(np.uint8)).cuda()
    res = net.detect_batch(x, K=10)
    res.append((np.zeros((0, 13)), []))                                  # an image without rows
    scene = _scene_for([res])
    chain = _Chain(6, 8, scene, 2, dict(max_age=0), min_hits=2, capacity=5)
    tr = T.Tracker(6, max_tracks=8, max_age=0)
    zn = ZN.Zones(tr, min_hits=2, capacity=5)
    for s in range(6):
        zn.set_stream(s, **scene)
    for step in range(4):
        frames = res if step != 2 else res[::-1]                         # other streams' rows: retirements inside regions and births
        want = chain.step(frames)
        dets, keeps = [d for d, _ in frames], [k for _, k in frames]
        dets[1] = torch.from_numpy(dets[1]).cuda()                       # a device result among host ones
        assert ZN.filter_keep(dets, keeps, zones=zn, stream0=2) == [w[1] for w in want]
        out = ZN.update_batch(dets, keeps, tracker=tr, zones=zn, stream0=2)
        assert len(out) == 4
        for (keep, tid, hits), w in zip(out, want):
            assert keep == w[1] and tid.dtype == np.int32 and tid.tolist() == w[2].tolist() and hits.tolist() == w[3].tolist()
    st, lines, regions, astate = zn._host_state()
    assert np.array_equal(_bits(st), _bits(chain.z[0])) and np.array_equal(regions, chain.z[2]) and np.array_equal(lines, chain.z[1])
    assert astate.tolist() == chain.astate.tolist() and astate[0] == 5 and astate[1] > 0
    assert np.array_equal(zn._events.cpu().numpy(), _bits(Z.as_events(chain.arena)))
    with pytest.raises(RuntimeError, match='events did not fit'):
        zn.events()
    assert chain.kept > 0 and chain.dropped > 0
