"""The best-shot gallery on the GPU: dbx_crop_sharpness == the NumPy restatement (tests/gallery_ref.py) at the sizes that cross a wave,
the workgroup and the LDS bound; dbx_track_gallery_update == the restatement bit for bit -- shots, crops, arena, arena crops and counters
after every step of seeded 8-frame sequences, the other streams' entries untouched, nothing written outside the buffers; commit = 0
writes nothing; net.track_plate_crops == detect_plate_crops + the two restatements, through the hipGraph and without it;
gallery.update_batch on host results gives the same state."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import densebox_amd as D
from densebox_amd import _lib, gallery as G, synth, track as T
from densebox_amd._lib import check, ptr, stream_ptr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gallery_ref as GR  # noqa: E402
import track_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64                     # sentinel elements in front of and behind every output (a multiple of 16 bytes: the alignment stays)
FILL_B = 0xEE


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class _Guarded:
    """a device buffer with sentinels around it, initialised from a host array"""

    def __init__(self, host):
        self.host = _bits(host)
        self.n = self.host.size
        self.whole = torch.full((self.n + 2 * GUARD,), FILL_B, dtype=torch.uint8, device='cuda')
        self.whole[GUARD:GUARD + self.n] = torch.from_numpy(self.host.copy()).cuda()
        self.ptr = C.c_void_p(self.whole.data_ptr() + GUARD)

    def read(self, name):
        h = self.whole.cpu().numpy()
        assert (h[:GUARD] == FILL_B).all() and (h[GUARD + self.n:] == FILL_B).all(), 'bytes outside %s were written' % name
        return h[GUARD:GUARD + self.n]


# ------------------------------------------------------------------------------------------------------------ sharpness
SIZES = [(1, 1), (2, 5), (3, 3), (65, 3), (3, 65), (94, 24), (257, 3), (128, 128)]           # (ow, oh)


@pytest.mark.parametrize('ow,oh', SIZES)
def test_crop_sharpness_equals_the_restatement(ow, oh):
    rs = np.random.RandomState(ow * 1000 + oh)
    for c in (1, 3):
        crops = rs.randint(0, 256, size=(257, oh, ow, c)).astype(np.uint8)
        want = GR.sharpness(crops)
        assert (want > 0).all() if oh >= 3 and ow >= 3 else not want.any()
        dev = torch.from_numpy(crops).cuda()
        for n in (1, 3, 257):
            out = _Guarded(np.full(n, -777, np.int64))
            check(_lib.lib().dbx_crop_sharpness(ptr(dev), n, oh, ow, c, out.ptr, stream_ptr()))
            torch.cuda.synchronize()
            got = out.read('out').view(np.int64)
            assert got.tolist() == want[:n].tolist(), (c, n)
        odd = torch.empty(crops.size + 1, dtype=torch.uint8, device='cuda')                  # crops that start on an odd address
        odd[1:] = dev.reshape(-1)
        got = torch.empty(3, dtype=torch.int64, device='cuda')
        check(_lib.lib().dbx_crop_sharpness(C.c_void_p(odd.data_ptr() + 1), 3, oh, ow, c, ptr(got), stream_ptr()))
        assert got.cpu().tolist() == want[:3].tolist(), c
    assert G.sharpness(crops[:5]).tolist() == want[:5].tolist()                              # numpy in, numpy out
    t = G.sharpness(dev[:5])
    assert t.is_cuda and t.dtype == torch.int64 and t.cpu().tolist() == want[:5].tolist()


def test_checkerboard_needs_64_bit_sums():
    yy, xx = np.mgrid[:128, :128]
    board = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[None, :, :, None], 3, axis=3)
    want = 4080 ** 2 * 126 * 126
    assert want > 1 << 32
    assert G.sharpness(board).tolist() == [want] == GR.sharpness(board).tolist()
    assert G.sharpness(np.ascontiguousarray(board[..., :1])).tolist() == [want]


# ------------------------------------------------------------------------------------------------------------ the update kernel
class _DevGallery:
    """a restatement gallery's buffers on the device, guarded"""

    def __init__(self, gal):
        self.bufs = {k: _Guarded(gal[k]) for k in ('shots', 'crops', 'arena', 'arena_crops', 'gstate')}
        self.streams, self.T, self.oh, self.ow, self.c = gal['crops'].shape
        self.capacity = gal['arena'].shape[0]

    def launch(self, state, res, crops, ok, cursor, stream0, policy, min_score, commit=1):
        """dbx_track_gallery_update on the tracker state and the per-frame results of the restatement"""
        B, slots = ok.shape
        slot = np.full((B, slots), -1, np.int32)
        retired = np.full((B, self.T, R.TRACK.itemsize), FILL_B, np.uint8)
        tally = np.zeros((B, 6), np.int32)
        for b, r in enumerate(res):
            slot[b, :len(r[1])] = r[1]
            retired[b, :len(r[3])] = _bits(r[3]).reshape(len(r[3]), R.TRACK.itemsize)
            tally[b] = r[4]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        d = [up(_bits(state[1])), up(state[0]), up(slot), up(crops), up(ok.astype(np.int32)), up(retired), up(tally),
             up(np.array([cursor, 0, 0, 0], np.int64))]
        g = self.bufs
        check(_lib.lib().dbx_track_gallery_update(*[ptr(t) for t in d], g['shots'].ptr, g['crops'].ptr, g['arena'].ptr, g['arena_crops'].ptr,
                                                  g['gstate'].ptr, B, slots, self.streams, stream0, self.T, self.oh, self.ow, self.c,
                                                  self.capacity, policy, min_score, commit, stream_ptr()))
        torch.cuda.synchronize()

    def equals(self, gal):
        for k, buf in self.bufs.items():
            got = buf.read(k)
            if k in ('shots', 'arena'):
                for name in GR.SHOT.names:
                    a = got.view(gal[k].dtype)
                    a, w = (a[name], gal[k].reshape(-1)[name]) if k == 'shots' else (a['shot'][name], gal[k]['shot'][name])
                    assert np.array_equal(_bits(a), _bits(w)), (k, name, a, w)
            assert np.array_equal(got, _bits(gal[k])), k


def _run_case(case, size, total):
    sc, calls = GR.case_script(case, size)
    stream0, policy = case[4], case[7]
    dev = _DevGallery(sc.gal)
    for frames, crops, ok, with_gallery in calls:
        cursor = int(sc.astate[0])
        res = sc.step(frames, crops, ok, stream0=stream0, gallery=with_gallery)
        if with_gallery:
            dev.launch(sc.state, res, crops, ok, cursor, stream0, policy, GR.MIN_SCORE)
        dev.equals(sc.gal)                                             # the whole gallery, the neighbours' entries included
    assert all(sc.events[name] > 0 for name in ('adopt', 'first', 'replace')), sc.events
    for name in GR.EVENTS:
        total[name] += sc.events[name]
    return sc, dev


@pytest.mark.parametrize('case', GR.CASES)
def test_kernel_equals_the_restatement_after_every_step(case):
    _run_case(case, (7, 5), dict.fromkeys(GR.EVENTS, 0))


def test_no_branch_passed_vacuously():
    """a condition, from the restatement's events alone: over the whole case list every branch ran"""
    total = dict.fromkeys(GR.EVENTS, 0)
    for case in GR.CASES:
        sc, calls = GR.case_script(case)
        for frames, crops, ok, with_gallery in calls:
            sc.step(frames, crops, ok, stream0=case[4], gallery=with_gallery)
        for name in GR.EVENTS:
            total[name] += sc.events[name]
    assert all(total[name] > 0 for name in ('stored', 'dropped', 'lost', 'reborn', 'coast', 'notok', 'gated', 'first', 'replace', 'keep')), total


def test_kernel_at_the_plate_size():
    """the third case with 94 x 24 crops: 6768 bytes, whole 16-byte words"""
    _run_case(GR.CASES[2], (94, 24), dict.fromkeys(GR.EVENTS, 0))


def test_commit_zero_writes_nothing():
    case = GR.CASES[2]
    sc, calls = GR.case_script(case)
    for frames, crops, ok, with_gallery in calls[:2]:
        sc.step(frames, crops, ok, stream0=case[4], gallery=with_gallery)
    dev = _DevGallery(sc.gal)
    before = {k: b.whole.cpu().numpy().copy() for k, b in dev.bufs.items()}
    frames, crops, ok, _ = calls[2]                                    # slot 0 retires here and is taken again
    cursor = int(sc.astate[0])
    res = R.update_batch(sc.state, frames, case[4], **sc.params)
    ev = GR.update(sc.gal, sc.state, res, crops, ok, cursor, case[4], sc.policy, sc.min_score, commit=False)
    assert min(ev['stored'], ev['reborn'], ev['first'], ev['replace']) > 0, ev                           # a commit would have written
    dev.launch(sc.state, res, crops, ok, cursor, case[4], case[7], GR.MIN_SCORE, commit=0)
    for k, b in dev.bufs.items():
        assert np.array_equal(b.whole.cpu().numpy(), before[k]), k
    dev.launch(sc.state, res, crops, ok, cursor, case[4], case[7], GR.MIN_SCORE, commit=1)               # and the same launch, committed
    GR.update(sc.gal, sc.state, res, crops, ok, cursor, case[4], sc.policy, sc.min_score)
    dev.equals(sc.gal)


# ------------------------------------------------------------------------------------------------------------ net.track_plate_crops
WEIGHT_SEED = 11               # synth.fill_params_ seed of the stand-in heads: with it the composition alone leaves live entries with shots
SIZE = (94, 24)


def _net(kind, dtype):
    net = getattr(D, kind)(synth.vgg19_standin(seed=0))
    synth.fill_params_(net, WEIGHT_SEED)
    # every pixel's box is 17 x 13 pixels around it, as in tests/test_hip_track.py: the same frame again matches its own tracks
    with torch.no_grad():
        net.conv5_2_loc.weight.zero_()
        net.conv5_2_loc.bias.copy_(torch.tensor([2.0, 1.5, -2.0, -1.5]))
    net = net.cuda().eval()
    net.compute_dtype = dtype
    return net


def _frames():
    rs = np.random.RandomState(17)
    X = torch.from_numpy(rs.randint(0, 256, size=(3, 64, 96, 3)).astype(np.uint8)).cuda()
    Y = torch.from_numpy(rs.randint(0, 256, size=(3, 64, 96, 3)).astype(np.uint8)).cuda()
    return [X, X, Y, X, Y]


def _composition(net, calls, policy, K=10):
    """detect_plate_crops per call, track_ref for ids and hits, the gallery restatement for the gallery: (refs, wants, Scripted)"""
    sc = GR.Scripted(4, 16, SIZE, 3, 8, policy=G.POLICIES[policy], max_age=0)
    cache, refs, wants = {}, [], []
    for x in calls:
        if id(x) not in cache:
            cache[id(x)] = net.detect_plate_crops(x, size=SIZE, K=K)
        ref = cache[id(x)]
        crops = np.zeros((len(ref), K, SIZE[1], SIZE[0], 3), np.uint8)
        ok = np.zeros((len(ref), K), np.int32)
        for b, (_, keep, c, o) in enumerate(ref):
            crops[b, :len(keep)] = c.cpu().numpy()
            ok[b, :len(keep)] = o
        refs.append(ref)
        wants.append(sc.step([(d, keep) for d, keep, _, _ in ref], crops, ok, stream0=1))
    return refs, wants, sc


def _same_gallery(gal, tr, sc):
    live = gal.live()
    want = GR.live(sc.gal)
    assert len(live) == len(want) == 4
    for (s, c), (ws, wc) in zip(live, want):
        assert s.dtype == G.SHOT and np.array_equal(_bits(s), _bits(ws)), (s, ws)
        assert c.dtype == np.uint8 and np.array_equal(c, wc)
    rec, crops, valid = gal.finished()
    m = min(int(sc.astate[0]), gal.capacity)
    assert rec.shape == (m,) and crops.shape == (m, SIZE[1], SIZE[0], 3) and valid.tolist() == (sc.gal['arena']['shot']['id'][:m] >= 0).tolist()
    assert np.array_equal(_bits(rec), _bits(sc.gal['arena'][:m])) and np.array_equal(crops, sc.gal['arena_crops'][:m])
    assert gal.counters() == tuple(int(v) for v in sc.gal['gstate'])
    done = tr.finished()
    assert np.array_equal(_bits(done), _bits(R.as_records(sc.records)))
    for i in np.nonzero(valid)[0]:                                      # the contract: the same index is the same track
        assert rec[i]['stream'] == done[i]['stream'] and rec[i]['shot']['id'] == done[i]['t']['id']
    h, t = tr._host_state()
    assert h.tolist() == sc.state[0].tolist() and np.array_equal(_bits(t), _bits(sc.state[1]))
    return sum(int((s['shots'] > 0).sum()) for s, _ in live), int(valid.sum())


@pytest.mark.parametrize('dtype', ['f32', 'f16'])
@pytest.mark.parametrize('kind', ['DenseBoxLM', 'DenseBoxLMLOC'])
def test_track_plate_crops_is_detect_plate_crops_plus_the_restatements(kind, dtype, monkeypatch):
    monkeypatch.delenv('DBX_GRAPH', raising=False)
    net = _net(kind, dtype)
    policy = 'sharpness' if kind == 'DenseBoxLM' else 'score'
    calls = _frames()
    refs, wants, sc = _composition(net, calls, policy)
    print(kind, dtype, 'events', sc.events, 'gstate', sc.gal['gstate'].tolist())
    for env in (None, '0'):                                             # the graph, then the same launches without it
        if env is not None:
            monkeypatch.setenv('DBX_GRAPH', env)
        tr = T.Tracker(4, max_tracks=16, max_age=0)
        gal = G.PlateGallery(tr, size=SIZE, policy=policy, capacity=8)
        for n, (x, ref, want) in enumerate(zip(calls, refs, wants)):
            got = net.track_plate_crops(x if n != 3 else list(x), tracker=tr, gallery=gal, stream0=1, K=10, max_batch=2)
            assert tr.headers()[:, 0].tolist() == [0, n + 1, n + 1, n + 1]        # every call counts exactly once: no trace of warm-ups
            for (d, keep, tid, hits), (rd, rkeep, _, _), w in zip(got, ref, want):
                assert np.array_equal(_bits(d), _bits(rd)) and keep == rkeep
                assert tid.dtype == np.int32 and tid.tolist() == w[0].tolist() and hits.tolist() == w[2].tolist()
        shots, stored = _same_gallery(gal, tr, sc)
        assert shots > 0 and stored > 0, (shots, stored)                 # a condition on the composition: WEIGHT_SEED is chosen for it
        if env is None:
            assert sorted(k[0] for k in net._detect_graphs if k[0] == 'track_plate_crops') == ['track_plate_crops'] * 2
        gal.reset()
        assert gal.counters() == (0, 0, 0, 0) and gal.finished()[0].shape == (0,) and all(s.shape == (0,) for s, _ in gal.live())
        assert not tr.headers().any()


def test_update_batch_on_host_results_gives_the_same_gallery():
    net = _net('DenseBoxLMLOC', 'f16')
    calls = _frames()
    tr1 = T.Tracker(4, max_tracks=16, max_age=0)
    g1 = G.PlateGallery(tr1, size=SIZE, policy='sharpness', min_score=-1e30, capacity=8)
    tr2 = T.Tracker(4, max_tracks=16, max_age=0)
    g2 = G.PlateGallery(tr2, size=SIZE, policy='sharpness', min_score=-1e30, capacity=8)
    for n, x in enumerate(calls):
        a = net.track_plate_crops(x, tracker=tr1, gallery=g1, stream0=1, K=10)
        res = net.detect_batch(x, K=10)
        images = x if n % 2 == 0 else [im.cpu().numpy() for im in x]     # a device batch, or frames on the host
        b = G.update_batch(images, [d for d, _ in res], [k for _, k in res], tracker=tr2, gallery=g2, stream0=1)
        for (_, keep, tid, hits), (tid2, hits2) in zip(a, b):
            assert tid2.dtype == np.int32 and tid.tolist() == tid2.tolist() and hits.tolist() == hits2.tolist() and len(tid2) == len(keep)
    for (s1, c1), (s2, c2) in zip(g1.live(), g2.live()):
        assert np.array_equal(_bits(s1), _bits(s2)) and np.array_equal(c1, c2)
    f1, f2 = g1.finished(), g2.finished()
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(f1, f2)) and f1[2].sum() > 0
    assert g1.counters() == g2.counters() and g1.counters()[0] > 0
    assert np.array_equal(_bits(tr1.finished()), _bits(tr2.finished()))
    assert sum(int((s['shots'] > 0).sum()) for s, _ in g1.live()) > 0
