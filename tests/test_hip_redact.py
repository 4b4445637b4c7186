"""Plate redaction on the GPU: dbx_redact_batch == the NumPy restatement (tests/redact_ref.py) bit for bit -- the crafted rows and tracks of
tests/redact_cases.py on frames from 1 x 1 to several tiles with 1, 3 and 4 channels, the three methods and both shapes, from even and
odd addresses, nothing written outside the frames, fill also in place; the LDS bound of 1024 rows + 256 tracks; the packed layout behind
the threshold decode and corrupted prefixes; frame records that must be skipped; a seeded mixed-size batch; redact.redact_batch on host
results; net.redact_batch == detect_batch / track_batch + the restatement over three calls with coasting tracks, through the hipGraph
and without it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import densebox_amd as D
from densebox_amd import _lib, decode as DC, redact, synth, track as T
from densebox_amd._lib import check, ptr, stream_ptr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import redact_cases as RC  # noqa: E402
import redact_ref as V  # noqa: E402
import thresh_ref  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64                     # sentinel bytes in front of and behind every output frame
FILL_B = 0xEE


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class _Frame:
    """one frame on the device: the source in a buffer of its own and, out of place, a destination between sentinels; odd: both start on
    an odd address"""

    def __init__(self, img, in_place=False, odd=False):
        self.img, self.n, self.off = img, img.size, GUARD + (1 if odd else 0)
        self.whole = torch.full((self.n + 2 * GUARD + 1,), FILL_B, dtype=torch.uint8, device='cuda')
        flat = torch.from_numpy(np.ascontiguousarray(img).reshape(-1)).cuda()
        if in_place:
            self.whole[self.off:self.off + self.n] = flat
            self.src = self.dst = self.whole.data_ptr() + self.off
        else:
            self.keep = torch.empty(self.n + 1, dtype=torch.uint8, device='cuda')
            self.keep[int(odd):int(odd) + self.n] = flat
            self.src, self.dst = self.keep.data_ptr() + (1 if odd else 0), self.whole.data_ptr() + self.off
        self.in_place, self.odd = in_place, odd

    def read(self):
        h = self.whole.cpu().numpy()
        assert (h[:self.off] == FILL_B).all() and (h[self.off + self.n:] == FILL_B).all(), 'bytes outside dst were written'
        if not self.in_place:                                     # the source is read only
            assert np.array_equal(self.keep.cpu().numpy()[int(self.odd):int(self.odd) + self.n], self.img.reshape(-1))
        return h[self.off:self.off + self.n].reshape(self.img.shape)


def _table(frames, records=None):
    rec = (_lib.OverlayFrame * len(frames))()
    for i, (r, f) in enumerate(zip(rec, frames)):
        r.src, r.dst, r.h, r.w = f.src, f.dst, f.img.shape[0], f.img.shape[1]
        if records and i in records:
            for k, v in records[i].items():
                setattr(r, k, v)
    return torch.frombuffer(rec, dtype=torch.uint8).cuda()


def _slot_inputs(rows, keeps, slots, dc):
    """device arrays in dbx_detect_batch's slot layout; keeps[b] is the raw keep record [count, entries...] (any count)"""
    B = len(rows)
    d = np.zeros((B, slots, dc), np.float64)
    k = np.zeros((B, slots + 1), np.int32)
    for b in range(B):
        d[b, :rows[b].shape[0]] = rows[b]
        k[b, :len(keeps[b])] = keeps[b][:slots + 1]
    return torch.from_numpy(d.reshape(B * slots, dc)).cuda(), torch.from_numpy(k).cuda()


def _track_table(per_frame, stream0=1, extra=1):
    """device table [stream0 + B + extra][max_tracks]: frame b's slots in stream stream0 + b; every other stream holds one coasting track
    over everything, which shows if a frame reads a stream that is not its own"""
    mt = max(1, max(t.size for t in per_frame))
    streams = stream0 + len(per_frame) + extra
    tab = np.zeros((streams, mt), T.TRACK)
    tab['id'] = -1
    tab['id'][:, 0], tab['age'][:, 0], tab['box'][:, 0] = 1, 1, [-1e6, -1e6, 1e6, 1e6]
    for b, t in enumerate(per_frame):
        tab[stream0 + b] = np.zeros(mt, T.TRACK)
        tab['id'][stream0 + b] = -1
        tab[stream0 + b, :t.size] = t
    return torch.from_numpy(tab.view(np.uint8).reshape(-1)).cuda(), streams, stream0, mt


def _launch(frames, c, dets, dc, det_rows, keep, prefix, slots, tracks, style, records=None, max_hw=None):
    table = _table(frames, records)
    mh, mw = max_hw or (max(f.img.shape[0] for f in frames), max(f.img.shape[1] for f in frames))
    tab, streams, stream0, mt = tracks if tracks is not None else (None, 0, 0, 0)
    rec = redact.Redaction(**style).record(dc, 0)
    check(_lib.lib().dbx_redact_batch(ptr(table), len(frames), c, mh, mw, ptr(dets), dc, det_rows, ptr(keep), ptr(prefix), slots, ptr(tab),
                                      streams, stream0, mt, C.byref(rec), stream_ptr()))
    torch.cuda.synchronize()


def _check_slot_case(imgs, rows, keeps, slots, dc, c, tracks, style, in_place=False, odd=False):
    """one launch in slot layout against the restatement, frame by frame; returns the redacted frames"""
    frames = [_Frame(im, in_place, odd) for im in imgs]
    d, k = _slot_inputs(rows, keeps, slots, dc)
    _launch(frames, c, d, dc, len(imgs) * slots, k, None, slots, None if tracks is None else _track_table(tracks), style)
    out = []
    for b, f in enumerate(frames):
        padded = np.zeros((slots, dc))
        padded[:rows[b].shape[0]] = rows[b]
        kl = RC.effective(list(keeps[b]) + [0] * (slots + 1 - len(keeps[b])), slots, slots)
        want = V.redact(f.img, padded, kl, None if tracks is None else tracks[b], style)
        got = f.read()
        assert np.array_equal(got, want), (b, f.img.shape, style, in_place, odd, np.argwhere((got != want).any(axis=2))[:5])
        out.append(got)
    return out


# ------------------------------------------------------------------------------------------------------------ crafted rows
@pytest.mark.parametrize('c', [1, 3, 4])
@pytest.mark.parametrize('h,w', [(1, 1), (5, 7), (17, 33), (48, 64), (67, 130)])
def test_kernel_equals_restatement_on_crafted_rows(h, w, c):
    rs = np.random.RandomState(h * 100 + w + c)
    img = rs.randint(0, 256, size=(h, w, c)).astype(np.uint8)
    rows, tr = RC.crafted(h, w), RC.tracks(h, w)
    n = rows.shape[0]
    lists = RC.keep_lists(h, w)
    for si, style in enumerate(RC.styles()):
        for odd in (False, True):
            got = _check_slot_case([img], [rows], [lists[0]], n, 13, c, [tr] if (si + odd) % 2 else None, style, False, odd)
        if style['method'] == 'fill':
            _check_slot_case([img], [rows], [lists[0]], n, 13, c, [tr], style, True, False)                     # in place
            _check_slot_case([img], [rows], [lists[0]], n, 13, c, None, style, True, True)
            if h >= 17:
                assert not np.array_equal(got[0], img)
    # entries out of range, a count above slots, no kept rows (the tracks remain), five columns under a quad style
    for style in (RC.styles()[3], RC.styles()[15]):
        _check_slot_case([img], [rows], [lists[1]], n, 13, c, [tr], style)
        _check_slot_case([img], [rows], [lists[2]], n, 13, c, None, style, False, True)
        _check_slot_case([img], [rows], [[0] + lists[0][1:]], n, 13, c, [tr], style)
        got = _check_slot_case([img], [rows], [[-3] + lists[0][1:]], n, 13, c, None, style)
        assert np.array_equal(got[0], img)
        _check_slot_case([img], [rows[:, :5]], [lists[0]], n, 5, c, [tr], style)


def test_1024_rows_and_256_tracks_on_one_frame():
    """the LDS bound: every list position and every track slot holds a region, all of them on the left of one 67 x 130 frame"""
    rs = np.random.RandomState(1024)
    img = rs.randint(0, 256, size=(67, 130, 4)).astype(np.uint8)
    rows = np.zeros((1024, 5))
    rows[:, 0], rows[:, 1] = rs.randint(0, 70, 1024), rs.randint(0, 66, 1024)
    rows[:, 2], rows[:, 3], rows[:, 4] = rows[:, 0] + 1, rows[:, 1] + 1, rs.rand(1024)
    tr = np.zeros(256, T.TRACK)
    tr['id'], tr['age'] = np.arange(256), rs.randint(1, RC.COAST + 1, 256)
    tr['box'][:, 0], tr['box'][:, 1] = rs.randint(0, 70, 256), rs.randint(0, 66, 256)
    tr['box'][:, 2], tr['box'][:, 3] = tr['box'][:, 0] + 2, tr['box'][:, 1] + 1
    order = [int(v) for v in rs.permutation(1024)]
    for m in (dict(method='blur', radius=16), dict(method='pixelate', cell=7), dict(method='fill')):
        style = dict(RC.BASE, shape='box', grow=0, grow_pct=0, min_score=-1.0, **m)
        got = _check_slot_case([img], [rows], [[1024] + order], 1024, 5, 4, [tr], style)
        assert np.array_equal(got[0][:, 80:], img[:, 80:]) and not np.array_equal(got[0][:, :80], img[:, :80])
    count = V.covered(67, 130, rows, order, tr, style)
    assert count.max() >= 3 and (count[:, :72] == 0).any()


# ------------------------------------------------------------------------------------------------------------ packed layout
def _thresh_decode(counts, cap=64):
    """dbx_detect_thresh_batch on crafted 16 x 16 maps, one image per entry of counts: (dets, keep, counts) device tensors and per image
    the host (rows, keep list)"""
    images = [thresh_ref.craft_maps(40 + i, 16, 16, n, 4) for i, n in enumerate(counts)]
    maps = {k: torch.from_numpy(np.ascontiguousarray(np.concatenate([m[k] for m in images]))).cuda() for k in images[0]}
    dets, keep, cnt = DC._run_thresh_batch(maps['score'], maps['loc'], 0.5, cap, maps['lm_heat'], maps['lm_loc'], 0.4, lists_behind_rows=False)
    torch.cuda.synchronize()
    B = len(counts)
    c, d, k = cnt.cpu().numpy(), dets.cpu().numpy(), keep.cpu().numpy()
    prefix = c[2 * B:]
    assert [int(c[2 * b]) for b in range(B)] == list(counts)
    host = []
    for b in range(B):
        p, n = int(prefix[b]), int(c[2 * b])
        l = k[p + b:p + b + n + 1]
        host.append((d[p:p + n].copy(), [int(v) for v in l[1:1 + int(l[0])]]))
    return dets, keep, cnt, host


def test_packed_layout_behind_the_threshold_decode_and_corrupted_prefixes():
    counts, cap, B = (20, 0, 37), 64, 3
    dets, keep, cnt, host = _thresh_decode(counts, cap)
    rs = np.random.RandomState(3)
    imgs = [rs.randint(0, 256, size=s).astype(np.uint8) for s in ((64, 64, 3), (40, 50, 3), (70, 61, 3))]
    trs = [RC.tracks(*im.shape[:2]) for im in imgs]
    tab = _track_table(trs)
    none = (np.zeros((0, 13)), [])
    d_all, k_all = dets.cpu().numpy(), keep.cpu().numpy()
    l2 = k_all[10 + 2:10 + 2 + 47 + 1]
    odd = (d_all[10:57].copy(), [int(v) for v in l2[1:1 + min(max(int(l2[0]), 0), 47)]])
    cases = [(cnt[2 * B:], host),
             (torch.tensor([0, 20, 10, 57], dtype=torch.int32, device='cuda'), [host[0], none, odd]),         # decreasing: frame 1 is empty
             (torch.tensor([0, 20, 20, 1 << 20], dtype=torch.int32, device='cuda'), [host[0], none, none]),   # beyond det_rows
             (torch.tensor([-5, 20, 20, 57], dtype=torch.int32, device='cuda'), [none, none, host[2]])]       # negative
    for ci, (prefix, want_frames) in enumerate(cases):
        style = dict(RC.BASE, shape=None, min_score=-1.0, **RC.METHODS[(1, 5, 0, 7)[ci]])
        frames = [_Frame(im) for im in imgs]
        _launch(frames, 3, dets, 13, int(dets.numel()) // 13, keep, prefix, cap, tab, style)
        for b, (f, (rows, kl)) in enumerate(zip(frames, want_frames)):
            got = f.read()
            assert np.array_equal(got, V.redact(f.img, rows, kl, trs[b], style)), (ci, b)
            if not kl:                                                                                         # copied, its coasting tracks redacted
                assert np.array_equal(got, V.redact(f.img, none[0], [], trs[b], style))
                if style['method'] == 'fill':
                    assert not np.array_equal(got, f.img)
        frames = [_Frame(im) for im in imgs]                                                                   # ... and without tracks: a copy
        _launch(frames, 3, dets, 13, int(dets.numel()) // 13, keep, prefix, cap, None, style)
        for b, (f, (rows, kl)) in enumerate(zip(frames, want_frames)):
            got = f.read()
            assert np.array_equal(got, V.redact(f.img, rows, kl, None, style)), (ci, b)
            if not kl:
                assert np.array_equal(got, f.img)


def test_bad_frame_records_and_in_place_records_are_skipped():
    rs = np.random.RandomState(8)
    imgs = [rs.randint(0, 256, size=(30, 40, 3)).astype(np.uint8) for _ in range(7)]
    rows = [np.array([[5.0, 12.0, 25.0, 22.0, 0.5]])] * 7
    d, k = _slot_inputs(rows, [[1, 0]] * 7, 2, 5)
    records = {1: dict(src=None), 2: dict(dst=None), 3: dict(h=31), 4: dict(w=41), 5: dict(h=0)}
    for m in RC.METHODS[0], RC.METHODS[2], RC.METHODS[6]:
        style = dict(RC.BASE, shape='box', **m)
        frames = [_Frame(im, in_place=(i == 6)) for i, im in enumerate(imgs)]
        before = [f.whole.clone() for f in frames]
        _launch(frames, 3, d, 5, 14, k, None, 2, None, style, records=records, max_hw=(30, 40))
        assert np.array_equal(frames[0].read(), V.redact(imgs[0], rows[0], [0], None, style))
        for f, b in zip(frames[1:6], before[1:6]):
            assert torch.equal(f.whole, b)                                                                     # sentinel-filled, untouched
        if m['method'] == 'fill':
            assert np.array_equal(frames[6].read(), V.redact(imgs[6], rows[6], [0], None, style))
        else:
            assert torch.equal(frames[6].whole, before[6])                                                     # dst == src: skipped


def _random_batch(seed, sizes, K=10, c=3):
    rs = np.random.RandomState(seed)
    imgs, rows, keeps, trs = [], [], [], []
    for h, w in sizes:
        imgs.append(rs.randint(0, 256, size=(h, w, c)).astype(np.uint8))
        r = np.zeros((K, 13))
        r[:, 0], r[:, 1] = rs.uniform(-10, w, K), rs.uniform(-10, h, K)
        r[:, 2], r[:, 3] = r[:, 0] + rs.uniform(-5, 0.3 * w, K), r[:, 1] + rs.uniform(-5, 0.25 * h, K)
        r[:, 4] = rs.uniform(0, 1, K)
        for q, (ix, iy) in enumerate(((0, 1), (2, 1), (2, 3), (0, 3))):                   # landmarks around the box's corners
            r[:, 5 + 2 * q], r[:, 6 + 2 * q] = r[:, ix] + rs.uniform(-4, 4, K), r[:, iy] + rs.uniform(-4, 4, K)
        k = rs.randint(0, K + 1)
        rows.append(r)
        keeps.append([int(v) for v in rs.permutation(K)[:k]])
        t = np.zeros(12, T.TRACK)
        t['id'], t['age'] = rs.randint(-1, 50, 12), rs.randint(0, RC.COAST + 2, 12)         # ages spread over 0..coast + 1
        t['box'][:, 0], t['box'][:, 1] = rs.uniform(-5, w, 12), rs.uniform(-5, h, 12)
        t['box'][:, 2], t['box'][:, 3] = t['box'][:, 0] + rs.uniform(0, 0.2 * w, 12), t['box'][:, 1] + rs.uniform(0, 0.2 * h, 12)
        trs.append(t)
    return imgs, rows, keeps, trs


def test_seeded_batch_of_mixed_sizes_with_tracks():
    sizes = [(64, 64), (37, 211), (130, 67), (1, 300), (200, 3), (96, 129)]
    imgs, rows, keeps, trs = _random_batch(77, sizes)
    assert {int(a) for t in trs for a in t['age']} == set(range(RC.COAST + 2))
    for m in (dict(method='fill'), dict(method='pixelate', cell=12), dict(method='blur', radius=8)):
        style = dict(RC.BASE, shape=None, grow=2, grow_pct=25, min_score=0.2, **m)
        got = _check_slot_case(imgs, rows, [[len(k)] + k for k in keeps], 10, 13, 3, trs, style, False, m['method'] == 'blur')
        bare = _check_slot_case(imgs, rows, [[len(k)] + k for k in keeps], 10, 13, 3, None, style)
        if m['method'] == 'fill':
            assert any(not np.array_equal(a, b) for a, b in zip(got, bare)) and any(not np.array_equal(a, im) for a, im in zip(bare, imgs))


# ------------------------------------------------------------------------------------------------------------ the Python layer
def test_redact_batch_on_host_results():
    sizes = [(64, 64), (37, 211), (130, 67), (20, 30)]
    imgs, rows, keeps, trs = _random_batch(91, sizes)
    rows[3], keeps[3] = np.zeros((0, 13)), []                                            # an image without rows: its tracks remain
    frames = [im.copy() for im in imgs]
    frames[1] = torch.from_numpy(frames[1]).cuda()                                       # one CUDA frame among numpy ones
    frames[2] = torch.from_numpy(frames[2])                                              # ... and a CPU tensor
    d_in = [r.copy() for r in rows]
    d_in[0] = torch.from_numpy(d_in[0]).cuda()                                           # a device result among host ones
    live = [t[t['id'] >= 0] for t in trs]                                                # as Tracker.live() returns them
    live[0] = live[0][:0]                                                                # a stream without tracks
    for kw in (dict(method='blur', radius=5, grow=3, grow_pct=20), dict(method='pixelate', cell=5, shape='box', coast=2), dict(method='fill')):
        out = redact.redact_batch(frames, d_in, keeps, tracks=live, style=redact.Redaction(**kw))
        sd = dict(V.STYLE, coast=1 << 30)                                                # coast None: every coasting track
        sd.update(kw)
        assert isinstance(out[0], np.ndarray) and out[1].is_cuda and torch.is_tensor(out[2]) and not out[2].is_cuda
        for b in range(4):
            got = out[b] if isinstance(out[b], np.ndarray) else out[b].cpu().numpy()
            assert got.dtype == np.uint8 and np.array_equal(got, V.redact(imgs[b], rows[b], keeps[b], live[b], sd)), (b, kw)
            src = frames[b] if isinstance(frames[b], np.ndarray) else frames[b].cpu().numpy()
            assert np.array_equal(src, imgs[b])                                          # the inputs are unchanged
    plain = redact.redact_batch(frames, rows, keeps)                                     # defaults, no tracks
    for b in range(4):
        got = plain[b] if isinstance(plain[b], np.ndarray) else plain[b].cpu().numpy()
        assert np.array_equal(got, V.redact(imgs[b], rows[b], keeps[b])), b
    assert np.array_equal(plain[3], imgs[3])
    batch = torch.from_numpy(np.stack([imgs[0], imgs[0][::-1].copy()])).cuda()           # a batch tensor, five-column rows
    five = redact.redact_batch(batch, [rows[0][:, :5]] * 2, [keeps[0]] * 2)
    assert all(t.is_cuda for t in five)
    assert np.array_equal(five[1].cpu().numpy(), V.redact(imgs[0][::-1], rows[0][:, :5], keeps[0]))


def _net(kind, dtype):
    net = getattr(D, kind)(synth.vgg19_standin(seed=0))
    synth.fill_params_(net, 11)
    # every pixel's box is 17 x 13 pixels around it, as tests/test_hip_viz.py and tests/test_hip_track.py set it
    with torch.no_grad():
        net.conv5_2_loc.weight.zero_()
        net.conv5_2_loc.bias.copy_(torch.tensor([2.0, 1.5, -2.0, -1.5]))
    net = net.cuda().eval()
    net.compute_dtype = dtype
    return net


@pytest.mark.parametrize('dtype', ['f32', 'f16'])
@pytest.mark.parametrize('kind', ['DenseBox', 'DenseBoxLMLOC'])
def test_net_redact_batch_is_the_other_calls_plus_the_restatement(kind, dtype, monkeypatch):
    monkeypatch.delenv('DBX_GRAPH', raising=False)
    net = _net(kind, dtype)
    rs = np.random.RandomState(29)
    X = torch.from_numpy(rs.randint(0, 256, size=(3, 64, 64, 3)).astype(np.uint8)).cuda()
    blank = torch.zeros_like(X)
    seq = [X, blank, X]                                                                  # the middle call's frames are blank: tracks coast
    kw = dict(K=10, max_batch=2)
    tops = [net.detect_batch(x, **kw) for x in seq]
    ref_tr = T.Tracker(5, max_tracks=64, max_age=2)
    tracked = [net.track_batch(x, tracker=ref_tr, stream0=1, **kw) for x in seq]
    assert sum(len(k) for _, k in tops[0]) > 0
    st = redact.Redaction(method='pixelate', cell=5)
    sd = dict(V.STYLE, cell=5, coast=2)                                                  # coast None: the tracker's max_age

    def run(env):
        if env is not None:
            monkeypatch.setenv('DBX_GRAPH', env)
        tr = T.Tracker(5, max_tracks=64, max_age=2)
        frames, coasted = [], 0
        for call, x in enumerate(seq):
            got = net.redact_batch(x, tracker=tr, stream0=1, style=st, **kw)
            assert tr.headers()[:, 0].tolist() == [0, call + 1, call + 1, call + 1, 0]   # the capture's warm-up runs did not count
            live = tr.live()
            imgs = x.cpu().numpy()
            for b, (d, keep, tid, red) in enumerate(got):
                assert np.array_equal(_bits(d), _bits(tops[call][b][0])) and keep == tops[call][b][1]
                assert tid.dtype == np.int32 and tid.tolist() == tracked[call][b][2].tolist()
                assert red.is_cuda and red.dtype == torch.uint8
                want = V.redact(imgs[b], d, keep, live[1 + b], sd)
                assert np.array_equal(red.cpu().numpy(), want), (env, call, b, kind, dtype)
                coasting = live[1 + b][live[1 + b]['age'] >= 1]
                if coasting.size and not np.array_equal(want, V.redact(imgs[b], d, keep, None, sd)):
                    coasted += 1
            frames.append([g[3].cpu().numpy() for g in got])
        assert coasted > 0, 'no frame was redacted at a coasting track'
        h, t = tr._host_state()
        rh, rt = ref_tr._host_state()
        assert h.tolist() == rh.tolist() and np.array_equal(_bits(t), _bits(rt))
        monkeypatch.delenv('DBX_GRAPH', raising=False)
        return frames

    replayed = run(None)
    assert sum(k[0] == 'redact' for k in net._detect_graphs) >= 2
    eager = run('0')
    assert all(np.array_equal(a, b) for fa, fb in zip(replayed, eager) for a, b in zip(fa, fb))      # graph replay x 3 == eager x 3
    # without a tracker; numpy frames in, numpy frames out; the other entries of the cache are not disturbed
    imgs = X.cpu().numpy()
    for env in (None, '0'):
        if env is not None:
            monkeypatch.setenv('DBX_GRAPH', env)
        got = net.redact_batch(X, style=st, **kw)
        host = net.redact_batch([im for im in imgs], style=st, **kw)
        for b, (d, keep, tid, red) in enumerate(got):
            assert tid is None and keep == tops[0][b][1] and np.array_equal(_bits(d), _bits(tops[0][b][0]))
            assert np.array_equal(red.cpu().numpy(), V.redact(imgs[b], d, keep, None, sd))
            assert isinstance(host[b][3], np.ndarray) and np.array_equal(host[b][3], red.cpu().numpy())
    monkeypatch.delenv('DBX_GRAPH')
    assert all(np.array_equal(_bits(a), _bits(b)) and ka == kb for (a, ka), (b, kb) in zip(net.detect_batch(X, **kw), tops[0]))
