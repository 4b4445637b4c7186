"""Annotated frames on the GPU: dbx_draw_overlay_batch == the NumPy restatement (tests/viz_ref.py) bit for bit -- crafted rows on frames
from 1 x 1 to several tiles with 1, 3 and 4 channels, out of place and in place, from even and odd addresses, nothing written outside
the frames; the LDS bound of 1024 rows; the packed layout behind the threshold decode and corrupted prefixes; frame records that must be
skipped; a seeded mixed-size batch; viz.draw_batch on host results; net.annotate_batch == detect_batch / detect_plate_crops / track_batch
+ the restatement, through the hipGraph and without it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import densebox_amd as D
from densebox_amd import _lib, decode as DC, synth, track as T, viz
from densebox_amd._lib import check, ptr, stream_ptr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import viz_ref as V  # noqa: E402
import thresh_ref  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64                     # sentinel bytes in front of and behind every output frame
FILL_B = 0xEE
NAN, INF = float('nan'), float('inf')


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _style_record(st):
    s = dict(V.STYLE)
    s.update(st or {})
    return viz.Style(**s)


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

    def read(self, name='dst'):
        h = self.whole.cpu().numpy()
        assert (h[:self.off] == FILL_B).all() and (h[self.off + self.n:] == FILL_B).all(), 'bytes outside %s were written' % name
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


def _slot_inputs(rows, keeps, slots, dc, ids=None, crops=None, ok=None):
    """device arrays in dbx_detect_batch's slot layout; keeps[b] is the raw keep record [count, entries...] (any count)"""
    B = len(rows)
    d = np.zeros((B, slots, dc), np.float64)
    k = np.zeros((B, slots + 1), np.int32)
    t = np.full((B, slots), -1, np.int32)
    o = np.zeros((B, slots), np.int32)
    for b in range(B):
        d[b, :rows[b].shape[0]] = rows[b]
        k[b, :len(keeps[b])] = keeps[b]
        if ids is not None:
            t[b, :len(ids[b])] = ids[b]
        if ok is not None:
            o[b, :len(ok[b])] = ok[b]
    cr = None
    if crops is not None:
        cr = np.zeros((B, slots) + crops[0].shape[1:], np.uint8)
        for b in range(B):
            cr[b, :crops[b].shape[0]] = crops[b]
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return up(d.reshape(B * slots, dc)), up(k), up(t) if ids is not None else None, up(cr), up(o) if ok is not None else None


def _launch(frames, c, dets, dc, det_rows, keep, prefix, slots, ids, crops, ok, style, records=None, max_hw=None):
    table = _table(frames, records)
    mh, mw = max_hw or (max(f.img.shape[0] for f in frames), max(f.img.shape[1] for f in frames))
    oh, ow = (int(crops.shape[2]), int(crops.shape[3])) if crops is not None else (0, 0)
    rec = _style_record(style).record()
    check(_lib.lib().dbx_draw_overlay_batch(ptr(table), len(frames), c, mh, mw, ptr(dets), dc, det_rows, ptr(keep), ptr(prefix), slots,
                                            ptr(ids), ptr(crops), ptr(ok), ow, oh, C.byref(rec), stream_ptr()))
    torch.cuda.synchronize()


def _effective(raw, n, slots):
    """the list the kernel walks for a raw keep record: the count clamped to 0..min(n, slots)"""
    k = min(max(int(raw[0]), 0), min(n, slots))
    return [int(v) for v in raw[1:1 + k]]


def _check_slot_case(imgs, rows, keeps, slots, dc, c, ids, crops, ok, style, in_place, odd):
    """one launch in slot layout against the restatement, frame by frame; returns the drawn frames"""
    frames = [_Frame(im, in_place, odd) for im in imgs]
    d, k, t, cr, o = _slot_inputs(rows, keeps, slots, dc, ids, crops, ok)
    _launch(frames, c, d, dc, len(imgs) * slots, k, None, slots, t, cr, o, style)
    out = []
    for b, f in enumerate(frames):
        padded = np.zeros((slots, dc))
        padded[:rows[b].shape[0]] = rows[b]
        kl = _effective(list(keeps[b]) + [0] * (slots + 1 - len(keeps[b])), slots, slots)
        part = lambda v: None if v is None else np.asarray(v[b])[:len(kl)]  # noqa: E731  (by list position: at least len(kl) entries)
        want = V.draw(f.img, padded, kl, part(ids), part(crops), part(ok), style)
        got = f.read()
        assert np.array_equal(got, want), (b, f.img.shape, style, in_place, odd, np.argwhere((got != want).any(axis=2))[:5])
        out.append(got)
    return out


# ------------------------------------------------------------------------------------------------------------ crafted rows
def _crafted(h, w):
    """13-column rows that exercise every clipping and rejection rule on an h x w frame, and the landmarks of each"""
    r = []
    r.append([0.2 * w, 0.3 * h, 0.7 * w, 0.8 * h])                       # inside
    r.append([w + 50.0, h + 50.0, w + 80.0, h + 70.0])                   # wholly outside, beyond the far corner
    r.append([-100.0, -100.0, -60.0, -70.0])                             # ... and before the origin
    r.append([-5.3, h / 2.0, 4.2, h / 2.0 + 6])                          # straddling the left edge
    r.append([w - 4.0, 2.0, w + 6.0, 8.0])                               # ... the right edge
    r.append([w / 3.0, -6.0, w / 3.0 + 8, 3.0])                          # ... the top edge: its label is clipped by it
    r.append([2.0, h - 3.0, 9.0, h + 5.0])                               # ... the bottom edge
    r.append([w / 2.0, h / 2.0, w / 2.0, h / 2.0])                       # zero size
    r.append([0.8 * w, 0.6 * h, 0.4 * w, 0.2 * h])                       # inverted: x2 < x1, y2 < y1
    r.append([NAN, 1.0, 5.0, 6.0])                                       # not usable: nothing is painted
    r.append([1.0, 2.0, 5.0, INF])
    r.append([1.0, 2.0, 1e300, 6.0])
    r.append([0.3 * w, 0.25 * h, 0.6 * w, 0.7 * h])                      # a NaN landmark in a row that is drawn
    r.append([0.45 * w - 2, 0.45 * h - 2, 0.45 * w + 9, 0.45 * h + 7])   # three rows that overlap each other
    r.append([0.45 * w, 0.45 * h, 0.45 * w + 11, 0.45 * h + 9])
    r.append([0.45 * w + 2, 0.45 * h + 2, 0.45 * w + 13, 0.45 * h + 11])
    rows = np.zeros((len(r), 13))
    rows[:, :4] = r
    rows[:, 4] = [0.987, 0.5, -0.25, 7.0625, 999.9996, NAN, -0.0, 0.0005, 123.4565, 0.1, 0.2, 0.3, 1000.0, 0.75, 0.5, 0.25]
    rs = np.random.RandomState(h * 1000 + w)
    for q in range(4):                                                   # landmarks around the box's corners (finite boxes only)
        cx = np.where(np.isfinite(rows[:, 0]) & (np.abs(rows[:, 2]) < 1e9), rows[:, 0 if q in (0, 3) else 2], 3.0)
        cy = np.where(np.isfinite(rows[:, 3]), rows[:, 1 if q < 2 else 3], 3.0)
        rows[:, 5 + 2 * q] = cx + rs.uniform(-3, 3, len(r))
        rows[:, 6 + 2 * q] = cy + rs.uniform(-3, 3, len(r))
    rows[12, 7], rows[12, 12], rows[0, 9], rows[3, 5] = NAN, INF, 1e300, -2.0 ** 31
    return rows


STYLES = [dict(thickness=1, radius=-1, font_scale=0, inset_scale=1),
          dict(thickness=2, radius=0, font_scale=1, inset_scale=2),
          dict(thickness=5, radius=5, font_scale=3, inset_scale=1, box_color=(10, 20, 30, 40), text_color=(50, 60, 70, 80),
               mark_color=(90, 100, 110, 120))]


@pytest.mark.parametrize('c', [1, 3, 4])
@pytest.mark.parametrize('h,w', [(1, 1), (5, 7), (17, 33), (48, 64), (67, 130)])
def test_kernel_equals_restatement_on_crafted_rows(h, w, c):
    rs = np.random.RandomState(h * 100 + w + c)
    img = rs.randint(0, 256, size=(h, w, c)).astype(np.uint8)
    rows = _crafted(h, w)
    n = rows.shape[0]
    order = [int(v) for v in rs.permutation(n)]
    ids = [[(-1 if j % 3 == 0 else 7 * j + (2147483647 - 200 if j == 4 else 0)) for j in range(n)]]
    crops = [rs.randint(0, 256, size=(n, 3, 6, c)).astype(np.uint8)]
    ok = [[int(j % 4 != 1) for j in range(n)]]
    for si, style in enumerate(STYLES):
        for in_place in (False, True):
            for odd in (False, True):
                with_ids, with_crops = si != 0, si != 0 or odd
                got = _check_slot_case([img], [rows], [[n] + order], n, 13, c, ids if with_ids else None, crops if with_crops else None,
                                       ok if with_crops else None, style, in_place, odd)
        count = np.zeros((h, w), np.int64)
        V.draw(img, rows, order, ids[0] if with_ids else None, crops[0] if with_crops else None, ok[0] if with_crops else None, style, count)
        if h >= 17:                                                       # (smaller frames do not hold the three overlapping rows)
            assert (count >= 2).any(), 'no pixel is covered by two rows'
            assert not np.array_equal(got[0], img)
    # five columns (no discs), k = 0, a count above slots, keep entries out of range
    _check_slot_case([img], [rows[:, :5]], [[n] + order], n, 5, c, None, None, None, STYLES[2], False, False)
    got = _check_slot_case([img], [rows], [[0] + order], n, 13, c, None, None, None, STYLES[1], False, True)
    assert np.array_equal(got[0], img)
    _check_slot_case([img], [rows], [[n + 5] + order], n, 13, c, ids, crops, ok, STYLES[1], False, False)
    _check_slot_case([img], [rows], [[-3] + order], n, 13, c, ids, crops, ok, STYLES[1], True, False)
    _check_slot_case([img], [rows], [[6, 13, -1, 14, n, 1 << 30, 15]], n, 13, c, ids, crops, ok, STYLES[1], False, False)


def test_1024_rows_on_one_frame():
    """the LDS bound: slots = 1024 kept 3 x 3 boxes whose labels pile up on a few tiles"""
    rs = np.random.RandomState(1024)
    img = rs.randint(0, 256, size=(256, 256, 3)).astype(np.uint8)
    rows = np.zeros((1024, 5))
    rows[:, 0], rows[:, 1] = rs.randint(0, 254, 1024), rs.randint(0, 62, 1024)
    rows[:, 2], rows[:, 3], rows[:, 4] = rows[:, 0] + 2, rows[:, 1] + 2, rs.rand(1024)
    order = [int(v) for v in rs.permutation(1024)]
    # rows whose label background (scale 1: x X1 .. X1 + 33, y Y1 - 13 .. Y1) meets the tile x 0..127, y 16..31
    meet = ((rows[:, 0] <= 127) & (rows[:, 1] - 13 <= 31) & (rows[:, 1] >= 16)).sum()
    assert meet >= 200, meet
    style = dict(font_scale=1, thickness=1)
    got = _check_slot_case([img], [rows], [[1024] + order], 1024, 5, 3, None, None, None, style, False, False)
    assert np.array_equal(got[0][80:], img[80:]) and not np.array_equal(got[0][:80], img[:80])


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
    ids = rs.randint(-1, 99, size=(B, cap)).astype(np.int32)
    d_ids = torch.from_numpy(ids).cuda()
    style = dict(font_scale=1)
    none = (np.zeros((0, 13)), [])
    d_all, k_all = dets.cpu().numpy(), keep.cpu().numpy()
    l2 = k_all[10 + 2:10 + 2 + 47 + 1]
    odd = (d_all[10:57].copy(), [int(v) for v in l2[1:1 + min(max(int(l2[0]), 0), 47)]])
    cases = [(cnt[2 * B:], host),
             (torch.tensor([0, 20, 10, 57], dtype=torch.int32, device='cuda'), [host[0], none, odd]),         # decreasing: frame 1 is empty
             (torch.tensor([0, 20, 20, 1 << 20], dtype=torch.int32, device='cuda'), [host[0], none, none]),   # beyond det_rows
             (torch.tensor([-5, 20, 20, 57], dtype=torch.int32, device='cuda'), [none, none, host[2]])]       # negative
    for prefix, want_frames in cases:
        frames = [_Frame(im) for im in imgs]
        _launch(frames, 3, dets, 13, int(dets.numel()) // 13, keep, prefix, cap, d_ids, None, None, style)
        for b, (f, (rows, kl)) in enumerate(zip(frames, want_frames)):
            got = f.read()
            assert np.array_equal(got, V.draw(f.img, rows, kl, ids[b], None, None, style)), b
            if not kl:
                assert np.array_equal(got, f.img)                                                              # copied undrawn
    assert not np.array_equal(got, imgs[2])


def test_bad_frame_records_are_skipped():
    rs = np.random.RandomState(8)
    imgs = [rs.randint(0, 256, size=(30, 40, 3)).astype(np.uint8) for _ in range(6)]
    rows = [np.array([[5.0, 12.0, 25.0, 22.0, 0.5]])] * 6
    frames = [_Frame(im) for im in imgs]
    d, k, _, _, _ = _slot_inputs(rows, [[1, 0]] * 6, 2, 5)
    records = {1: dict(src=None), 2: dict(dst=None), 3: dict(h=31), 4: dict(w=41), 5: dict(h=0)}
    before = [f.whole.clone() for f in frames]
    _launch(frames, 3, d, 5, 12, k, None, 2, None, None, None, None, records=records, max_hw=(30, 40))
    assert np.array_equal(frames[0].read(), V.draw(imgs[0], rows[0], [0]))
    for f, b in zip(frames[1:], before[1:]):
        assert torch.equal(f.whole, b)                                                                         # sentinel-filled, untouched


def _random_batch(seed, sizes, K=10, c=3):
    rs = np.random.RandomState(seed)
    imgs, rows, keeps, ids, crops, ok = [], [], [], [], [], []
    for h, w in sizes:
        imgs.append(rs.randint(0, 256, size=(h, w, c)).astype(np.uint8))
        r = np.zeros((K, 13))
        r[:, 0], r[:, 1] = rs.uniform(-10, w, K), rs.uniform(-10, h, K)
        r[:, 2], r[:, 3] = r[:, 0] + rs.uniform(-5, 0.6 * w, K), r[:, 1] + rs.uniform(-5, 0.5 * h, K)
        r[:, 4] = rs.uniform(0, 1, K)
        r[:, 5::2], r[:, 6::2] = rs.uniform(-8, w + 8, (K, 4)), rs.uniform(-8, h + 8, (K, 4))
        k = rs.randint(0, K + 1)
        rows.append(r)
        keeps.append([int(v) for v in rs.permutation(K)[:k]])
        ids.append(rs.randint(-1, 500, k).astype(np.int32))
        crops.append(rs.randint(0, 256, size=(k, 8, 31, c)).astype(np.uint8))
        ok.append(rs.randint(0, 3, k) != 0)
    return imgs, rows, keeps, ids, crops, ok


def test_seeded_batch_of_mixed_sizes_with_ids_and_crops():
    sizes = [(64, 64), (37, 211), (130, 67), (1, 300), (200, 3), (96, 129), (16, 128), (17, 257)]
    imgs, rows, keeps, ids, crops, ok = _random_batch(77, sizes)
    for in_place, odd in ((False, False), (True, True)):
        _check_slot_case(imgs, rows, [[len(k)] + k for k in keeps], 10, 13, 3, ids, crops, [o.astype(np.int32) for o in ok], None,
                         in_place, odd)


# ------------------------------------------------------------------------------------------------------------ the Python layer
def test_draw_batch_on_host_results():
    sizes = [(64, 64), (37, 211), (130, 67), (20, 30)]
    imgs, rows, keeps, ids, crops, ok = _random_batch(91, sizes)
    rows[3], keeps[3], ids[3], crops[3], ok[3] = np.zeros((0, 13)), [], ids[3][:0], crops[3][:0], ok[3][:0]         # an image without rows
    frames = [im.copy() for im in imgs]
    frames[1] = torch.from_numpy(frames[1]).cuda()                                       # one CUDA frame among numpy ones
    frames[2] = torch.from_numpy(frames[2])                                              # ... and a CPU tensor
    d_in = [r.copy() for r in rows]
    d_in[0] = torch.from_numpy(d_in[0]).cuda()                                           # a device result among host ones
    st = viz.Style(thickness=3, font_scale=1, inset_scale=2)
    sd = dict(thickness=3, font_scale=1, inset_scale=2)
    out = viz.draw_batch(frames, d_in, keeps, track_ids=ids, crops=crops, ok=ok, style=st)
    assert isinstance(out[0], np.ndarray) and out[1].is_cuda and torch.is_tensor(out[2]) and not out[2].is_cuda and isinstance(out[3], np.ndarray)
    for b in range(4):
        got = out[b] if isinstance(out[b], np.ndarray) else out[b].cpu().numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, V.draw(imgs[b], rows[b], keeps[b], ids[b], crops[b], ok[b], sd)), b
        src = frames[b] if isinstance(frames[b], np.ndarray) else frames[b].cpu().numpy()
        assert np.array_equal(src, imgs[b])                                              # the inputs are unchanged
    assert np.array_equal(out[3], imgs[3])
    plain = viz.draw_batch(frames, rows, keeps)                                          # defaults: no ids, no inset
    for b in range(4):
        got = plain[b] if isinstance(plain[b], np.ndarray) else plain[b].cpu().numpy()
        assert np.array_equal(got, V.draw(imgs[b], rows[b], keeps[b])), b
    batch = torch.from_numpy(np.stack([imgs[0], imgs[0][::-1].copy()])).cuda()           # a batch tensor, five-column rows
    five = viz.draw_batch(batch, [rows[0][:, :5]] * 2, [keeps[0]] * 2)
    assert all(t.is_cuda for t in five)
    assert np.array_equal(five[1].cpu().numpy(), V.draw(imgs[0][::-1], rows[0][:, :5], keeps[0]))


def _net(kind, dtype):
    net = getattr(D, kind)(synth.vgg19_standin(seed=0))
    synth.fill_params_(net, 11)
    # The seeded stand-in gives boxes of any shape, most of them with x2 < x1, which overlap nothing.  The last layer of the box head is
    # set so that every pixel's box is 17 x 13 pixels around it, as tests/test_hip_track.py does.
    with torch.no_grad():
        net.conv5_2_loc.weight.zero_()
        net.conv5_2_loc.bias.copy_(torch.tensor([2.0, 1.5, -2.0, -1.5]))
    net = net.cuda().eval()
    net.compute_dtype = dtype
    return net


@pytest.mark.parametrize('dtype', ['f32', 'f16'])
@pytest.mark.parametrize('kind', ['DenseBox', 'DenseBoxLMLOC'])
def test_annotate_batch_is_the_other_calls_plus_the_restatement(kind, dtype, monkeypatch):
    monkeypatch.delenv('DBX_GRAPH', raising=False)
    net = _net(kind, dtype)
    rs = np.random.RandomState(29)
    X = torch.from_numpy(rs.randint(0, 256, size=(3, 64, 64, 3)).astype(np.uint8)).cuda()
    imgs = X.cpu().numpy()
    kw = dict(K=10, max_batch=2)
    top = net.detect_batch(X, **kw)
    inset = None
    crops = oks = [None] * 3
    if kind == 'DenseBox':
        with pytest.raises(RuntimeError, match='landmarks'):
            net.annotate_batch(X, inset=(94, 24), **kw)
    else:
        inset = (94, 24)
        pc = net.detect_plate_crops(X, size=inset, **kw)
        crops, oks = [p[2].cpu().numpy() for p in pc], [p[3] for p in pc]
    ref_tr = T.Tracker(5, max_tracks=64, max_age=1)
    tracked = [net.track_batch(X, tracker=ref_tr, stream0=1, **kw) for _ in range(2)]
    assert sum(len(k) for _, k in top) > 0                                               # at least one kept row overall

    def same(got, ids):
        for b, (d, keep, tid, ann) in enumerate(got):
            assert np.array_equal(_bits(d), _bits(top[b][0])) and keep == top[b][1]
            if ids is None:
                assert tid is None
            else:
                assert tid.dtype == np.int32 and tid.tolist() == ids[b][2].tolist()
            assert ann.is_cuda and ann.dtype == torch.uint8
            want = V.draw(imgs[b], d, keep, None if ids is None else ids[b][2], crops[b], oks[b])
            assert np.array_equal(ann.cpu().numpy(), want), (b, kind, dtype)
            assert not np.array_equal(want, imgs[b]) or not keep

    for env in (None, '0'):                                                              # the graph, then the same launches without it
        if env is not None:
            monkeypatch.setenv('DBX_GRAPH', env)
        got = net.annotate_batch(X, inset=inset, **kw)
        same(got, None)
        tr = T.Tracker(5, max_tracks=64, max_age=1)
        first = net.annotate_batch(X, tracker=tr, stream0=1, inset=inset, **kw)
        assert tr.headers()[:, 0].tolist() == [0, 1, 1, 1, 0]                            # the capture's warm-up runs did not count
        same(first, tracked[0])
        again = net.annotate_batch(X, tracker=tr, stream0=1, inset=inset, **kw)
        same(again, tracked[1])
        for (_, keep, tid, _), (_, _, tid0, _) in zip(again, first):                     # every kept row continues its own track
            assert tid.tolist() == tid0.tolist() and (tid >= 0).all()
        assert np.array_equal(got[0][3].cpu().numpy(), V.draw(imgs[0], top[0][0], top[0][1], None, crops[0], oks[0]))     # results own their memory
        h, t = tr._host_state()
        rh, rt = ref_tr._host_state()
        assert h.tolist() == rh.tolist() and np.array_equal(_bits(t), _bits(rt))
        if env is None:
            assert sum(k[0] == 'annotate' for k in net._detect_graphs) >= 2
        host = net.annotate_batch([im for im in imgs], inset=inset, **kw)                # numpy frames in, numpy frames out
        for b, (d, keep, tid, ann) in enumerate(host):
            assert isinstance(ann, np.ndarray) and np.array_equal(ann, got[b][3].cpu().numpy()) and keep == top[b][1]
    monkeypatch.delenv('DBX_GRAPH')
    # the other entries of the cache are not disturbed
    assert all(np.array_equal(_bits(a), _bits(b)) and ka == kb for (a, ka), (b, kb) in zip(net.detect_batch(X, **kw), top))
