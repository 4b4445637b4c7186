"""NV12 frames on the GPU: dbx_nv12_to_rgb_batch and dbx_rgb_to_nv12_batch == the NumPy restatement (tests/nv12_ref.py) bit for bit -- frames
from one block to several tiles, pitches w, w + 1 and w + 13, planes at even and odd addresses, sentinels around every output plane and
in the pitch gap of every row; one 4096 x 4096 frame holding every (Y, U, V); a mixed-size batch with skipped records;
dbx_resize_cubic_batch_nv12 == dbx_resize_cubic_batch_u8 on the converted frame; the Python layer; the net-level calls ==
detect_batch / detect_batch_resized / redact_batch on the restated RGB; the Python-level refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import densebox_amd as D
from densebox_amd import _lib, color, redact, resize, synth, track as T
from densebox_amd._lib import check, stream_ptr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cubic_ref  # noqa: E402
import nv12_ref as N  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64                     # sentinel bytes in front of and behind every plane
FILL_B = 0xEE
SIZES = [(2, 2), (2, 4), (4, 2), (16, 64), (18, 66), (34, 130)]
RANGE = {'limited': 0, 'full': 1}
ORDER = {'rgb': 0, 'bgr': 1}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _record(std=601, rng='limited', order='rgb'):
    return _lib.Nv12Params(std, RANGE[rng], ORDER[order], 0)


class _Plane:
    """`rows` rows of `row` bytes at `pitch` on the device between sentinels, its pitch gaps sentinels as well; odd: it starts on an odd
    address.  data: the rows' bytes (an input plane), or None (an output plane: all sentinels)."""

    def __init__(self, rows, row, pitch, odd, data=None):
        self.rows, self.row, self.pitch, self.off, self.n = rows, row, pitch, GUARD + (1 if odd else 0), rows * pitch
        host = np.full(self.n + 2 * GUARD + 1, FILL_B, np.uint8)
        if data is not None:
            host[self.off:self.off + self.n].reshape(rows, pitch)[:, :row] = np.asarray(data).reshape(rows, row)
        self.before = host
        self.buf = torch.from_numpy(host.copy()).cuda()
        self.ptr = self.buf.data_ptr() + self.off
        assert self.ptr % 2 == (1 if odd else 0)

    def read(self):
        """the rows' bytes; everything else -- the guards and every pitch gap -- must be as it was"""
        h = self.buf.cpu().numpy()
        got, was = h.copy(), self.before.copy()
        body = got[self.off:self.off + self.n].reshape(self.rows, self.pitch)
        data = body[:, :self.row].copy()
        body[:, :self.row] = 0
        was[self.off:self.off + self.n].reshape(self.rows, self.pitch)[:, :self.row] = 0
        assert np.array_equal(got, was), 'bytes outside the rows were written (guards or a pitch gap)'
        return data

    def untouched(self):
        return np.array_equal(self.buf.cpu().numpy(), self.before)


class _Frame:
    """one h x w frame as three device planes; nv12 / rgb: the input side's data (the other side is the sentinel-filled output)"""

    def __init__(self, h, w, extra, odd, nv12=None, rgb=None):
        self.h, self.w = h, w
        self.y = _Plane(h, w, w + extra, odd, None if nv12 is None else nv12[:h])
        self.uv = _Plane(h // 2, w, w + extra, odd, None if nv12 is None else nv12[h:])
        self.rgb = _Plane(h, 3 * w, 3 * w + extra, odd, None if rgb is None else rgb.reshape(h, 3 * w))

    def record(self, **over):
        r = _lib.Nv12Frame(self.y.ptr, self.uv.ptr, self.rgb.ptr, self.h, self.w, self.y.pitch, self.uv.pitch, self.rgb.pitch, 0)
        for k, v in over.items():
            setattr(r, k, v)
        return r

    def image(self):
        return self.rgb.read().reshape(self.h, self.w, 3)

    def nv12(self):
        return np.concatenate([self.y.read(), self.uv.read()])


def _launch(frames, to_rgb, par, records=None, max_hw=None):
    rec = (_lib.Nv12Frame * len(frames))(*[f.record(**(records or {}).get(i, {})) for i, f in enumerate(frames)])
    table = torch.frombuffer(rec, dtype=torch.uint8).cuda()
    mh, mw = max_hw or (max(f.h for f in frames), max(f.w for f in frames))
    fn = _lib.lib().dbx_nv12_to_rgb_batch if to_rgb else _lib.lib().dbx_rgb_to_nv12_batch
    check(fn(C.c_void_p(table.data_ptr()), len(frames), mh, mw, C.byref(par), stream_ptr()))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ the conversions
@pytest.mark.parametrize('h,w', SIZES)
def test_both_launches_equal_the_restatement(h, w):
    rs = np.random.RandomState(h * 1000 + w)
    for extra in (0, 1, 13):
        for odd in (False, True):
            for std, rng in N.VARIANTS:
                for order in ('rgb', 'bgr'):
                    par = _record(std, rng, order)
                    nv = rs.randint(0, 256, size=(h * 3 // 2, w)).astype(np.uint8)
                    f = _Frame(h, w, extra, odd, nv12=nv)
                    _launch([f], True, par)
                    assert np.array_equal(f.image(), N.nv12_to_rgb(nv, None, std, rng, order)), (extra, odd, std, rng, order)
                    assert np.array_equal(f.nv12(), nv)                                    # the source is read only
                    img = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
                    g = _Frame(h, w, extra, odd, rgb=img)
                    _launch([g], False, par)
                    assert np.array_equal(g.nv12(), N.rgb_to_nv12(img, std, rng, order)), (extra, odd, std, rng, order)
                    assert np.array_equal(g.image(), img)


def test_every_yuv_triple_on_one_frame():
    """4096 x 4096, 601 limited: block b = 2048 * by + bx holds the chroma pair b >> 6 and the four Y values 4 * (b & 63) + 0..3"""
    side = 4096
    b = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
    nv = np.empty((side * 3 // 2, side), np.uint8)
    yb = (4 * (b & 63)).astype(np.uint8)
    nv[0:side:2, 0::2], nv[0:side:2, 1::2], nv[1:side:2, 0::2], nv[1:side:2, 1::2] = yb, yb + 1, yb + 2, yb + 3
    nv[side:, 0::2], nv[side:, 1::2] = ((b >> 6) >> 8).astype(np.uint8), ((b >> 6) & 255).astype(np.uint8)
    seen = np.zeros(1 << 24, bool)
    seen[(nv[:side].astype(np.int64) << 16) | (np.repeat(np.repeat(b >> 6, 2, axis=0), 2, axis=1))] = True
    assert seen.all(), 'the frame does not hold every (Y, U, V)'
    dev = torch.from_numpy(nv).cuda()
    out = torch.full((side * side * 3 + 2 * GUARD,), FILL_B, dtype=torch.uint8, device='cuda')
    rec = _lib.Nv12Frame(dev.data_ptr(), dev.data_ptr() + side * side, out.data_ptr() + GUARD, side, side, side, side, 3 * side, 0)
    table = torch.frombuffer(rec, dtype=torch.uint8).cuda()
    check(_lib.lib().dbx_nv12_to_rgb_batch(C.c_void_p(table.data_ptr()), 1, side, side, C.byref(_record()), stream_ptr()))
    got = out.cpu().numpy()
    assert (got[:GUARD] == FILL_B).all() and (got[-GUARD:] == FILL_B).all()
    got = got[GUARD:-GUARD].reshape(side, side, 3)
    for y0 in range(0, side, 512):                                                    # in strips: the restatement works in int64
        strip = np.concatenate([nv[y0:y0 + 512], nv[side + y0 // 2:side + y0 // 2 + 256]])
        assert np.array_equal(got[y0:y0 + 512], N.nv12_to_rgb(strip)), y0


def test_mixed_size_batch_with_skipped_records():
    rs = np.random.RandomState(5)
    sizes = [(34, 130), (2, 2), (16, 64), (18, 66), (4, 2), (6, 8), (8, 6), (10, 12)]
    nvs = [rs.randint(0, 256, size=(h * 3 // 2, w)).astype(np.uint8) for h, w in sizes]
    imgs = [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in sizes]
    records = {5: dict(y=None), 6: dict(h=7), 7: dict(w=140)}                           # null, odd size, over max_w
    for to_rgb in (True, False):
        for skip_field in ('y', 'uv', 'rgb'):
            records[5] = {skip_field: None}
            frames = [_Frame(h, w, 3 * i, i % 2 == 1, nv12=nvs[i] if to_rgb else None, rgb=None if to_rgb else imgs[i])
                      for i, (h, w) in enumerate(sizes)]
            _launch(frames, to_rgb, _record(709, 'full', 'bgr'), records, max_hw=(34, 130))
            for i, f in enumerate(frames[:5]):                                             # five frames of five sizes in one launch
                if to_rgb:
                    assert np.array_equal(f.image(), N.nv12_to_rgb(nvs[i], None, 709, 'full', 'bgr')), i
                else:
                    assert np.array_equal(f.nv12(), N.rgb_to_nv12(imgs[i], 709, 'full', 'bgr')), i
            for f in frames[5:]:
                assert f.y.untouched() and f.uv.untouched() and f.rgb.untouched()
    # a pitch below its row, a frame above max_h: skipped as well
    frames = [_Frame(16, 64, 0, False, nv12=nvs[2]) for _ in range(4)]
    _launch(frames, True, _record(), {0: dict(pitch_y=62), 1: dict(pitch_uv=63), 2: dict(pitch_rgb=191)}, max_hw=(16, 64))
    assert all(f.rgb.untouched() for f in frames[:3])
    assert np.array_equal(frames[3].image(), N.nv12_to_rgb(nvs[2]))
    frames = [_Frame(16, 64, 0, False, nv12=nvs[2])]
    _launch(frames, True, _record(), max_hw=(14, 64))
    assert frames[0].rgb.untouched()


# ------------------------------------------------------------------------------------------------------------ the fused resize
def _fused_against_two_launches(nv, w, jobs, par_kw, extra=0, odd=False):
    """jobs = [(cx0, cy0, cw, ch, (l, t, r, b), dh, dw)] on one frame: the fused launch against dbx_resize_cubic_batch_u8 on the restated
    RGB, job blocks at odd offsets between sentinels in both arenas; returns the blocks"""
    h = nv.shape[0] // 3 * 2
    y = _Plane(h, w, w + extra, odd, nv[:h, :w])
    uv = _Plane(h // 2, w, w + extra, odd, nv[h:, :w])
    rgb = N.nv12_to_rgb(nv, w, **par_kw)
    src = torch.from_numpy(rgb).cuda()
    offs, at = [], 1
    for (_, _, _, _, _, dh, dw) in jobs:
        offs.append(at)
        at += dh * dw * 3 + 7                                                            # odd offsets, 7 sentinels between blocks
    fused = torch.full((at + GUARD,), FILL_B, dtype=torch.uint8, device='cuda')
    plain = torch.full((at + GUARD,), FILL_B, dtype=torch.uint8, device='cuda')
    jn = (_lib.ResizeJobNv12 * len(jobs))()
    ju = (_lib.ResizeJob * len(jobs))()
    for a, b, (cx0, cy0, cw, ch, (pl, pt, pr, pb), dh, dw), off in zip(jn, ju, jobs, offs):
        a.y, a.uv, a.pitch_y, a.pitch_uv, a.sh, a.sw = y.ptr, uv.ptr, y.pitch, uv.pitch, h, w
        b.src, b.sh, b.sw = src.data_ptr(), h, w
        for r in (a, b):
            r.cx0, r.cy0, r.cw, r.ch, r.pad_l, r.pad_t, r.pad_r, r.pad_b, r.pad_value = cx0, cy0, cw, ch, pl, pt, pr, pb, 128
            r.dh, r.dw, r.dst_off = dh, dw, off
    L = _lib.lib()
    par = _record(par_kw.get('standard', 601), par_kw.get('rng', 'limited'), par_kw.get('order', 'rgb'))
    ws = torch.empty(L.dbx_resize_batch_nv12_workspace_bytes(len(jobs)), dtype=torch.uint8, device='cuda')
    check(L.dbx_resize_cubic_batch_nv12(jn, len(jobs), C.byref(par), C.c_void_p(fused.data_ptr()), C.c_void_p(ws.data_ptr()), stream_ptr()))
    ws2 = torch.empty(L.dbx_resize_batch_workspace_bytes(len(jobs)), dtype=torch.uint8, device='cuda')
    check(L.dbx_resize_cubic_batch_u8(ju, len(jobs), 3, C.c_void_p(plain.data_ptr()), C.c_void_p(ws2.data_ptr()), stream_ptr()))
    torch.cuda.synchronize()
    f, p = fused.cpu().numpy(), plain.cpu().numpy()
    mask = np.ones(f.size, bool)
    blocks = []
    for (_, _, _, _, _, dh, dw), off in zip(jobs, offs):
        mask[off:off + dh * dw * 3] = False
        blocks.append(f[off:off + dh * dw * 3].reshape(dh, dw, 3))
    assert (f[mask] == FILL_B).all(), 'bytes outside the jobs\' blocks were written'
    assert np.array_equal(f, p), [np.argwhere(f != p)[:5]]
    assert y.untouched() and uv.untouched()
    return blocks


def test_fused_resize_is_the_resize_of_the_converted_frame():
    rs = np.random.RandomState(12)
    nv = rs.randint(0, 256, size=(51, 130)).astype(np.uint8)                             # 34 x 130
    side, px, py = resize.pad_geometry(34, 130)
    whole = (0, 0, 130, 34, (0, 0, 0, 0))
    jobs = [whole + (16, 64), whole + (17, 65), whole + (240, 240),                      # down and up
            (0, 0, 130, 34, (px, py, side - 130 - px, side - 34 - py), 64, 64),          # pad_img's geometry
            (1, 1, 99, 31, (0, 0, 0, 0), 40, 50), (3, 5, 64, 16, (0, 0, 0, 0), 16, 64),  # crops from odd cx0 / cy0
            (7, 3, 33, 9, (2, 1, 0, 3), 30, 71), (129, 33, 1, 1, (0, 0, 0, 0), 3, 3)]
    for extra, odd, par_kw in ((0, False, {}), (13, True, dict(standard=709, rng='full', order='bgr')), (1, False, dict(rng='full'))):
        pitched = np.full((51, 130 + extra), FILL_B, np.uint8)
        pitched[:, :130] = nv
        blocks = _fused_against_two_launches(pitched, 130, jobs, par_kw, extra, odd)
        ref_kw = dict(standard=par_kw.get('standard', 601), rng=par_kw.get('rng', 'limited'), order=par_kw.get('order', 'rgb'))
        assert np.array_equal(blocks[1], N.resize_nv12(nv, (65, 17), **ref_kw))
        assert np.array_equal(blocks[4], N.resize_nv12(nv, (50, 40), window=(1, 1, 100, 32), **ref_kw))
        assert np.array_equal(blocks[3], cubic_ref.pad_resize(N.nv12_to_rgb(nv, **ref_kw), 64))
    tiny = rs.randint(0, 256, size=(3, 2)).astype(np.uint8)                              # 2 x 2 to 7 x 5
    blocks = _fused_against_two_launches(tiny, 2, [(0, 0, 2, 2, (0, 0, 0, 0), 5, 7), (1, 1, 1, 1, (1, 0, 0, 1), 2, 2)], {})
    assert np.array_equal(blocks[0], N.resize_nv12(tiny, (7, 5)))


def test_python_resizes_equal_the_two_step_forms():
    rs = np.random.RandomState(21)
    frames = [rs.randint(0, 256, size=(51, 143)).astype(np.uint8), torch.from_numpy(rs.randint(0, 256, size=(72, 48)).astype(np.uint8)).cuda(),
              torch.from_numpy(rs.randint(0, 256, size=(3, 2)).astype(np.uint8))]
    width = [130, 48, 2]
    p = color.Params(709, 'limited', 'bgr')
    rgb = color.nv12_to_rgb_batch(frames, width, p)
    assert [tuple(t.shape) for t in rgb] == [(34, 130, 3), (48, 48, 3), (2, 2, 3)] and all(t.is_cuda for t in rgb)
    for f, w, t in zip(frames, width, rgb):
        host = f if isinstance(f, np.ndarray) else f.cpu().numpy()
        assert np.array_equal(t.cpu().numpy(), N.nv12_to_rgb(host, w, 709, 'limited', 'bgr'))
    assert torch.equal(resize.pad_resize_batch_nv12(frames, 64, width, p), resize.pad_resize_batch(rgb, 64))
    windows = [[(1, 1, 100, 30), (-31, -7, 130, 34), (3, 5, 67, 21)], [(0, 0, 48, 48), (5, 7, 20, 40)], [(0, 0, 2, 2)]]
    assert torch.equal(resize.crop_resize_batch_nv12(frames, windows, (30, 20), width, p), resize.crop_resize_batch(rgb, windows, (30, 20)))
    # a batch tensor in, one tensor out; the inverse returns the kind it was given
    batch = torch.from_numpy(rs.randint(0, 256, size=(3, 24, 40)).astype(np.uint8))
    out = color.nv12_to_rgb_batch(batch.cuda(), 38)
    assert tuple(out.shape) == (3, 16, 38, 3) and out.is_cuda
    for b in range(3):
        assert np.array_equal(out[b].cpu().numpy(), N.nv12_to_rgb(batch[b].numpy(), 38))
    imgs = [rs.randint(0, 256, size=s).astype(np.uint8) for s in ((34, 130, 3), (2, 2, 3), (16, 64, 3))]
    mixed = [imgs[0], torch.from_numpy(imgs[1]), torch.from_numpy(imgs[2]).cuda()]
    back = color.rgb_to_nv12_batch(mixed, p)
    assert isinstance(back[0], np.ndarray) and torch.is_tensor(back[1]) and not back[1].is_cuda and back[2].is_cuda
    for im, nv in zip(imgs, back):
        got = nv if isinstance(nv, np.ndarray) else nv.cpu().numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, N.rgb_to_nv12(im, 709, 'limited', 'bgr'))
    stack = torch.from_numpy(np.stack([imgs[2], imgs[2][::-1].copy()]))
    one = color.rgb_to_nv12_batch(stack)
    assert tuple(one.shape) == (2, 24, 64) and not one.is_cuda and np.array_equal(one[1].numpy(), N.rgb_to_nv12(imgs[2][::-1]))


# ------------------------------------------------------------------------------------------------------------ the net-level calls
def _net(kind, dtype):
    net = getattr(D, kind)(synth.vgg19_standin(seed=0))
    synth.fill_params_(net, 11)
    # every pixel's box is 17 x 13 pixels around it, as tests/test_hip_redact.py sets it
    with torch.no_grad():
        net.conv5_2_loc.weight.zero_()
        net.conv5_2_loc.bias.copy_(torch.tensor([2.0, 1.5, -2.0, -1.5]))
    net = net.cuda().eval()
    net.compute_dtype = dtype
    return net


def _same_rows(got, want):
    assert len(got) == len(want)
    for (d, k), (rd, rk) in zip(got, want):
        assert np.array_equal(_bits(d), _bits(rd)) and k == rk


@pytest.mark.parametrize('dtype', ['f32', 'f16'])
@pytest.mark.parametrize('kind', ['DenseBox', 'DenseBoxLMLOC'])
def test_net_calls_equal_the_rgb_calls_on_the_restated_frames(kind, dtype):
    net = _net(kind, dtype)
    rs = np.random.RandomState(31)
    p = color.Params(601, 'full', 'rgb')
    kw = dict(K=10, max_batch=3)
    nv = [rs.randint(0, 256, size=(96, 70)).astype(np.uint8) for _ in range(4)]          # 64 x 64, pitch 70
    X = torch.from_numpy(np.stack([N.nv12_to_rgb(f, 64, 601, 'full') for f in nv])).cuda()
    _same_rows(net.detect_batch_nv12(nv, 64, p, **kw), net.detect_batch(X, **kw))
    _same_rows(net.detect_batch_nv12(torch.from_numpy(np.stack(nv)).cuda(), 64, p, **kw), net.detect_batch(X, **kw))
    wide = [rs.randint(0, 256, size=(72, 80)).astype(np.uint8) for _ in range(4)]        # 48 x 80
    wide[1] = torch.from_numpy(wide[1]).cuda()
    W = [torch.from_numpy(N.nv12_to_rgb(f if isinstance(f, np.ndarray) else f.cpu().numpy(), None, 601, 'full')) for f in wide]
    got, want = net.detect_batch_resized_nv12(wide, 64, params=p, **kw), net.detect_batch_resized(W, 64, **kw)
    _same_rows(got, want)
    got = net.detect_batch_resized_nv12(wide, 64, params=p, score_thresh=0.3, max_dets=64)
    _same_rows(got, net.detect_batch_resized(W, 64, score_thresh=0.3, max_dets=64))

    # redaction: NV12 in, NV12 out, each frame returned in the kind it came in, over two calls
    st = redact.Redaction(method='pixelate', cell=5)
    frames = [nv[0], torch.from_numpy(nv[1]), torch.from_numpy(nv[2]).cuda(), nv[3]]
    for with_tracker in (False, True):
        tr, ref_tr = (T.Tracker(5, max_tracks=64, max_age=2), T.Tracker(5, max_tracks=64, max_age=2)) if with_tracker else (None, None)
        for call in range(2):
            got = net.redact_batch_nv12(frames, width=64, tracker=tr, stream0=1, style=st, params=p, **kw)
            want = net.redact_batch(X, tracker=ref_tr, stream0=1, style=st, **kw)
            assert isinstance(got[0][3], np.ndarray) and torch.is_tensor(got[1][3]) and not got[1][3].is_cuda and got[2][3].is_cuda
            for b, ((d, keep, tid, f), (rd, rkeep, rtid, painted)) in enumerate(zip(got, want)):
                assert np.array_equal(_bits(d), _bits(rd)) and keep == rkeep
                assert (tid is None and rtid is None) if not with_tracker else tid.tolist() == rtid.tolist()
                host = f if isinstance(f, np.ndarray) else f.cpu().numpy()
                assert host.dtype == np.uint8 and host.shape == (96, 64)
                assert np.array_equal(host, N.rgb_to_nv12(painted.cpu().numpy(), 601, 'full')), (with_tracker, call, b)
            assert any(not np.array_equal(w[3].cpu().numpy(), x.cpu().numpy()) for w, x in zip(want, X)), 'nothing was redacted'
        if with_tracker:
            h, t = tr._host_state()
            rh, rt = ref_tr._host_state()
            assert h.tolist() == rh.tolist() and np.array_equal(_bits(t), _bits(rt))


def test_python_level_refusals():
    good = np.zeros((24, 40), np.uint8)
    calls = [('nv12_to_rgb_batch', lambda f, **k: color.nv12_to_rgb_batch(f, **k)),
             ('pad_resize_batch_nv12', lambda f, **k: resize.pad_resize_batch_nv12(f, 32, **k)),
             ('crop_resize_batch_nv12', lambda f, **k: resize.crop_resize_batch_nv12(f, [[(0, 0, 2, 2)]] * len(f), (8, 8), **k)),
             ('detect_batch_nv12', lambda f, **k: color.detect_batch_nv12(None, f, **k)),
             ('detect_batch_resized_nv12', lambda f, **k: color.detect_batch_resized_nv12(None, f, 32, **k)),
             ('redact_batch_nv12', lambda f, **k: color.redact_batch_nv12(None, f, **k))]
    for name, call in calls:
        for frames, k in (([np.zeros((25, 40), np.uint8)], {}),                              # rows not h * 3 / 2 with h even
                          ([good], dict(width=39)),                                          # odd width
                          ([good], dict(width=42)),                                          # width > pitch
                          ([np.zeros((24, 41), np.uint8)], {}),                              # odd pitch taken as the width
                          ([good.astype(np.int16)], {}), ([np.zeros((2, 24, 40), np.uint8)], {}), ([good], dict(width=[40, 40])),
                          ([good], dict(params='601')), ([], {})):
            with pytest.raises(RuntimeError, match=name):
                call(frames, **k)
        with pytest.raises(RuntimeError, match=name):
            call(torch.zeros((24, 40), dtype=torch.uint8))                                  # a batch tensor is three-dimensional
    for name in ('detect_batch_nv12', 'redact_batch_nv12'):
        with pytest.raises(RuntimeError, match=name + '.*one size'):
            getattr(color, name)(None, [good, np.zeros((24, 42), np.uint8)])
    with pytest.raises(RuntimeError, match='rgb_to_nv12_batch'):
        color.rgb_to_nv12_batch([np.zeros((3, 4, 3), np.uint8)])
    with pytest.raises(RuntimeError, match='rgb_to_nv12_batch'):
        color.rgb_to_nv12_batch([np.zeros((4, 4), np.uint8)])
    for kw in (dict(standard=600), dict(range='wide'), dict(order='gbr'), dict(standard=601.5)):
        with pytest.raises(RuntimeError, match='Params'):
            color.Params(**kw)
