"""Batched pad + bicubic resize on the GPU: every output of dbx_resize_cubic_batch_u8 -- through the C ABI, resize.pad_resize_batch and
resize.crop_resize_batch -- is bit for bit the NumPy restatement tests/cubic_ref.py (integer arithmetic: there is no tolerance to
choose); detect_batch_resized is detect_batch on the resized frames plus the documented float64 map back to the source frame."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cubic_ref as R                                   # noqa: E402

import densebox_amd as D                                # noqa: E402
from densebox_amd import _lib, rectify, resize, synth   # noqa: E402
from densebox_amd._lib import check, stream_ptr         # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def _img(rs, h, w, c, stripes=True):
    img = rs.randint(0, 256, size=(h, w, c)).astype(np.uint8)
    if stripes and h > 8 and w > 12:                     # rows of 0 and columns of 255: over- and undershoot saturate
        img[::7] = 0
        img[:, ::11] = 255
    return img


# (image index, crop (cx0, cy0, cw, ch) or None, pad (l, t, r, b), pad_value, dh, dw, dst_off % 16)
def _abi_jobs(sizes):
    full = lambda i: (0, 0, sizes[i][1], sizes[i][0])     # noqa: E731
    return [
        (0, None, (0, 0, 0, 0), 0, 8, 8, 0),               # 1 x 1 source, up-scale
        (0, None, (2, 1, 0, 3), 128, 5, 7, 1),             # 1 x 1 source inside padding
        (1, None, (0, 0, 0, 0), 0, 9, 9, 2),               # 2 x 3
        (2, None, (0, 0, 0, 0), 0, 64, 64, 3),             # 37 x 53 up-scale, non-uniform
        (2, None, (0, 8, 0, 8), 128, 240, 240, 4),         # pad_img geometry of a landscape image
        (3, None, (26, 0, 27, 0), 128, 64, 64, 8),         # portrait, odd difference
        (2, (0, 0, 20, 15), (0, 0, 0, 0), 0, 33, 47, 5),   # crop touching the left / top border
        (2, (33, 22, 20, 15), (0, 0, 0, 0), 0, 31, 17, 6),  # crop touching the right / bottom border
        (2, (10, 0, 30, 37), (3, 0, 0, 5), 7, 50, 100, 7),
        (2, (0, 5, 53, 20), (0, 2, 9, 0), 255, 13, 130, 9),
        (4, None, (0, 0, 0, 0), 0, 300, 300, 0),           # 480 x 640 down-scale by non-integer factors, non-uniform
        (4, None, (0, 80, 0, 80), 128, 512, 512, 12),
        (4, (100, 50, 300, 200), (0, 0, 0, 0), 0, 240, 240, 10),
        (4, (0, 0, 640, 480), (0, 0, 0, 0), 0, 480, 640, 11),   # identity
        (4, (639, 0, 1, 480), (0, 0, 0, 0), 0, 7, 3, 13),  # one source column
        (4, (0, 479, 640, 1), (1, 1, 1, 1), 200, 3, 65, 14),    # one source row, 65 = a tile and one pixel
        (5, None, (0, 420, 0, 420), 128, 720, 720, 0),     # 1080 x 1920 frame, the flagship geometry
        (5, None, (0, 0, 0, 0), 0, 101, 203, 15),          # strong down-scale: taps of neighbouring pixels do not overlap
        (5, (1000, 500, 400, 300), (0, 0, 0, 0), 0, 240, 240, 4),
        (5, (1520, 780, 400, 300), (0, 0, 0, 0), 0, 61, 127, 1),
        (3, None, (0, 0, 0, 0), 0, 1, 1, 3),               # a single destination pixel
        (3, None, (0, 0, 0, 0), 0, 1, 200, 2),             # a single destination row
        (3, None, (0, 0, 0, 0), 0, 200, 1, 5),             # a single destination column
        (2, None, (0, 0, 0, 0), 0, 17, 16, 8),
        (2, None, (0, 0, 0, 0), 0, 16, 4, 4),
        (1, None, (40, 40, 40, 40), 3, 90, 90, 0),         # mostly padding
    ]


@pytest.mark.parametrize('c', [1, 3, 4])
def test_abi_mixed_jobs_are_bitwise_the_restatement_and_write_nothing_else(c):
    rs = np.random.RandomState(100 + c)
    sizes = [(1, 1), (2, 3), (37, 53), (80, 27), (480, 640), (1080, 1920)]
    imgs = [_img(rs, h, w, c) for h, w in sizes]
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    spec = _abi_jobs(sizes)
    assert len(spec) >= 24
    offs, pos = [], 0
    for (_, _, _, _, dh, dw, res) in spec:
        pos += 5
        pos += (res - pos % 16) % 16                       # pos % 16 = the listed residue
        offs.append(pos)
        pos += dh * dw * c
    assert {o % 16 for o in offs} == set(range(16))
    arena = torch.full((pos + 64,), SENTINEL, dtype=torch.uint8, device='cuda')
    assert arena.data_ptr() % 16 == 0
    jobs = (_lib.ResizeJob * len(spec))()
    for r, (i, crop, pad, pv, dh, dw, _), off in zip(jobs, spec, offs):
        h, w = sizes[i]
        r.src, r.sh, r.sw = dev[i].data_ptr(), h, w
        r.cx0, r.cy0, r.cw, r.ch = crop if crop is not None else (0, 0, w, h)
        r.pad_l, r.pad_t, r.pad_r, r.pad_b = pad
        r.pad_value, r.dh, r.dw, r.dst_off = pv, dh, dw, off
    L = _lib.lib()
    ws = torch.empty(L.dbx_resize_batch_workspace_bytes(len(spec)), dtype=torch.uint8, device='cuda')

    def run():
        arena.fill_(SENTINEL)
        check(L.dbx_resize_cubic_batch_u8(jobs, len(spec), c, C.c_void_p(arena.data_ptr()), C.c_void_p(ws.data_ptr()), stream_ptr()))
        return arena.cpu().numpy()
    got = run()
    untouched = np.ones(got.size, dtype=bool)
    for k, ((i, crop, pad, pv, dh, dw, _), off) in enumerate(zip(spec, offs)):
        ref = R.resize_cubic_u8(R.virtual_source(imgs[i], crop, pad, pv), dh, dw)
        blk = got[off:off + dh * dw * c].reshape(dh, dw, c)
        assert np.array_equal(blk, ref), (k, spec[k], int(np.abs(blk.astype(int) - ref).max()), int((blk != ref).sum()))
        untouched[off:off + dh * dw * c] = False
    assert (got[untouched] == SENTINEL).all()
    assert np.array_equal(run(), got)                      # no atomics, no order dependence: a second call gives the same bytes


def _mixed_frames(rs, c=3):
    return [_img(rs, h, w, c) for h, w in ((480, 640), (640, 480), (333, 333), (301, 500), (500, 301), (720, 1280), (97, 64))]


@pytest.mark.parametrize('size', [720, 512])
def test_pad_resize_batch_is_the_restatement_of_resize_of_pad_img(size):
    rs = np.random.RandomState(size)
    frames = _mixed_frames(rs)
    out = resize.pad_resize_batch(frames, size)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (len(frames), size, size, 3) and out.is_contiguous()
    got = out.cpu().numpy()
    for b, im in enumerate(frames):
        padded = resize.pad_img(im)
        assert padded.shape[0] == padded.shape[1]
        assert np.array_equal(got[b], R.resize_cubic_u8(padded, size, size)), b
    cpu = resize.pad_resize_batch([torch.from_numpy(f) for f in frames], size)
    cuda = resize.pad_resize_batch([torch.from_numpy(f).cuda() for f in frames], size)
    assert torch.equal(cpu, out) and torch.equal(cuda, out)
    same = np.stack([frames[0], frames[0][::-1].copy()])
    for batch in (torch.from_numpy(same), torch.from_numpy(same).cuda()):      # a [B,H,W,C] tensor
        t = resize.pad_resize_batch(batch, size).cpu().numpy()
        assert np.array_equal(t[0], got[0]) and np.array_equal(t[1], R.pad_resize(same[1], size))


def test_pad_resize_batch_grey_images_and_small_sizes():
    rs = np.random.RandomState(9)
    frames = [_img(rs, h, w, 1) for h, w in ((50, 81), (81, 50), (1, 9))]
    got = resize.pad_resize_batch(frames, 36).cpu().numpy()
    for b, im in enumerate(frames):
        assert np.array_equal(got[b, :, :, 0], R.resize_cubic_u8(resize.pad_img(im[:, :, 0]), 36, 36)), b


def test_crop_resize_batch_is_the_restatement_on_numpy_slices():
    rs = np.random.RandomState(12)
    frames = [_img(rs, 200, 300, 3), _img(rs, 150, 90, 3), _img(rs, 64, 64, 3)]
    windows = [[(10, 20, 250, 180), (-50, -40, 400, 500), (0, 0, 300, 200), (290, 190, 1000, 1000)],     # numpy clamps these
               [],
               [(0, 0, 64, 64), (-10, 5, -2, 60), (30, -20, 64, 64)]]
    for size in ((240, 240), (100, 37)):
        out = resize.crop_resize_batch(frames, windows, size)
        n = sum(len(w) for w in windows)
        assert out.is_cuda and tuple(out.shape) == (n, size[1], size[0], 3)
        got, p = out.cpu().numpy(), 0
        for im, wins in zip(frames, windows):
            for (x0, y0, x1, y1) in wins:
                crop = im[y0:y1, x0:x1]
                assert crop.size > 0
                assert np.array_equal(got[p], R.resize_cubic_u8(crop, size[1], size[0])), (p, x0, y0, x1, y1)
                p += 1
        assert torch.equal(resize.crop_resize_batch([torch.from_numpy(f).cuda() for f in frames], windows, size), out)


def _net(kind, dtype='f32'):
    net = getattr(D, kind)(synth.vgg19_standin(seed=0))
    synth.fill_params_(net, 11)
    net = net.cuda().eval()
    net.compute_dtype = dtype
    return net


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


@pytest.mark.parametrize('kind', ['DenseBoxLMLOC', 'DenseBox'])
def test_detect_batch_resized_is_detect_batch_on_the_resized_frames_mapped_back(kind):
    net = _net(kind)
    rs = np.random.RandomState(21)
    frames = [_img(rs, h, w, 3) for h, w in ((120, 200), (200, 120), (160, 160), (97, 240), (240, 97), (120, 200))]
    size = 240
    ref = net.detect_batch(resize.pad_resize_batch(frames, size), K=10)
    graphs = dict(net.__dict__['_detect_graphs'])
    net.__dict__['_detect_graphs'].clear()
    res = net.detect_batch_resized(frames, size=size, K=10)
    cache = net.__dict__['_detect_graphs']
    assert len(cache) == 1 and next(iter(cache))[0] == 'batch' and next(iter(cache))[1] == (len(frames), size, size, 3), list(cache)
    assert list(cache) == list(graphs)
    assert len(res) == len(frames)
    for im, (d, keep), (d0, keep0) in zip(frames, res, ref):
        h, w = im.shape[:2]
        side, pad_x, pad_y = max(h, w), ((h - w) // 2 if h > w else 0), ((w - h) // 2 if h <= w else 0)
        assert (side, pad_x, pad_y) == resize.pad_geometry(h, w)
        want = d0.copy()
        for col in range(d0.shape[1]):
            if col == 4:
                continue
            is_x = col in (0, 2) or (col >= 5 and col % 2 == 1)
            want[:, col] = d0[:, col] * (side / size) - (pad_x if is_x else pad_y)
        assert keep == keep0
        assert d.dtype == np.float64 and d.shape == d0.shape == (10, 5 if kind == 'DenseBox' else 13)
        assert np.array_equal(_bits(d), _bits(want))
        assert np.array_equal(_bits(d[:, 4]), _bits(d0[:, 4]))
    res2 = net.detect_batch_resized([torch.from_numpy(f) for f in frames], size=size, K=10, max_batch=2)
    for (d, keep), (d2, keep2) in zip(res, res2):
        assert keep == keep2 and np.array_equal(_bits(d), _bits(d2))


def test_detections_of_resized_frames_rectify_plates_of_the_source_frames():
    net = _net('DenseBoxLMLOC')
    rs = np.random.RandomState(22)
    frames = [_img(rs, h, w, 3) for h, w in ((120, 200), (200, 120), (160, 160))]
    res = net.detect_batch_resized(frames, size=240, K=10)
    quads = [[[d[k, 5:7], d[k, 7:9], d[k, 9:11], d[k, 11:13]] for k in keep] for d, keep in res]
    plates = rectify.perspective_transform_batch(frames, quads, region='canvas')
    assert [len(p) for p in plates] == [len(keep) for _, keep in res]
    n = 0
    for im, ps in zip(frames, plates):
        for p in ps:
            if p is None:
                continue
            n += 1
            assert isinstance(p, np.ndarray) and p.dtype == np.uint8 and p.shape == rectify.canvas_size(*im.shape[:2]) + (3,)
    assert sum(len(keep) for _, keep in res) > 0
    print('%d plates rectified from %d kept rows' % (n, sum(len(keep) for _, keep in res)))
