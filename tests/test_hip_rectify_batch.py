"""Batched plate rectification on the GPU: every output of dbx_warp_perspective_batch_u8 (through rectify.perspective_transform_batch)
is bit for bit the single-plate warp's -- the whole canvas, or its plate window -- across image sizes, channel counts, quads partly
outside the image, degenerate / NaN quads and an output arena above 2 GiB; detect_plates is detect_batch plus those warps."""
import numpy as np
import pytest
import torch

import densebox_amd as D
from densebox_amd import rectify, synth
from oracle import densebox_oracle as O

pytestmark = pytest.mark.gpu


def _quads(rs, h, w, n):
    """n plausible plate quads on an h x w image (a skewed rectangle, jittered corners); the last two reach past the image."""
    out = []
    for i in range(n):
        cx, cy = rs.uniform(0.2, 0.8) * w, rs.uniform(0.2, 0.8) * h
        hw, hh = rs.uniform(0.08, 0.3) * w, rs.uniform(0.05, 0.2) * h
        if i >= n - 2:
            cx, hw = (-0.05 * w if i == n - 1 else 1.02 * w), 0.2 * w
        c = np.array([[cx - hw, cy - hh], [cx + hw, cy - hh * 0.9], [cx + hw * 0.95, cy + hh], [cx - hw * 1.05, cy + hh * 1.1]])
        out.append((c + rs.uniform(-0.02, 0.02, size=(4, 2)) * np.array([w, h])).tolist())
    return out


def _np(x):
    return x.cpu().numpy() if torch.is_tensor(x) else x


def _window(q, h, w):
    dh, dw = rectify.canvas_size(h, w)
    return rectify.plate_window(rectify.dst_rectangle(q), dh, dw)


@pytest.mark.parametrize('c', [1, 3, 4])
def test_canvas_and_plate_parity_mixed_sizes(c):
    rs = np.random.RandomState(10 + c)
    sizes = [(120, 200), (61, 47), (1080, 1920), (33, 90)]
    imgs = [rs.randint(0, 256, size=(h, w, c)).astype(np.uint8) for h, w in sizes]
    quads = [_quads(rs, h, w, 4) for h, w in sizes]
    quads[3] = []                                                      # an image with no quads
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    canv = rectify.perspective_transform_batch(dev, quads, region='canvas')
    plate = rectify.perspective_transform_batch(imgs, quads, region='plate')   # numpy in -> numpy out
    assert [len(o) for o in canv] == [len(o) for o in plate] == [4, 4, 4, 0]
    for b, (h, w) in enumerate(sizes):
        for j, q in enumerate(quads[b]):
            got = canv[b][j]
            assert torch.is_tensor(got) and got.is_cuda
            got = got.cpu().numpy()
            ref = _np(rectify.perspective_transform(dev[b], q))
            assert got.shape == ref.shape == rectify.canvas_size(h, w) + (c,)
            assert np.array_equal(got, ref), (b, j)
            if h * w <= 120 * 200:
                assert np.array_equal(got, O.perspective_transform(imgs[b], q)), (b, j)
            x0, y0, oh, ow = _window(q, h, w)
            p = plate[b][j]
            assert isinstance(p, np.ndarray) and p.shape == (oh, ow, c)
            assert np.array_equal(p, ref[y0:y0 + oh, x0:x0 + ow]), (b, j)


def test_batch_tensor_input_and_bad_quads_next_to_good_ones():
    rs = np.random.RandomState(3)
    x = torch.from_numpy(rs.randint(0, 256, size=(3, 96, 160, 3)).astype(np.uint8))      # CPU tensor in -> CPU tensors out
    good = [_quads(rs, 96, 160, 3) for _ in range(3)]
    nan = float('nan')
    quads = [[good[0][0], [[0, 0], [1, 1], [2, 2], [3, 3]], good[0][1]],              # degenerate corners
             [[[5, 5], [nan, 5], [40, 30], [5, 30]], good[1][0]],                       # a NaN coordinate
             [[[-60, -50], [-40, -50], [-38, -30], [-61, -32]], good[2][2], good[2][1]]]  # an empty plate window
    for region in ('canvas', 'plate'):
        out = rectify.perspective_transform_batch(x, quads, region=region)
        assert out[0][1] is None and out[1][0] is None
        assert (out[2][0] is None) == (region == 'plate')
        for b, qs in enumerate(quads):
            for j, q in enumerate(qs):
                if out[b][j] is None:
                    continue
                assert torch.is_tensor(out[b][j]) and not out[b][j].is_cuda
                ref = O.perspective_transform(x[b].numpy(), q)
                if region == 'plate':
                    x0, y0, oh, ow = _window(q, 96, 160)
                    ref = ref[y0:y0 + oh, x0:x0 + ow]
                assert np.array_equal(out[b][j].numpy(), ref), (region, b, j)


def test_arena_above_2_gib_uses_64_bit_offsets():
    rs = np.random.RandomState(4)
    h, w = 1080, 1920
    img = torch.from_numpy(rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).cuda()
    n = 160
    quads = _quads(rs, h, w, n)
    dh, dw = rectify.canvas_size(h, w)
    assert n * dh * dw * 3 > 2 ** 31
    out = rectify.perspective_transform_batch([img], [quads], region='canvas')[0]
    assert out[-1].data_ptr() - out[0].data_ptr() + dh * dw * 3 > 2 ** 31
    for j in (0, n - 2, n - 1):
        assert torch.equal(out[j], rectify.perspective_transform(img, quads[j])), j
    del out
    torch.cuda.empty_cache()


def _net(kind, dtype):
    net = getattr(D, kind)(synth.vgg19_standin(seed=0))
    synth.fill_params_(net, 11)
    net = net.cuda().eval()
    net.compute_dtype = dtype
    return net


def _check_plates(res, ref, frames, region):
    assert len(res) == len(ref) == len(frames)
    n = 0
    for (d, keep, plates), (d0, keep0), f in zip(res, ref, frames):
        assert d.dtype == d0.dtype and np.array_equal(d.view(np.uint8), d0.view(np.uint8)) and keep == keep0
        assert len(plates) == len(keep)
        f = _np(f)
        for j, k in enumerate(keep):
            q = [[d[k, 5], d[k, 6]], [d[k, 7], d[k, 8]], [d[k, 9], d[k, 10]], [d[k, 11], d[k, 12]]]
            try:
                ok = np.all(np.isfinite(np.float32(q)))
                want = rectify.perspective_transform(f, q) if ok else None
            except RuntimeError:                               # degenerate corners
                want = None
            if want is not None and region == 'plate':
                win = _window(q, f.shape[0], f.shape[1])
                want = None if win is None else want[win[1]:win[1] + win[2], win[0]:win[0] + win[3]]
            if want is None:
                assert plates[j] is None
                continue
            n += 1
            assert np.array_equal(_np(plates[j]), want), (k, j)
    return n


@pytest.mark.parametrize('kind', ['DenseBoxLM', 'DenseBoxLMLOC'])
@pytest.mark.parametrize('dtype', ['f32', 'f16'])
def test_detect_plates_is_detect_batch_plus_the_warps(kind, dtype):
    net = _net(kind, dtype)
    rs = np.random.RandomState(5)
    x = torch.from_numpy(rs.randint(0, 256, size=(3, 240, 240, 3)).astype(np.uint8))
    ref = net.detect_batch(x.cuda(), K=10)
    res = net.detect_plates(x, K=10, region='canvas')
    checked = _check_plates(res, ref, [x[b] for b in range(3)], 'canvas')
    assert all(p is None or (torch.is_tensor(p) and not p.is_cuda) for _, _, ps in res for p in ps)
    mixed = [rs.randint(0, 256, size=s).astype(np.uint8) for s in ((240, 240, 3), (160, 208, 3), (240, 240, 3))]
    ref = net.detect_batch([torch.from_numpy(m) for m in mixed], K=10, max_batch=1)
    res = net.detect_plates([torch.from_numpy(m).cuda() for m in mixed], K=10, max_batch=1, region='plate')
    checked += _check_plates(res, ref, mixed, 'plate')
    assert all(p is None or p.is_cuda for _, _, ps in res for p in ps)
    assert checked > 0


@pytest.mark.parametrize('c', [1, 2, 3, 4])
def test_abi_job_offsets_of_every_alignment(c):
    """dbx_warp_perspective_batch_u8 called directly with job offsets that are odd, 2 mod 4, 4-aligned but not 16-aligned and 16-aligned
    (every store path of the kernel), windows smaller than one word, one row, and a whole canvas: each window is bitwise the
    single-image warp's, and not a byte between the windows is written."""
    import ctypes as C
    from densebox_amd import _lib
    from densebox_amd._lib import check, stream_ptr
    rs = np.random.RandomState(30 + c)
    h, w = 70, 90
    img = torch.from_numpy(rs.randint(0, 256, size=(h, w, c)).astype(np.uint8)).cuda()
    dh, dw = rectify.canvas_size(h, w)
    qs = _quads(rs, h, w, 6)
    wins = [_window(qs[0], h, w), (0, 0, dh, dw), (10, 7, 3, 5), (0, dh - 1, 1, dw), (dw - 1, 3, 4, 1), _window(qs[1], h, w)]
    mats = [rectify.get_perspective_matrix(q, rectify.dst_rectangle(q)) for q in qs]
    offs, pos = [], 0
    for k, (x0, y0, oh, ow) in enumerate(wins):
        pos += 5
        pos += [1, 2, 4, 0, 3, 8][k] - pos % 16 + (16 if [1, 2, 4, 0, 3, 8][k] < pos % 16 else 0)   # pos % 16 = the listed residue
        offs.append(pos)
        pos += oh * ow * c
    assert sorted({o % 16 for o in offs}) == [0, 1, 2, 3, 4, 8]
    arena = torch.full((pos + 64,), 0xA5, dtype=torch.uint8, device='cuda')
    jobs = (_lib.WarpJob * len(wins))()
    for r, (x0, y0, oh, ow), M, off in zip(jobs, wins, mats, offs):
        r.src, r.sh, r.sw = img.data_ptr(), h, w
        r.m9[:] = [float(v) for v in M.reshape(9)]
        r.dh, r.dw, r.x0, r.y0, r.oh, r.ow, r.dst_off = dh, dw, x0, y0, oh, ow, off
    L = _lib.lib()
    ws = torch.empty(L.dbx_warp_batch_workspace_bytes(len(wins)), dtype=torch.uint8, device='cuda')
    check(L.dbx_warp_perspective_batch_u8(jobs, len(wins), c, C.c_void_p(arena.data_ptr()), C.c_void_p(ws.data_ptr()), stream_ptr()))
    got = arena.cpu().numpy()
    untouched = np.ones(got.size, dtype=bool)
    for (x0, y0, oh, ow), M, off in zip(wins, mats, offs):
        ref = rectify.warp_perspective(img, M, (dw, dh)).cpu().numpy()[y0:y0 + oh, x0:x0 + ow]
        assert np.array_equal(got[off:off + oh * ow * c].reshape(oh, ow, c), ref), (off, x0, y0, oh, ow)
        untouched[off:off + oh * ow * c] = False
    assert (got[untouched] == 0xA5).all()
