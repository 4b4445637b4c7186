"""Fixed-size plate crops rectified on the device (dbx_plate_crops_batch, rectify.plate_crops_batch, detect_plate_crops): the matrices
the kernel solves are bit for bit the host solver's; every crop is bit for bit the single-plate warp with the host matrix, across
channel counts, crop sizes that put the slot bases on every alignment and more than one tile per slot; `sel` picks rows in its own
order; detect_plate_crops is detect_batch plus that composition, captured in one graph per chunk shape and crop size.

Bitwise equality of the device solve with the host solve rests on fp64 add, multiply, divide and fabs being correctly rounded on gfx950
with contraction off; test_device_matrices_equal_the_host_solver_bitwise is the test of that."""
import ctypes as C

import numpy as np
import pytest
import torch

import densebox_amd as D
from densebox_amd import _lib, rectify, synth
from densebox_amd._lib import check, stream_ptr

pytestmark = pytest.mark.gpu

NAN, INF = float('nan'), float('inf')
# an axis-aligned rectangle, a skewed plate, a rotated one, corners outside the frame, a nearly flat quad that still passes; then three
# collinear points, a repeated corner, a NaN, an inf and a coordinate that overflows float32
QUADS = [
    [[5, 6], [40, 6], [40, 20], [5, 20]],
    [[8.3, 10.7], [41.2, 7.9], [43.6, 22.4], [6.1, 25.2]],
    [[30.5, 4.25], [50.75, 24.5], [44.0, 31.5], [23.25, 11.0]],
    [[-12.5, -7.0], [70.0, -3.5], [75.5, 55.0], [-9.0, 60.25]],
    [[10, 20], [50, 20], [50, 20.001], [10, 20.001]],
    [[0, 0], [10, 10], [20, 20], [0, 30]],
    [[5, 5], [5, 5], [30, 20], [5, 20]],
    [[5, 5], [NAN, 5], [40, 30], [5, 30]],
    [[5, 5], [40, 5], [40, INF], [5, 30]],
    [[5, 5], [1e300, 5], [40, 30], [5, 30]],
]
N_GOOD = 5                                  # the first five are valid at every size but (1, 1)
FRAME_SIZES = [(48, 64), (37, 29)]
GUARD = 64                                  # bytes (dst) and words (ok) of guard on each side; a multiple of 16 keeps dst's alignment
FILL = 0xAB


def _host_matrix(q, size):
    """The forward matrix of quad q onto plate_rectangle(size), or None exactly where rectify._rect_job gives None for its corners: a
    coordinate that is not finite in float32, a solve that dbx_perspective_matrix refuses, a map that is not invertible."""
    q = np.asarray(q, dtype=np.float64).reshape(4, 2)
    with np.errstate(over='ignore'):
        if not np.all(np.isfinite(np.float32(q))):
            return None
        try:
            M = rectify.get_perspective_matrix(q.tolist(), rectify.plate_rectangle(size))
        except RuntimeError:
            return None
    return M if rectify._invertible(M) else None


def _frames(c, seed=7):
    rs = np.random.RandomState(seed + c)
    return [torch.from_numpy(rs.randint(0, 256, size=(h, w, c)).astype(np.uint8)).cuda() for h, w in FRAME_SIZES]


def _launch(frames, quads, size, sel=None, slots=None):
    """dbx_plate_crops_batch called directly: quads float64 [B, Q, 8]; returns (crops [B, slots, oh, ow, c], ok [B, slots], m9 [B, slots, 9])
    as numpy arrays after checking that the guard bytes around dst and ok still hold the fill."""
    ow, oh = size
    B, Q = quads.shape[:2]
    slots = Q if slots is None else slots
    c = int(frames[0].size(2))
    table = rectify.frame_table(frames)
    dq = torch.from_numpy(np.ascontiguousarray(quads, dtype=np.float64)).cuda()
    dsel = None if sel is None else torch.from_numpy(np.ascontiguousarray(sel, dtype=np.int32)).cuda()
    n = B * slots * oh * ow * c
    dst = torch.full((GUARD + n + GUARD,), FILL, dtype=torch.uint8, device='cuda')
    ok = torch.full((GUARD + B * slots + GUARD,), FILL, dtype=torch.int32, device='cuda')
    m9 = torch.full((B, slots, 9), NAN, dtype=torch.float64, device='cuda')
    check(_lib.lib().dbx_plate_crops_batch(C.c_void_p(table.data_ptr()), B, c, C.c_void_p(dq.data_ptr()), 8, Q * 8, _lib.ptr(dsel), slots,
                                           ow, oh, C.c_void_p(dst.data_ptr() + GUARD), C.c_void_p(ok.data_ptr() + 4 * GUARD),
                                           C.c_void_p(m9.data_ptr()), stream_ptr()))
    dst, ok = dst.cpu().numpy(), ok.cpu().numpy()
    assert (dst[:GUARD] == FILL).all() and (dst[GUARD + n:] == FILL).all(), 'bytes outside dst were written'
    assert (ok[:GUARD] == FILL).all() and (ok[GUARD + B * slots:] == FILL).all(), 'words outside ok were written'
    return dst[GUARD:GUARD + n].reshape(B, slots, oh, ow, c), ok[GUARD:GUARD + B * slots].reshape(B, slots), m9.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


@pytest.mark.parametrize('size', [(94, 24), (2, 2), (1, 1)])
def test_device_matrices_equal_the_host_solver_bitwise(size):
    frames = _frames(3)
    quads = np.array([QUADS, QUADS], dtype=np.float64).reshape(2, len(QUADS), 8)
    want = [_host_matrix(q, size) for q in QUADS]
    assert [m is not None for m in want] == [size != (1, 1)] * N_GOOD + [False] * (len(QUADS) - N_GOOD)
    _, ok, m9 = _launch(frames, quads, size)
    for b in range(2):
        assert ok[b].tolist() == [int(m is not None) for m in want], (b, ok[b])
        for j, m in enumerate(want):
            if m is not None:
                assert np.array_equal(_bits(m9[b, j]), _bits(m)), (b, j, m9[b, j], m.reshape(9))


@pytest.mark.parametrize('c', [1, 3, 4])
def test_crops_equal_the_single_plate_warp_bitwise(c):
    frames = _frames(c)
    Q = len(QUADS)
    quads = np.array([QUADS, QUADS[::-1]], dtype=np.float64).reshape(2, Q, 8)        # frame 1 reads the list backwards
    # frame 0: every row in order; frame 1: seven rows out of order (two of them bad), so three slots lie past its count
    sel = np.zeros((2, Q + 1), dtype=np.int32)
    sel[0] = [Q] + list(range(Q))
    sel[1, :8] = [7, 9, 2, 8, 0, 5, 7, 6]
    bases = set()
    for size in ((94, 24), (33, 7), (2, 2), (100, 41)):
        ow, oh = size
        crops, ok, _ = _launch(frames, quads, size, sel=sel)
        n_ok = 0
        for b in range(2):
            for j in range(Q):
                M = _host_matrix(quads[b, sel[b, 1 + j]], size) if j < sel[b, 0] else None
                assert ok[b, j] == int(M is not None), (size, b, j)
                if M is None:
                    assert not crops[b, j].any(), (size, b, j)
                    continue
                n_ok += 1
                ref = rectify.warp_perspective(frames[b], M, size).cpu().numpy()
                assert ref.shape == (oh, ow, c)
                assert np.array_equal(crops[b, j], ref), (size, b, j)
                bases.add((b * Q + j) * oh * ow * c % 16)
        assert n_ok == 2 * N_GOOD and crops.any(), (size, n_ok)  # rows 9, 8, 5, 7, 6 of the reversed list are QUADS[0], [1], [4], [2], [3]
    if c == 3:               # 693 bytes per slot at (33, 7): odd, 2 mod 4, 4-aligned and 16-aligned slot bases all hold an ok crop
        assert {b % 2 for b in bases} == {0, 1} and any(b % 4 == 2 for b in bases) and any(b % 16 in (4, 8, 12) for b in bases) and 0 in bases


def test_sel_picks_rows_in_its_own_order():
    frames = _frames(3)
    quads = np.array([QUADS[:5], QUADS[4::-1]], dtype=np.float64).reshape(2, 5, 8)
    size = (33, 7)
    plain, ok_plain, _ = _launch(frames, quads, size, sel=None)          # NULL: rows 0..4 in order
    assert ok_plain.tolist() == [[1] * 5] * 2
    for b in range(2):
        for j in range(5):
            ref = rectify.warp_perspective(frames[b], _host_matrix(quads[b, j], size), size).cpu().numpy()
            assert np.array_equal(plain[b, j], ref), (b, j)
    assert len({plain[0, j].tobytes() for j in range(5)}) == 5           # the rows differ, so an order mix-up would show
    sel = np.array([[3, 3, 0, 2, 1, 4], [2, 4, 1, 0, 0, 0]], dtype=np.int32)
    got, ok, _ = _launch(frames, quads, size, sel=sel)
    assert ok.tolist() == [[1, 1, 1, 0, 0], [1, 1, 0, 0, 0]]
    for b in range(2):
        for j in range(5):
            if j < sel[b, 0]:
                assert np.array_equal(got[b, j], plain[b, sel[b, 1 + j]]), (b, j)
            else:
                assert not got[b, j].any(), (b, j)


def test_plate_crops_batch_front_end_kinds_and_counts():
    """rectify.plate_crops_batch: one launch over images of different sizes with different numbers of quads (none included); the results
    are of the images' kinds and equal the direct call's."""
    dev = _frames(3)
    imgs = [dev[0], dev[1].cpu().numpy(), dev[0].cpu()]
    quads = [QUADS, np.array(QUADS[:3], dtype=np.float32).reshape(3, 8), []]
    size = (33, 7)
    out = rectify.plate_crops_batch(imgs, quads, size=size)
    assert torch.is_tensor(out[0][0]) and out[0][0].is_cuda and isinstance(out[1][0], np.ndarray) and not out[2][0].is_cuda
    assert [tuple(o[0].shape) for o in out] == [(10, 7, 33, 3), (3, 7, 33, 3), (0, 7, 33, 3)]
    assert [o[1].dtype for o in out] == [np.dtype(bool)] * 3 and [o[1].shape for o in out] == [(10,), (3,), (0,)]
    for (crops, ok), im, qs in zip(out[:2], dev, quads[:2]):
        crops = crops.cpu().numpy() if torch.is_tensor(crops) else crops
        for j, q in enumerate(np.asarray(qs, dtype=np.float64).reshape(-1, 8)):
            M = _host_matrix(q, size)
            assert ok[j] == (M is not None)
            want = rectify.warp_perspective(im, M, size).cpu().numpy() if M is not None else np.zeros((7, 33, 3), np.uint8)
            assert np.array_equal(crops[j], want), j


def _net(kind, dtype):
    net = getattr(D, kind)(synth.vgg19_standin(seed=0))
    synth.fill_params_(net, 11)
    net = net.cuda().eval()
    net.compute_dtype = dtype
    return net


def _np(x):
    return x.cpu().numpy() if torch.is_tensor(x) else x


def _check_crops(res, ref, frames, size):
    """res is detect_batch's ref plus, per kept row, the host solve and the single-plate warp (or zeros and False); the number of ok crops"""
    ow, oh = size
    assert len(res) == len(ref) == len(frames)
    n = 0
    for (d, keep, crops, ok), (d0, keep0), f in zip(res, ref, frames):
        assert d.dtype == d0.dtype and np.array_equal(_bits(d), _bits(d0)) and keep == keep0
        assert isinstance(ok, np.ndarray) and ok.dtype == np.bool_ and ok.shape == (len(keep),)
        crops = _np(crops)
        assert crops.shape == (len(keep), oh, ow, 3) and crops.dtype == np.uint8
        for j, k in enumerate(keep):
            M = _host_matrix(d[k, 5:13], size)
            assert ok[j] == (M is not None), (k, j)
            if M is None:
                assert not crops[j].any(), (k, j)
                continue
            n += 1
            assert np.array_equal(crops[j], rectify.warp_perspective(_np(f), M, size)), (k, j)
    return n


@pytest.mark.parametrize('kind', ['DenseBoxLM', 'DenseBoxLMLOC'])
@pytest.mark.parametrize('dtype', ['f32', 'f16'])
def test_detect_plate_crops_is_detect_batch_plus_the_host_composition(kind, dtype):
    net = _net(kind, dtype)
    size = (94, 24)
    rs = np.random.RandomState(5)
    x = torch.from_numpy(rs.randint(0, 256, size=(3, 240, 240, 3)).astype(np.uint8))
    ref = net.detect_batch(x.cuda(), K=10)
    res = net.detect_plate_crops(x, size=size, K=10)                                    # a CPU tensor in -> CPU tensors out
    checked = [_check_crops(res, ref, [x[b] for b in range(3)], size)]
    assert all(torch.is_tensor(c) and not c.is_cuda for _, _, c, _ in res)
    mixed = [rs.randint(0, 256, size=s).astype(np.uint8) for s in ((240, 240, 3), (160, 208, 3), (240, 240, 3))]
    ref = net.detect_batch([torch.from_numpy(m) for m in mixed], K=10, max_batch=1)
    res = net.detect_plate_crops([torch.from_numpy(m).cuda() for m in mixed], size=size, K=10, max_batch=1)
    checked.append(_check_crops(res, ref, mixed, size))
    assert all(torch.is_tensor(c) and c.is_cuda for _, _, c, _ in res)
    frames = [x[b].numpy() for b in range(3)]
    res = net.detect_plate_crops(frames, size=size, K=10)                               # numpy in -> numpy out
    checked.append(_check_crops(res, net.detect_batch(x.cuda(), K=10), frames, size))
    assert all(isinstance(c, np.ndarray) for _, _, c, _ in res)
    assert sum(checked) > 0, checked


def _snapshot(res):
    return [(d.copy(), list(keep), _np(c).copy(), ok.copy()) for d, keep, c, ok in res]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(_bits(d), _bits(d0)) and keep == keep0 and np.array_equal(_np(c), _np(c0))
                                    and np.array_equal(ok, ok0) for (d, keep, c, ok), (d0, keep0, c0, ok0) in zip(a, b))


@pytest.mark.parametrize('where', ['cuda', 'cpu'])
def test_graph_path_one_entry_per_shape_and_size_and_results_own_their_memory(where, monkeypatch):
    monkeypatch.delenv('DBX_GRAPH', raising=False)
    net = _net('DenseBoxLMLOC', 'f16')
    rs = np.random.RandomState(5)
    a, b = (torch.from_numpy(rs.randint(0, 256, size=(2, 240, 240, 3)).astype(np.uint8)).to(where) for _ in range(2))
    size = (94, 24)
    assert not net.__dict__.get('_detect_graphs')
    r1 = net.detect_plate_crops(a, size=size)
    snap = _snapshot(r1)
    r2 = net.detect_plate_crops(b, size=size)
    cache = net._detect_graphs
    assert len(cache) == 1 and next(iter(cache))[0] == 'plate_crops', list(cache)
    assert _same(r1, snap), 'the second call changed what the first returned'
    assert not _same(r1, r2)
    assert all((c.is_cuda if where == 'cuda' else not c.is_cuda) for _, _, c, _ in r1 + r2)
    assert sum(int(ok.sum()) for _, _, _, ok in r1 + r2) > 0
    monkeypatch.setenv('DBX_GRAPH', '0')
    assert _same(net.detect_plate_crops(a, size=size), r1) and _same(net.detect_plate_crops(b, size=size), r2)
    assert len(cache) == 1
    monkeypatch.delenv('DBX_GRAPH')
    r3 = net.detect_plate_crops(a, size=(33, 7))
    assert len(cache) == 2 and [k[0] for k in cache] == ['plate_crops'] * 2, list(cache)
    assert _same(r1, snap) and tuple(r3[0][2].shape[1:]) == (7, 33, 3)
    net.train()
    net.detect_plate_crops(a, size=size)
    assert len(cache) == 2
