"""CPU-side checks of the batched pad + bicubic resize: the NumPy restatement tests/cubic_ref.py (the oracle of the GPU tests) is
pinned against torch's CPU bicubic interpolation; pad_img / pad_geometry; dbx_resize_cubic_batch_u8 refuses every bad argument on the
host, with an error code and a message naming the entry point, before anything is launched; the Python argument checks."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cubic_ref as R                                   # noqa: E402

from densebox_amd import _lib, resize                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _noise(seed, h, w, c=None, stripes=False):
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, size=(h, w) if c is None else (h, w, c)).astype(np.uint8)
    if stripes:                                          # rows of 0 and columns of 255: over- and undershoot saturate
        img[::7] = 0
        img[:, ::11] = 255
    return img


def _torch_bicubic(img, dh, dw):
    """torch's CPU bicubic (A = -0.75, the same sample positions, clamped indices) in float64, clamped to 0..255 and rounded half up."""
    x = torch.from_numpy(np.ascontiguousarray(img if img.ndim == 3 else img[:, :, None])).permute(2, 0, 1)[None].double()
    y = torch.nn.functional.interpolate(x, size=(dh, dw), mode='bicubic', align_corners=False)[0].permute(1, 2, 0).numpy()
    y = np.floor(np.clip(y, 0.0, 255.0) + 0.5).astype(np.int64)
    return y if img.ndim == 3 else y[:, :, 0]


# (source h, w, channels or None, destination h, w, stripes): up- and down-scaling, non-uniform scaling, tiny sources
TORCH_CASES = [
    (37, 53, 3, 64, 64, False), (480, 640, 3, 720, 720, True), (1080, 1080, None, 512, 512, True), (97, 97, 1, 240, 240, False),
    (1200, 1200, None, 512, 512, True), (1, 1, 3, 8, 8, False), (2, 3, 4, 9, 9, False), (300, 300, 3, 240, 240, False),
    (200, 331, 3, 77, 501, True), (331, 200, None, 501, 77, True), (5, 400, 1, 40, 50, False), (64, 48, 3, 17, 131, False),
]


@pytest.mark.parametrize('case', TORCH_CASES, ids=lambda c: '%dx%dx%s-%dx%d' % c[:5])
def test_restatement_is_within_one_grey_level_of_torch_bicubic(case):
    """Each 11-bit coefficient is off by at most 2^-12; the horizontal pass is then off by at most 255 * 4 * 2^-12 = 0.25, which the
    vertical pass (absolute weight at most 1.375) carries as 0.34 and to which it adds 255 * 1.375 * 4 * 2^-12 = 0.34 of its own: under
    0.7 grey levels before rounding, and two roundings of values less than 1 apart differ by at most 1."""
    sh, sw, c, dh, dw, stripes = case
    img = _noise(sh * 1000 + sw, sh, sw, c, stripes)
    got = R.resize_cubic_u8(img, dh, dw)
    assert got.dtype == np.uint8 and got.shape == ((dh, dw) if c is None else (dh, dw, c))
    diff = np.abs(got.astype(np.int64) - _torch_bicubic(img, dh, dw))
    print('%s: worst difference %d, %.2f %% of the pixels differ' % (case, diff.max(), 100.0 * (diff > 0).mean()))
    assert diff.max() <= 1


def test_restatement_exact_fractions_match_torch_everywhere():
    """300 -> 240: scale 1.25, every fraction a multiple of 1/4, every coefficient exact in 11 bits."""
    img = _noise(1, 300, 300, 3)
    assert np.array_equal(R.resize_cubic_u8(img, 240, 240).astype(np.int64), _torch_bicubic(img, 240, 240))


@pytest.mark.parametrize('shape', [(720, 720, 3), (33, 57), (1, 1, 4), (2, 5, 1)])
def test_restatement_identity_size_returns_the_source(shape):
    img = _noise(2, *shape[:2], shape[2] if len(shape) == 3 else None, stripes=shape[0] > 8)
    s, a = R.cubic_taps(shape[1], shape[1])
    assert np.array_equal(s + 1, np.arange(shape[1])) and np.array_equal(a, np.tile([0, 2048, 0, 0], (shape[1], 1)))
    assert np.array_equal(R.resize_cubic_u8(img, shape[0], shape[1]), img)


def test_restatement_constant_image_stays_within_one_grey_level():
    """The four integer coefficients of a pixel sum to 2047..2049, not always 2048, and 255 * 2049^2 / 2^22 = 255.25."""
    sums = set()
    for n_src, n_dst in [(37, 64), (1920, 720), (1080, 512), (97, 240), (3, 200), (1000, 7), (240, 241)]:
        sums |= set(R.cubic_taps(n_src, n_dst)[1].sum(axis=1).tolist())
        for v in (0, 1, 127, 128, 254, 255):
            out = R.resize_cubic_u8(np.full((n_src, 31, 3), v, np.uint8), n_dst, 45).astype(np.int64)
            assert np.abs(out - v).max() <= 1, (n_src, n_dst, v)
    assert sums <= {2047, 2048, 2049} and 2048 in sums, sums


def test_restatement_virtual_source_is_np_pad_of_the_crop():
    img = _noise(3, 20, 30, 3)
    v = R.virtual_source(img, (4, 5, 10, 7), (1, 2, 3, 4), 128)
    assert v.shape == (7 + 2 + 4, 10 + 1 + 3, 3)
    assert np.array_equal(v[2:9, 1:11], img[5:12, 4:14]) and (v[:2] == 128).all() and (v[:, 11:] == 128).all()
    assert np.array_equal(R.virtual_source(img), img)
    assert R.pad_square(img).shape == (30, 30, 3) and np.array_equal(R.pad_square(img)[5:25], img)


@pytest.mark.parametrize('shape', [(20, 31), (20, 30), (31, 20), (30, 20), (25, 25), (1, 6), (7, 2),
                                   (20, 31, 3), (20, 30, 3), (31, 20, 3), (30, 20, 3), (25, 25, 3)])
def test_pad_img_and_pad_geometry(shape):
    img = _noise(4, *shape[:2], shape[2] if len(shape) == 3 else None)
    h, w = shape[:2]
    diff = abs(h - w)
    lu, rd = diff // 2, diff - diff // 2
    widths = (((lu, rd), (0, 0)) if h <= w else ((0, 0), (lu, rd))) + (((0, 0),) if len(shape) == 3 else ())
    want = np.pad(img, widths, 'constant', constant_values=128)
    got = resize.pad_img(img)
    assert got.dtype == np.uint8 and np.array_equal(got, want) and got.shape[0] == got.shape[1] == max(h, w)
    side, px, py = resize.pad_geometry(h, w)
    assert (side, px, py) == (max(h, w), 0 if h <= w else lu, lu if h <= w else 0)
    assert np.array_equal(got[py:py + h, px:px + w], img)
    assert np.array_equal(R.pad_square(img), want)


def test_pad_img_refuses_what_the_reference_does_not_handle():
    with pytest.raises(RuntimeError, match='pad_img'):
        resize.pad_img(torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='pad_img'):
        resize.pad_img(np.zeros((4, 4, 4), np.uint8))


# ------------------------------------------------------------------------------------------------------------------- C ABI
def _job(**kw):
    j = _lib.ResizeJob()
    j.src, j.sh, j.sw = 0x1000, 120, 200
    j.cx0, j.cy0, j.cw, j.ch = 0, 0, 200, 120
    j.pad_l, j.pad_t, j.pad_r, j.pad_b, j.pad_value = 0, 40, 0, 40, 128
    j.dh, j.dw, j.dst_off = 64, 64, 0
    for k, v in kw.items():
        setattr(j, k, v)
    return j


def _call(L, jobs, njobs=None, c=3, dst=0x2000, ws=0x3000):
    arr = (_lib.ResizeJob * max(1, len(jobs)))(*jobs)
    vp = lambda a: None if a is None else C.c_void_p(a)       # noqa: E731
    return L.dbx_resize_cubic_batch_u8(arr, len(jobs) if njobs is None else njobs, c, vp(dst), vp(ws), None)


@pytest.mark.parametrize('bad', [
    dict(njobs=-1), dict(c=0), dict(c=5), dict(dst=None), dict(ws=None),
    dict(job=dict(src=None)),
    dict(job=dict(sh=0)), dict(job=dict(sw=-2)), dict(job=dict(cw=0)), dict(job=dict(ch=-1)), dict(job=dict(dh=0)), dict(job=dict(dw=-3)),
    dict(job=dict(cx0=-1, cw=10)), dict(job=dict(cy0=-1, ch=10)), dict(job=dict(cx0=1)), dict(job=dict(cy0=111, ch=10)),
    dict(job=dict(cx0=190, cw=11)), dict(job=dict(cw=201)), dict(job=dict(ch=121)),
    dict(job=dict(pad_l=-1)), dict(job=dict(pad_t=-1)), dict(job=dict(pad_r=-1)), dict(job=dict(pad_b=-40)),
    dict(job=dict(pad_value=-1)), dict(job=dict(pad_value=256)), dict(job=dict(dst_off=-16)),
    dict(job=dict(sh=30000, sw=30000)), dict(job=dict(pad_l=2 ** 30)),
])
def test_resize_batch_rejects_bad_arguments_without_touching_the_gpu(bad):
    L = _lib.lib()
    bad = dict(bad)
    jobs = [_job(), _job(**bad.pop('job', {}))]
    rc = _call(L, jobs, **bad)
    assert rc == -1, bad
    msg = L.dbx_last_error()
    assert b'resize_cubic_batch' in msg, msg
    with pytest.raises(RuntimeError, match='resize_cubic_batch'):
        _lib.check(rc)


def test_resize_batch_null_job_list_and_empty_call():
    L = _lib.lib()
    assert L.dbx_resize_cubic_batch_u8(None, 1, 3, C.c_void_p(0x2000), C.c_void_p(0x3000), None) == -1
    assert b'resize_cubic_batch' in L.dbx_last_error()
    assert _call(L, [_job()], njobs=0) == 0                              # njobs == 0: a no-op that launches nothing
    assert L.dbx_resize_cubic_batch_u8(None, 0, 3, None, None, None) == 0


def test_resize_batch_workspace_grows_with_the_job_count():
    L = _lib.lib()
    sizes = [L.dbx_resize_batch_workspace_bytes(n) for n in (0, 1, 2, 10, 100, 320, 10000)]
    assert all(s > 0 and s % 256 == 0 for s in sizes), sizes
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] < sizes[3] < sizes[4] < sizes[5] < sizes[6], sizes
    assert L.dbx_resize_batch_workspace_bytes(-1) < 0


def test_resize_job_struct_layout_matches_the_header():
    """The offsets the header documents, read from its comment, against ctypes' layout of the binding."""
    src = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    m = re.search(r'Layout \((\d+) bytes\):(.*?)\*/\s*typedef struct dbx_resize_job', src, re.S)
    assert m, 'the header does not document the layout of dbx_resize_job'
    assert C.sizeof(_lib.ResizeJob) == int(m.group(1)) == 72
    doc = {n: int(o) for n, o in re.findall(r'\b([a-z_0-9]+) (\d+)\b', m.group(2).replace('\n *', ' '))}
    got = {n: getattr(_lib.ResizeJob, n).offset for n, _ in _lib.ResizeJob._fields_}
    assert doc == got, (doc, got)
    assert got['src'] == 0 and got['pad_value'] == 48 and got['dw'] == 56 and got['dst_off'] == 64
    fields = re.search(r'typedef struct dbx_resize_job \{(.*?)\} dbx_resize_job;', src, re.S).group(1)
    names = re.findall(r'\b(\w+)\s*[,;]', re.sub(r'/\*.*?\*/', '', fields))
    assert names == [n for n, _ in _lib.ResizeJob._fields_], names


def test_integration_doc_shows_the_resize_job_struct():
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    m = re.search(r'class ResizeJob\(C\.Structure\):.*?_fields_ = \[(.*?)\]\n', doc, re.S)
    assert m, 'INTEGRATION.md does not show ResizeJob'
    names = re.findall(r"\('(\w+)', C\.(\w+)\)", m.group(1))
    assert [n for n, _ in names] == [f[0] for f in _lib.ResizeJob._fields_], names
    assert [getattr(C, t) for _, t in names] == [f[1] for f in _lib.ResizeJob._fields_], names


# ------------------------------------------------------------------------------------------------- Python argument checks
def test_pad_resize_batch_argument_checks():
    img = np.zeros((20, 30, 3), np.uint8)
    with pytest.raises(RuntimeError, match='uint8'):
        resize.pad_resize_batch([img.astype(np.float32)])
    with pytest.raises(RuntimeError, match='uint8'):
        resize.pad_resize_batch(torch.zeros(2, 3, 20, 30))
    with pytest.raises(RuntimeError, match='channels'):
        resize.pad_resize_batch([img, np.zeros((20, 30, 1), np.uint8)])
    with pytest.raises(RuntimeError, match='channels'):
        resize.pad_resize_batch([np.zeros((20, 30, 5), np.uint8)])
    with pytest.raises(RuntimeError, match='no images'):
        resize.pad_resize_batch([])
    for size in (0, -8, 7.5, (64, 64)):
        with pytest.raises(RuntimeError, match='size'):
            resize.pad_resize_batch([img], size=size)


def test_crop_resize_batch_argument_checks():
    img = np.zeros((20, 30, 3), np.uint8)
    with pytest.raises(RuntimeError, match='uint8'):
        resize.crop_resize_batch([img.astype(np.float32)], [[(0, 0, 5, 5)]])
    with pytest.raises(RuntimeError, match='channels'):
        resize.crop_resize_batch([img, np.zeros((20, 30, 4), np.uint8)], [[(0, 0, 5, 5)], []])
    with pytest.raises(RuntimeError, match='2 lists of windows for 1 images'):
        resize.crop_resize_batch([img], [[(0, 0, 5, 5)], []])
    with pytest.raises(RuntimeError, match='lists of windows'):
        resize.crop_resize_batch(torch.zeros(3, 20, 30, 3, dtype=torch.uint8), [[(0, 0, 5, 5)]])
    for win in ((5, 5, 5, 9), (8, 3, 2, 9), (40, 0, 50, 9), (0, 25, 9, 30), (0, -3, 9, -3)):
        with pytest.raises(RuntimeError, match=r'window .* of image 1 \(20 x 30\) is an empty slice'):
            resize.crop_resize_batch([img, img], [[(0, 0, 5, 5)], [(1, 1, 9, 9), win]])
    with pytest.raises(RuntimeError, match='4 integers'):
        resize.crop_resize_batch([img], [[(0, 0, 5.5, 5)]])
    with pytest.raises(RuntimeError, match='4 integers'):
        resize.crop_resize_batch([img], [[(0, 0, 5)]])
    with pytest.raises(RuntimeError, match='size'):
        resize.crop_resize_batch([img], [[(0, 0, 5, 5)]], size=(0, 240))
    with pytest.raises(RuntimeError, match='no windows'):
        resize.crop_resize_batch([img], [[]])


def test_detect_batch_resized_python_argument_checks():
    """Float frames, a size that is not a positive multiple of 4 and a wrong channel count are refused before any device work."""
    import densebox_amd as D
    from densebox_amd import decode as DC, synth
    net = D.DenseBoxLMLOC(synth.vgg19_standin(seed=0)).eval()
    frames = [np.zeros((48, 64, 3), np.uint8), np.zeros((64, 40, 3), np.uint8)]
    for size in (0, -4, 6, 718, 720.0, (720, 720)):
        with pytest.raises(RuntimeError, match='detect_batch_resized: size'):
            net.detect_batch_resized(frames, size=size)
    with pytest.raises(RuntimeError, match='uint8'):
        net.detect_batch_resized(torch.zeros(2, 3, 64, 64))
    with pytest.raises(RuntimeError, match='uint8'):
        DC.detect_batch_resized(net, [torch.zeros(64, 64, 3)])
    with pytest.raises(RuntimeError, match='channels'):
        net.detect_batch_resized(torch.zeros(2, 64, 64, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='no images'):
        net.detect_batch_resized([])
