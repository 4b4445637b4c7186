"""Every up-sampling, pooling and layout kernel of csrc/aux_ops.hip against the NumPy float64 reference of tests/aux_ref.py, whole buffers.

Kernels and the cases that pin them (backward paths asserted through dbx_upsample_bilinear_bwd_plan, the library's own read-only query,
and against its restatement aux_ref.plan_ref; a case that no longer selects its path fails with the computed plan in the message):
  upsample_bwd_walk_kernel   walk-dyadic-1seg (odd row count: the single-row last pair; 10 workgroups, no multiple of 8: the XCD remap),
                             walk-dyadic-segs (3 segments, seams at source columns 8 / 16, 9 workgroups), walk-rounds2 (320 channel
                             groups: a second round on 64 of 256 threads), walk-7rows (7 of MAXR 8 rows in a pair), walk-workload
                             (30 <- 60, the training geometry)
  upsample_bwd_rows_kernel   rows-below-walk (63 groups: one short of the walk; more than 256 items per row), rows-identity, rows-3/8
                             (weights in eighths), rows-widest (5 <- 12: the 6-wide window, 36 terms), rows-2x-small-c, flat-down
                             (down-sampling by 2 -- both scales 2 > 0.34, so the dispatcher gives it to this kernel: the sources that
                             receive no term must be written 0, not left at 7)
  upsample_bwd_kernel        flat-quarter, flat-mixed (sy 1/2 but sx 1/4: the && of both conditions), flat-down-y (down-sampling in y
                             under sx 1/4: rows without a term on the flat kernel proper), flat-degenerate-out1 / -in1 (scale 0 both
                             ways), flat-third (0.333 < 0.34)
  upsample_rows_kernel       y.w x cg = 7 (a partial round), 1024 (exactly one trip), 1320 (a second trip with clamped loads), the
                             training call's view(0, 512) of a 768-wide frame; 9 -> 17, identity, 4x7 -> 9x17, 15 -> 30, 5 -> 12, 9 -> 5,
                             in = 1, out = 1
  upsample_nchw_f32_kernel   bit for bit against the float32 restatement
  maxpool_kernel (with and without idx), maxpool_bwd_kernel, maxpool_bwd_idx_kernel   12x20, 15x9, 6x7, 1x1 (no window at all), maps in
                             halves (ties, all-zero windows), accumulate x gate, the idx bytes from 0xAB with an intact tail, views
  u8hwc_to_framed_kernel, nchw_to_framed_kernel, nchw_to_framed_ch_kernel, framed_add_ch_kernel, framed_to_nchw_kernel

Per case: every buffer between guard bands (tests/framed_buf.py), inputs with halos of 200 .. 500 and, in the view variants, 1000 in
the channels outside the view; outputs starting at 7 everywhere; the WHOLE buffer compared -- halo, guards and foreign channels
included -- inputs unchanged, and a second call into fresh buffers bitwise equal.  Operands are integers in {-2 .. 2}, gates in
{-1, 0, 1}, pooled maps in halves.  Exact cases (aux_ref.assert_exact_premise) must give round_T(reference) bit for bit; the others
must lie in [round_T(ref - E), round_T(ref + E)] (fp32: within E + ulp / 2) with E = K 2**-24 sum |terms| and the K aux_ref derives
per kernel: 13 on walk-7rows and walk-workload, 39 on rows-widest, 19 on rows-2x-small-c, 28 on flat-third, 8 forward.  The share of
outputs whose interval holds more than one value (from the reference: tests/test_aux_ref.py caps it at 2.5 % / 10 %) is at most
1.50 % in bf16 and 7.42 % in f16; aux_ref's docstring has the table.  The 2**32 guard of the walk is asserted on the host only
(tests/test_aux_ref.py): a map that large needs more than 8 GB.

Cost.  References are NumPy on the CPU, one per case, shared by the dtypes.  On an MI355X host the 328 tests of this file took 3.3 s in
all, references included; the slowest five: walk-dyadic-1seg-bf16-nogate 0.43 s (the first call of the process: the library and the
device come up), walk-7rows-bf16-gate 0.05 s, walk-workload-f16-gate 0.05 s, walk-workload-bf16-nogate 0.05 s, walk-workload-bf16-gate
0.03 s.  tests/test_aux_ref.py (CPU, 187 tests) takes 9 s, of which the table sweep over the sizes 2 .. 259 is 4 s."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aux_ref as A                                     # noqa: E402
from framed_buf import Buf, assert_holds                # noqa: E402

from densebox_amd import _lib                           # noqa: E402
from densebox_amd._lib import check, stream_ptr         # noqa: E402

pytestmark = pytest.mark.gpu

TDT = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}
DTNS = ('bf16', 'f16', 'f32')
SENTINEL, FILL, TAIL = 1000.0, 7.0, 256                     # 1000 and 7 are exact in bf16, f16 and fp32
HALO = dict(dy=300.0, gate=500.0, x=200.0)                  # what an input's halo and guards hold: a kernel that read them would show
KERNEL = {A.FLAT: 'upsample_bwd_kernel', A.ROWS: 'upsample_bwd_rows_kernel', A.WALK: 'upsample_bwd_walk_kernel'}


def f64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def framed(name, dtn, n, h, w, pad, c, fill, data=None, c_off=0, ld=None):
    """A Buf whose view is channels [c_off, c_off + c) of a frame of ld channels: the view holds `data` (default: fill), the other
    channels of the pixels 1000."""
    ld = ld or c
    interior = np.full((n, h, w, ld), SENTINEL if ld != c else fill)
    interior[..., c_off:c_off + c] = fill if data is None else data
    b = Buf(name, n, h, w, pad, ld, TDT[dtn], fill, interior)
    b.c, b.c_off = c, c_off
    return b.upload()


def vw(b):
    return b.view(c=b.c, c_off=b.c_off)


def geo(b):
    n, h, w = b.shape
    return A.Geo(n, h, w, b.pad, b.ld, b.c)


def check_output(b, lo, hi, what):
    """The whole buffer: [lo, hi] (float64, [n][h][w][c]) inside the view, what it was created with everywhere else."""
    assert_holds(b, lo=f64(b.host_with_interior(lo, b.c_off)), hi=f64(b.host_with_interior(hi, b.c_off)), what=what)


# ---------------------------------------------------------------------------------------------------------------- backward up-sampling
def query(dtn, dy, dx):
    out = _lib.UpsampleBwdPlan()
    check(_lib.lib().dbx_upsample_bilinear_bwd_plan(_lib.DTYPE_ID[dtn], C.byref(vw(dy)), C.byref(vw(dx)), C.byref(out)))
    return A.Plan(out.kernel, out.nseg, out.workgroups, out.lds_bytes)


def run_bwd(case, dtn, gated, content='dense', views=False):
    L, dt = _lib.lib(), _lib.DTYPE_ID[dtn]
    m = A.make_bwd(case, content)
    c = case.cg * A.VEC[dtn]
    n, h, w, hs, ws = case.n, case.h, case.w, case.hs, case.ws
    if case.exact:
        A.assert_exact_premise(h, w, hs, ws, m['ref'], m['ref_abs'])
    lo, hi, _ = A.bwd_bounds(case, m, dtn, gated)
    # views: dy a slice at channel 64 of a pad-0 frame, dx a slice at 16 of a pad-1 frame, the gate a slice at 8 of a pad-2 frame
    fr = dict(dy=(0, 64, c + 96), dx=(1, 16, c + 48), gate=(2, 8, c + 24)) if views else dict(dy=(0, 0, c), dx=(1, 0, c), gate=(1, 0, c))

    def inputs():
        dy = framed('dy', dtn, n, h, w, fr['dy'][0], c, HALO['dy'], m['dy'][..., :c], *fr['dy'][1:])
        gate = framed('gate', dtn, n, hs, ws, fr['gate'][0], c, HALO['gate'], m['gate'][..., :c], *fr['gate'][1:]) if gated else None
        return dy, gate

    def call(dy, gate):
        dx = framed('dx', dtn, n, hs, ws, fr['dx'][0], c, FILL, None, *fr['dx'][1:])
        check(L.dbx_upsample_bilinear_bwd(dt, C.byref(vw(dy)), C.byref(vw(dx)), C.byref(vw(gate)) if gate else None, stream_ptr()))
        torch.cuda.synchronize()
        return dx

    dy, gate = inputs()
    dx = framed('dx', dtn, n, hs, ws, fr['dx'][0], c, FILL, None, *fr['dx'][1:])
    plan = query(dtn, dy, dx)
    want = A.plan_ref(dtn, geo(dy), geo(dx))
    assert plan == want and (plan.kernel, plan.nseg) == (case.path, case.nseg), \
        '%s %s: the library plans %s (%r), plan_ref %r, the case is there for %s with nseg %d' % (
            case.name, dtn, KERNEL[plan.kernel], plan, want, KERNEL[case.path], case.nseg)
    what = '%s %s %s [%s nseg %d, %d workgroups]' % (case.name, dtn, content, KERNEL[plan.kernel], plan.nseg, plan.workgroups)
    print(what)                                             # (pytest -s / -rP: which kernel every case ran)
    dx = call(dy, gate)
    for b in [dy] + ([gate] if gate else []):
        assert_holds(b, what=what + ': input')
    check_output(dx, lo, hi, what)
    dy2, gate2 = inputs()
    dx2 = call(dy2, gate2)
    check_output(dx2, lo, hi, what + ' (second call)')
    assert torch.equal(dx.dev.view(torch.uint8), dx2.dev.view(torch.uint8)), what + ': the second call differs from the first'
    return plan


@pytest.mark.parametrize('gated', [False, True], ids=['nogate', 'gate'])
@pytest.mark.parametrize('dtn', DTNS)
@pytest.mark.parametrize('name', list(A.BWD))
def test_upsample_backward(name, dtn, gated):
    run_bwd(A.BWD[name], dtn, gated)


@pytest.mark.parametrize('gated', [False, True], ids=['nogate', 'gate'])
@pytest.mark.parametrize('dtn', DTNS)
@pytest.mark.parametrize('name', A.VARIANTS)
def test_upsample_backward_on_channel_slices_of_wider_frames(name, dtn, gated):
    """dy at c_off 64 of a pad-0 frame, dx at c_off 16 of a pad-1 frame, the gate at c_off 8 of a pad-2 frame of a third width: the
    channels outside the views hold 1000 and must stay."""
    run_bwd(A.BWD[name], dtn, gated, views=True)


@pytest.mark.parametrize('dtn', DTNS)
@pytest.mark.parametrize('name', A.VARIANTS)
def test_upsample_backward_impulses(name, dtn):
    """Single ones in dy at the corners of the first and last image, either side of every segment seam, in the last column and the last
    row: a failure names the pixel, and with it the coefficient."""
    run_bwd(A.BWD[name], dtn, False, content='impulse')


# ---------------------------------------------------------------------------------------------------------------- forward up-sampling
def run_fwd(case, dtn, wide=False):
    L, dt = _lib.lib(), _lib.DTYPE_ID[dtn]
    m = A.make_fwd(case)
    c = case.cg * A.VEC[dtn]
    if case.exact:
        A.assert_exact_premise(case.ho, case.wo, case.hi, case.wi, m['ref'], m['ref_abs'])
    lo, hi, _ = A.fwd_bounds(case, m, dtn)
    what = '%s %s%s' % (case.name, dtn, ' into view(0, %d) of %d channels' % (c, c * 3 // 2) if wide else '')

    def call():
        x = framed('x', dtn, case.n, case.hi, case.wi, 1, c, HALO['x'], m['x'][..., :c])
        y = framed('y', dtn, case.n, case.ho, case.wo, 1, c, FILL, None, 0, c * 3 // 2 if wide else c)
        check(L.dbx_upsample_bilinear(dt, C.byref(vw(x)), C.byref(vw(y)), stream_ptr()))
        torch.cuda.synchronize()
        assert_holds(x, what=what + ': input')
        check_output(y, lo, hi, what)
        return y
    y, y2 = call(), call()
    assert torch.equal(y.dev.view(torch.uint8), y2.dev.view(torch.uint8)), what + ': the second call differs from the first'


@pytest.mark.parametrize('dtn', DTNS)
@pytest.mark.parametrize('name', list(A.FWD))
def test_upsample_forward(name, dtn):
    case = A.FWD[name]
    items = case.wo * case.cg
    assert {'fwd-identity-7': 7, 'fwd-identity-1024': 1024, 'fwd-2x-1320': 1320}.get(name, items) == items
    run_fwd(case, dtn)


@pytest.mark.parametrize('dtn', DTNS)
def test_upsample_forward_into_the_fusion_frame_slice(dtn):
    """The training forward's call: dbx_upsample_bilinear(a44.view(), fusion.view(0, 512)), two thirds of a frame whose other channels
    (here 1000) belong to another tensor."""
    assert A.FWD['fwd-dyadic'].cg * 8 == 512
    run_fwd(A.FWD['fwd-dyadic'], dtn, wide=True)


GUARD = 64


def guarded_f32(a):
    """A float32 device array between two bands of 7: (tensor, pointer to the array)."""
    t = torch.full((a.size + 2 * GUARD,), FILL, dtype=torch.float32)
    t[GUARD:GUARD + a.size] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).flatten()
    t = t.cuda()
    return t, C.c_void_p(t.data_ptr() + 4 * GUARD)


def assert_f32(t, want, what):
    """Bit for bit, guards included."""
    exp = torch.full((want.size + 2 * GUARD,), FILL, dtype=torch.float32)
    exp[GUARD:GUARD + want.size] = torch.from_numpy(np.ascontiguousarray(want, dtype=np.float32)).flatten()
    got = t.cpu()
    bad = got.view(torch.int32) != exp.view(torch.int32)
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0, 0])
        raise AssertionError('%s: %d of %d floats differ, the first at flat index %d (array at [%d, %d)): got %r, want %r' % (
            what, int(bad.sum()), got.numel(), i, GUARD, GUARD + want.size, float(got[i]), float(exp[i])))


@pytest.mark.parametrize('planes,hi,wi,ho,wo', [(2, 14, 20, 40, 52), (17, 15, 15, 31, 31), (2, 1, 1, 3, 4), (17, 5, 7, 1, 1), (2, 9, 9, 17, 17)])
def test_upsample_nchw_f32_bit_for_bit(planes, hi, wi, ho, wo):
    x = np.random.RandomState(planes * 100 + ho).standard_normal((planes, hi, wi)).astype(np.float32)
    want = A.up_nchw_f32(x, ho, wo)
    outs = []
    for _ in range(2):
        xt, xp = guarded_f32(x)
        yt, yp = guarded_f32(np.full((planes, ho, wo), FILL))
        check(_lib.lib().dbx_upsample_bilinear_nchw_f32(xp, planes, hi, wi, yp, ho, wo, stream_ptr()))
        torch.cuda.synchronize()
        assert_f32(xt, x, 'input')
        assert_f32(yt, want, 'dbx_upsample_bilinear_nchw_f32 %dx%d -> %dx%d' % (hi, wi, ho, wo))
        outs.append(yt)
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------------------- pooling
POOL_SIZES = [(12, 20), (15, 9), (6, 7), (1, 1)]
POOL_TYPES = [('bf16', 1), ('bf16', 16), ('f16', 1), ('f16', 16), ('f32', 1), ('f32', 3), ('f32', 16)]
POOL_N = 2
_POOL = {}


def pool_data(h, w):
    """x in halves, dy and the old dx in integers, 128 channels (a dtype takes the first 8 cg / 4 cg), and the reference."""
    if (h, w) not in _POOL:
        x = A.halves(h * 100 + w, (POOL_N, h, w, 128))
        y, nib = A.pool_forward(x)
        rng = np.random.RandomState(h + w)
        dy = rng.randint(-2, 3, size=y.shape).astype(np.float64)
        old = rng.randint(-3, 4, size=x.shape).astype(np.float64)
        _POOL[(h, w)] = dict(x=x, y=y, nib=nib, dy=dy, old=old)
        if h > 1:
            assert (nib == 0).any() and all(((nib & 3) == k).any() for k in range(4)) and ((nib & 4) != 0).any()      # all-zero windows, every arg
    return _POOL[(h, w)]


def idx_buffer(content=None, nbytes=0):
    t = torch.full((nbytes + TAIL,), 0xAB, dtype=torch.uint8)
    if content is not None:
        t[:nbytes] = torch.from_numpy(content)
    return t.cuda()


def pool_frames(dtn, h, w, c, views):
    """(pad, c_off, ld) of x / dx, y and dy."""
    if views:
        return dict(x=(1, 2 * A.VEC[dtn], c + 3 * A.VEC[dtn]), y=(0, A.VEC[dtn], c + 2 * A.VEC[dtn]), dy=(2, 0, c + A.VEC[dtn]))
    return dict(x=(1, 0, c), y=(1, 0, c), dy=(1, 0, c))


def run_pool_forward(h, w, dtn, cg, views=False):
    L, dt = _lib.lib(), _lib.DTYPE_ID[dtn]
    d = pool_data(h, w)
    c = cg * A.VEC[dtn]
    ph, pw = h // 2, w // 2
    fr = pool_frames(dtn, h, w, c, views)
    want = d['y'][..., :c]
    nbytes = int(L.dbx_maxpool_idx_bytes(POOL_N, h, w, c))
    assert nbytes == POOL_N * ph * pw * c // 2
    want_idx = A.pool_idx_bytes(d['nib'][..., :c])
    assert want_idx.size == nbytes
    outs = []
    for with_idx in (False, True, True):
        what = 'dbx_maxpool2x2%s %dx%d %s cg %d' % ('_idx' if with_idx else '', h, w, dtn, cg)
        x = framed('x', dtn, POOL_N, h, w, fr['x'][0], c, HALO['x'], d['x'][..., :c], *fr['x'][1:])
        y = framed('y', dtn, POOL_N, ph, pw, fr['y'][0], c, FILL, None, *fr['y'][1:])
        idx = idx_buffer(nbytes=nbytes)
        if with_idx:
            check(L.dbx_maxpool2x2_idx(dt, C.byref(vw(x)), C.byref(vw(y)), C.c_void_p(idx.data_ptr()), stream_ptr()))
        else:
            check(L.dbx_maxpool2x2(dt, C.byref(vw(x)), C.byref(vw(y)), stream_ptr()))
        torch.cuda.synchronize()
        assert_holds(x, what=what + ': input')
        check_output(y, want, want, what)
        got = idx.cpu().numpy()
        assert (got[nbytes:] == 0xAB).all(), what + ': the tail behind idx was written'
        if with_idx:
            bad = np.nonzero(got[:nbytes] != want_idx)[0]
            assert bad.size == 0, '%s: %d of %d idx bytes differ, the first at %d (pooled pixel %d, channels %d / %d): got 0x%02x, want 0x%02x' % (
                what, bad.size, nbytes, bad[0], bad[0] // (c // 2), 2 * (bad[0] % (c // 2)), 2 * (bad[0] % (c // 2)) + 1, got[bad[0]], want_idx[bad[0]])
            outs.append((y.dev.view(torch.uint8), idx))
        else:
            assert (got[:nbytes] == 0xAB).all(), what + ': idx written without being asked for'
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def run_pool_backward(h, w, dtn, cg, accumulate, gate, views=False):
    L, dt = _lib.lib(), _lib.DTYPE_ID[dtn]
    d = pool_data(h, w)
    c = cg * A.VEC[dtn]
    ph, pw = h // 2, w // 2
    fr = pool_frames(dtn, h, w, c, views)
    old = d['old'][..., :c] if accumulate else None
    want = A.pool_backward(d['nib'][..., :c], d['dy'][..., :c], h, w, old, relu_gate=bool(gate))
    if h == 1:
        assert np.array_equal(want, np.zeros_like(want) if old is None else old)                # no window: nothing but zeros arrive
    nbytes = int(L.dbx_maxpool_idx_bytes(POOL_N, h, w, c))
    want_idx = A.pool_idx_bytes(d['nib'][..., :c])
    outs = {}
    for fn in ('bwd', 'bwd_idx', 'bwd', 'bwd_idx'):
        what = 'dbx_maxpool2x2_%s %dx%d %s cg %d accumulate %d gate %d' % (fn, h, w, dtn, cg, accumulate, gate)
        x = framed('x', dtn, POOL_N, h, w, fr['x'][0], c, HALO['x'], d['x'][..., :c], *fr['x'][1:])
        dy = framed('dy', dtn, POOL_N, ph, pw, fr['dy'][0], c, HALO['dy'], d['dy'][..., :c], *fr['dy'][1:])
        # dx starts at 7 (halo, guards, and the pixels when nothing is accumulated); accumulate: the pixels hold `old`
        dx = framed('dx', dtn, POOL_N, h, w, fr['x'][0], c, FILL, old, *fr['x'][1:])
        idx = idx_buffer(want_idx, nbytes)
        if fn == 'bwd':
            check(L.dbx_maxpool2x2_bwd(dt, C.byref(vw(x)), C.byref(vw(dy)), C.byref(vw(dx)), accumulate, gate, stream_ptr()))
        else:
            check(L.dbx_maxpool2x2_bwd_idx(dt, C.c_void_p(idx.data_ptr()), C.byref(vw(dy)), C.byref(vw(dx)), accumulate, gate, stream_ptr()))
        torch.cuda.synchronize()
        for b in (x, dy):
            assert_holds(b, what=what + ': input')
        got = idx.cpu().numpy()
        assert (got[:nbytes] == want_idx).all() and (got[nbytes:] == 0xAB).all(), what + ': idx changed'
        check_output(dx, want, want, what)
        outs.setdefault(fn, []).append(dx.dev.view(torch.uint8))
    assert all(torch.equal(a, b) for a, b in outs.values())


@pytest.mark.parametrize('dtn,cg', POOL_TYPES)
@pytest.mark.parametrize('h,w', POOL_SIZES)
def test_maxpool_forward(h, w, dtn, cg):
    run_pool_forward(h, w, dtn, cg)


@pytest.mark.parametrize('accumulate,gate', [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize('dtn,cg', POOL_TYPES)
@pytest.mark.parametrize('h,w', POOL_SIZES)
def test_maxpool_backward(h, w, dtn, cg, accumulate, gate):
    run_pool_backward(h, w, dtn, cg, accumulate, gate)


@pytest.mark.parametrize('dtn', DTNS)
def test_maxpool_on_channel_slices_with_differing_pads(dtn):
    """x and dx: the third group of a pad-1 frame; y: the second group of a pad-0 frame; dy: the first group of a pad-2 frame.  The other
    channels hold 1000 and must stay."""
    run_pool_forward(15, 9, dtn, 2, views=True)
    for accumulate, gate in ((0, 1), (1, 0)):
        run_pool_backward(15, 9, dtn, 2, accumulate, gate, views=True)


# ---------------------------------------------------------------------------------------------------------------- layout
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def dev_f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


@pytest.mark.parametrize('dtn,c', [('bf16', 8), ('bf16', 16), ('f16', 8), ('f16', 16), ('f32', 8), ('f32', 4)])
def test_u8hwc_to_framed_every_byte_value(dtn, c):
    """All 256 values in each of the three channels (their mean and std differ), two images, bit for bit; channels 3 and up zero."""
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    img = np.stack([np.stack([v, v.T, v[::-1]], axis=-1), np.stack([v[::-1], v, v.T], axis=-1)])
    assert img.shape == (2, 16, 16, 3) and all(len(np.unique(img[i, ..., ch])) == 256 for i in range(2) for ch in range(3))
    want = np.zeros((2, 16, 16, c))
    want[..., :3] = A.u8hwc(img, MEAN, STD, dtn)
    src = torch.cat([torch.full((64,), 0xAB, dtype=torch.uint8), torch.from_numpy(img).flatten(), torch.full((64,), 0xAB, dtype=torch.uint8)]).cuda()
    keep = src.clone()
    outs = []
    for _ in range(2):
        y = framed('y', dtn, 2, 16, 16, 1, c, FILL, None, 0, c + 2 * A.VEC[dtn])
        check(_lib.lib().dbx_u8hwc_to_framed(_lib.DTYPE_ID[dtn], C.c_void_p(src.data_ptr() + 64), C.byref(vw(y)), (C.c_float * 3)(*MEAN),
                                             (C.c_float * 3)(*STD), stream_ptr()))
        torch.cuda.synchronize()
        check_output(y, want, want, 'dbx_u8hwc_to_framed %s into %d channels' % (dtn, c))
        outs.append(y.dev.view(torch.uint8))
    assert torch.equal(src, keep) and torch.equal(outs[0], outs[1])


@pytest.mark.parametrize('sliced', [False, True], ids=['full', 'slice'])
@pytest.mark.parametrize('dtn', DTNS)
def test_nchw_to_framed_zero_fills_past_c_src(dtn, sliced):
    n, cs, h, w = 2, 3, 5, 7
    c = 2 * A.VEC[dtn]
    x = np.random.RandomState(1).randint(-9, 10, size=(n, cs, h, w)).astype(np.float32)
    want = A.nchw_to_framed(x, c, dtn)
    xt, xp = guarded_f32(x)
    y = framed('y', dtn, n, h, w, 1, c, FILL, None, *((A.VEC[dtn], c + 2 * A.VEC[dtn]) if sliced else (0, c)))
    check(_lib.lib().dbx_nchw_to_framed(_lib.DTYPE_ID[dtn], xp, cs, C.byref(vw(y)), stream_ptr()))
    torch.cuda.synchronize()
    assert_f32(xt, x, 'input')
    assert not want[..., cs:].any()
    check_output(y, want, want, 'dbx_nchw_to_framed %s' % dtn)


@pytest.mark.parametrize('dtn', DTNS)
def test_nchw_to_framed_ch_builds_the_refine_input(dtn):
    """The engine's two calls: 4 landmark planes to channels 0 .. 3, the score plane to channel 4, of an 8-channel frame; channels
    5 .. 7, the halo and the guards are not touched."""
    n, h, w, c = 2, 6, 5, 8
    rng = np.random.RandomState(2)
    lm, sc = rng.randint(-9, 10, size=(n, 4, h, w)).astype(np.float32), rng.randint(-9, 10, size=(n, 1, h, w)).astype(np.float32)
    before = rng.randint(20, 30, size=(n, h, w, c)).astype(np.float64)
    y = framed('refine input', dtn, n, h, w, 1, c, FILL, before)
    lt, lp = guarded_f32(lm)
    st, sp = guarded_f32(sc)
    L, dt = _lib.lib(), _lib.DTYPE_ID[dtn]
    check(L.dbx_nchw_to_framed_ch(dt, lp, 4, C.byref(vw(y)), 0, stream_ptr()))
    torch.cuda.synchronize()
    want = A.nchw_to_framed_ch(before, lm, 0, dtn)
    assert np.array_equal(want[..., 4:], before[..., 4:])
    check_output(y, want, want, 'dbx_nchw_to_framed_ch landmarks')
    check(L.dbx_nchw_to_framed_ch(dt, sp, 1, C.byref(vw(y)), 4, stream_ptr()))
    torch.cuda.synchronize()
    want = A.nchw_to_framed_ch(want, sc, 4, dtn)
    assert np.array_equal(want[..., 5:], before[..., 5:])
    check_output(y, want, want, 'dbx_nchw_to_framed_ch score')
    assert_f32(lt, lm, 'input')
    assert_f32(st, sc, 'input')
    assert L.dbx_nchw_to_framed_ch(dt, sp, 1, C.byref(vw(y)), 8, stream_ptr()) == -1 and b'slice out of range' in L.dbx_last_error()


@pytest.mark.parametrize('dtn', DTNS)
def test_framed_add_ch_routes_the_refine_gradient(dtn):
    """The engine's two calls -- channels 0 .. 3 of d_rf_in onto the landmark gradient, channel 4 onto the score gradient -- and the same
    onto channel offset 4; integers: the sums are exact.  src on pad 1 with a halo of 200, dst on pad 0."""
    n, h, w = 2, 6, 5
    rng = np.random.RandomState(3)
    s = rng.randint(-9, 10, size=(n, h, w, 8)).astype(np.float64)
    d0 = rng.randint(-9, 10, size=(n, h, w, 16)).astype(np.float64)
    L, dt = _lib.lib(), _lib.DTYPE_ID[dtn]
    src = framed('src', dtn, n, h, w, 1, 8, HALO['x'], s)
    for c_src_off, n_ch, c_dst_off in ((0, 4, 0), (4, 1, 0), (0, 4, 4), (4, 1, 4), (3, 5, 11)):
        dst = framed('dst', dtn, n, h, w, 0, 16, FILL, d0)
        check(L.dbx_framed_add_ch(dt, C.byref(vw(src)), c_src_off, n_ch, C.byref(vw(dst)), c_dst_off, stream_ptr()))
        torch.cuda.synchronize()
        want = A.framed_add_ch(d0, s, c_src_off, n_ch, c_dst_off, dtn)
        untouched = [ch for ch in range(16) if not c_dst_off <= ch < c_dst_off + n_ch]
        assert np.array_equal(want[..., untouched], d0[..., untouched]) and not np.array_equal(want, d0)
        check_output(dst, want, want, 'dbx_framed_add_ch(%d, %d, %d)' % (c_src_off, n_ch, c_dst_off))
        assert_holds(src, what='input')


@pytest.mark.parametrize('dtn', DTNS)
def test_framed_to_nchw_f32_reads_the_view_only(dtn):
    """From channels [8, 16) of a 24-channel pad-1 frame whose halo holds 200 and whose other channels hold 1000: neither leaks."""
    n, h, w, c = 2, 5, 7, 8
    x = np.random.RandomState(4).randint(-9, 10, size=(n, h, w, c)).astype(np.float64)
    src = framed('x', dtn, n, h, w, 1, c, HALO['x'], x, 8, 24)
    want = A.framed_to_nchw(x)
    assert want.shape == (n, c, h, w) and np.abs(want).max() < 10
    yt, yp = guarded_f32(np.full(want.shape, FILL))
    check(_lib.lib().dbx_framed_to_nchw_f32(_lib.DTYPE_ID[dtn], C.byref(vw(src)), yp, stream_ptr()))
    torch.cuda.synchronize()
    assert_f32(yt, want, 'dbx_framed_to_nchw_f32 %s' % dtn)
    assert_holds(src, what='input')
