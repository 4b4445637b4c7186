"""Every weight-gradient kernel path wgrad_plan (csrc/conv_wgrad.hip) can select by default, pinned with exact-integer cases.

Each case (a) asks dbx_conv_wgrad_plan and asserts the kernel NAME and the split count -- both derived here from the planner's rule,
restated below, with the device's CU count where the rule uses it -- plus the split premise the case was sized for ("last split
short", "trailing split empty"), (b) runs on integer operands in [-3, 3] and asserts BITWISE equality with the float64 CPU reference
of tests/wgrad_ref.py (its docstring derives the zero tolerance: every partial sum in any order is an integer below 2**24, exact in
fp32; the premise is asserted from the reference before anything is launched), (c) runs again with accumulate = 1 and asserts exactly
2 x reference, (d) launches a third time into fresh buffers and asserts bitwise equality with the first.  The scratch buffer starts as
NaN bytes, so a slab that is reduced without having been written shows too.

Shapes are about the smallest that select each path: (n, H, W, view channels of x, real ci, co).  The 3x3 cases with 128 couts on 64
input channels go to wgrad_all9_kernel (dz->c % 128 == 0, x->c % 64 == 0), so the all-taps / strip cases use 64 couts (or an x view
that is no multiple of 64 channels).

Content variants on the all9, strip, wide2 and all-taps cases: single-impulse operands (one 1 in x, one 1 in dz) at the corners of the
first and last image, across every image seam, and in the last column of the (ragged) last strip -- the expected dw has at most one
nonzero tap, so a failure names the dropped or doubled pixel; and channel-slice views (c_off > 0, ld > c for x and dz) whose
neighbouring channels hold 1000 at every image pixel (the frame halo and the guard bands stay zero, as the ABI requires) -- a read
outside the slice breaks exact equality, and the frames must come back unchanged.

DBX_WGRAD_VARIANT is read once per process, so wgrad_row3_kernel and wgrad_wide_kernel cannot be selected here; they keep their
comparison in test_hip_kernels.py::test_forced_kernel_variants_in_subprocesses, which re-runs test_conv_wgrad_kernel under
DBX_WGRAD_VARIANT=20 (its 128 -> 128 3x3 case takes wgrad_row3_kernel, its 768 -> 512 1x1 case wgrad_wide_kernel)."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_ref as R                                   # noqa: E402

from densebox_amd import _lib                           # noqa: E402
from densebox_amd._lib import View, check, ptr, stream_ptr   # noqa: E402

pytestmark = pytest.mark.gpu
TDT = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}
SENTINEL = 1000.0            # exact in f16 (11 significand bits), bf16 (1000 = 250 * 4: 8 bits) and fp32

NAMES = {'c8': 'wgrad3x3_c8_kernel<%s>', 'alltaps': 'wgrad3x3_kernel<%s>', 'strip': 'wgrad3x3_strip_kernel<%s>',
         'all9': 'wgrad_all9_kernel<%s>', 'wide2': 'wgrad_wide2_kernel<%s>', 'g64': 'wgrad_kernel<%s,64,64>',
         'g128': 'wgrad_kernel<%s,128,128>'}


class Case:
    """path: the kernel wgrad_plan must select (read off the planner, not off a run).  premise: what the split layout must look like
    ('short': > 1 split, the last one shorter than the first but not empty; 'empty': a trailing split without work; 'short_or_empty':
    > 1 split, the last shorter than the first; 'ragged': > 1 split and a last column strip of fewer than 32 columns)."""

    def __init__(self, name, path, n, h, w, civ, ci, co, k=3, cpad=1, xpad=1, f32=False, premise=None, variants=False):
        self.name, self.path, self.n, self.h, self.w, self.civ, self.ci, self.co = name, path, n, h, w, civ, ci, co
        self.k, self.cpad, self.xpad, self.f32, self.premise, self.variants = k, cpad, xpad, f32, premise, variants
        self.ho, self.wo = h + 2 * cpad - k + 1, w + 2 * cpad - k + 1
        assert (h - self.ho) % 2 == 0
        self.zpad = xpad + (h - self.ho) // 2            # dz lives on a frame congruent with x's
        self.cov = (max(co, 8) + 7) // 8 * 8
        self.hp, self.wp = h + 2 * xpad, w + 2 * xpad
        self.Q = n * self.hp * self.wp

    def __repr__(self):
        return self.name


CASES = [
    # conv1_1's kernel: one 16-byte chunk per pixel, ld == c (no slice possible), 64 couts
    Case('c8', 'c8', 2, 13, 19, 8, 3, 64),
    # all nine taps per workgroup, linear walk: padded width below 64
    Case('alltaps-64', 'alltaps', 2, 20, 28, 64, 64, 64, variants=True),
    Case('alltaps-100of128', 'alltaps', 3, 17, 23, 128, 100, 64, variants=True),
    # column-strip walk: padded width 64 (exactly two strips), 65 (a third strip of ONE column), 96
    Case('strip-w62', 'strip', 2, 9, 62, 128, 128, 64, variants=True),
    Case('strip-w63', 'strip', 2, 9, 63, 128, 128, 64, premise='ragged', variants=True),
    Case('strip-w94', 'strip', 2, 9, 94, 128, 128, 64, variants=True),
    # 128 x 64 tiles over nine taps by LDS-DMA: compact walk from padded width 32, linear below
    Case('all9-compact-w30', 'all9', 3, 9, 30, 128, 128, 128, variants=True),
    Case('all9-compact-w33-3x2tiles', 'all9', 2, 7, 33, 192, 192, 256, variants=True),
    Case('all9-linear-w29', 'all9', 3, 9, 29, 128, 128, 128, variants=True),
    # 256 x 256 tiles of the 1x1 layers: compact / linear walk on frames with pad 1, and on frames without a halo
    Case('wide2-compact-w30', 'wide2', 2, 9, 30, 256, 256, 256, k=1, cpad=0, variants=True),
    Case('wide2-linear-w29', 'wide2', 2, 9, 29, 256, 256, 512, k=1, cpad=0, variants=True),
    Case('wide2-pad0', 'wide2', 2, 9, 30, 256, 256, 256, k=1, cpad=0, xpad=0, variants=True),
    # the generic per-tap kernel, 64 x 64 tiles: 8 couts under 512 input channels; 5x5 without padding (dz on a frame of pad 2)
    Case('generic64-1x1', 'g64', 2, 16, 16, 512, 512, 8, k=1, cpad=0, f32=True),
    Case('generic64-5x5', 'g64', 2, 14, 14, 64, 64, 64, k=5, cpad=0, xpad=0, f32=True),
    # ... 128 x 128 tiles: 384 channels are no multiple of 256, so the wide 1x1 kernel does not take them
    Case('generic128-1x1', 'g128', 2, 15, 15, 384, 384, 384, k=1, cpad=0, f32=True),
    # split edges.  all9: 2 x 7 = 14 compact steps in splits of 5, 5, 4; 3 x 11 = 33 steps in eight splits of 5 (the last: 3, 0)
    Case('all9-split-short', 'all9', 2, 13, 30, 128, 128, 128, premise='short'),
    Case('all9-split-8-short-empty', 'all9', 3, 21, 30, 128, 128, 128, premise='short_or_empty'),
    # strip: a split takes more than one (image, strip) unit only beyond ceil(1024 / tiles) >= 256 units, so the one case with a short
    # trailing split is wider than the rest of this file: 37 x 7 = 259 units over four 64 x 64 tiles -> 129 splits of 2 and one of 1
    Case('strip-split-short', 'strip', 37, 2, 222, 72, 72, 128, premise='short'),
    # generic kernel: 147 32-row steps -> 9 splits by the 16-step rule, rounded up to 16 of 10 steps: the last one starts past the frame
    Case('generic64-split-empty', 'g64', 2, 46, 47, 64, 64, 64, k=1, cpad=0, f32=True, premise='empty'),
]
RUNS = [(c, d) for c in CASES for d in (('bf16', 'f16', 'f32') if c.f32 else ('bf16', 'f16'))]
VARIANT_RUNS = [(c, d) for c in CASES if c.variants for d in ('bf16', 'f16')]
_ids = lambda r: '%s-%s' % (r[0].name, r[1])            # noqa: E731


def cdiv(a, b):
    return (a + b - 1) // b


def expected_plan(c, dtn, cus):
    """wgrad_plan's split rule, restated: (splits, work per split) -- work in frame rows, 64- / 32-row steps or strip units."""
    es = 4 if dtn == 'f32' else 2
    xc, zc = c.civ, c.cov
    if c.path in ('all9', 'wide2'):
        # one workgroup per CU: CUs / tiles splits, each at least 4 (all9: 64 rows) / 8 (wide2: 32 rows) steps, a multiple of 8 from 8 on
        if c.path == 'all9':
            ntile, R_, least, compact = (zc // 128) * (xc // 64), 64, 4, c.zpad == 1 and c.wp >= 32
        else:
            ntile, R_, least, compact = (zc // 256) * (xc // 256), 32, 8, c.zpad >= 1 and c.wp >= 32
        steps = c.n * cdiv(c.ho * c.wp, R_) if compact else cdiv(c.Q, R_)      # compact: the valid rows of each image only
        sp = max(cus // ntile, 1)
        if sp > steps // least:
            sp = max(steps // least, 1)
        if sp >= 8:
            sp = sp // 8 * 8
        sps = cdiv(steps, sp)
        splits = cdiv(steps, sps)
        if sp >= 8 and splits % 8:
            splits = sp
        return splits, [max(0, min(sps, steps - i * sps)) for i in range(splits)]
    if c.path == 'strip':
        tiles = cdiv(zc, 64) * cdiv(xc, 64)
        units = c.n * cdiv(c.wp, 32)
        want = max(1, min(cdiv(1024, tiles), units))
        ups = cdiv(units, want)
        splits = cdiv(units, ups)
        return splits, [min(ups, units - i * ups) for i in range(splits)]
    # linear walk over all frame rows: ~1024 workgroups (c8: 512), at least 16 32-row steps per split, a multiple of 8 from 8 on
    if c.path == 'c8':
        tiles, target, cap = 1, 512, 512
    elif c.path == 'alltaps':
        tiles, target, cap = cdiv(zc, 64) * cdiv(xc, 64), 1024, 256
    else:
        bm = 128 if (zc > 64 and xc > 64) else 64
        tiles, target, cap = cdiv(zc, bm) * cdiv(xc, bm) * c.k * c.k, 1024, 256
    steps = cdiv(c.Q, 32)
    splits = max(1, min(cdiv(target, tiles), max(steps // 16, 1), cap))
    if splits >= 8:
        splits = cdiv(splits, 8) * 8
    rows = cdiv(cdiv(steps, splits), 2) * 2 * 32
    assert es in (2, 4)
    return splits, [max(0, min(rows, c.Q - i * rows)) for i in range(splits)]


def make_frame(data_nchw, pad, tdt, c_off=0, ld=None):
    """NCHW fp32 -> zero-framed NHWC tensor between zero guard bands (the kernels walk frames linearly and read a tile and some frame
    rows past either end) + its View.  ld > c: the view is a channel slice; the other channels hold SENTINEL at every image pixel."""
    n, c, h, w = data_nchw.shape
    ld = c if ld is None else ld
    hp, wp = h + 2 * pad, w + 2 * pad
    guard = max(8 * wp, 576 + 4 * wp) * ld
    flat = torch.zeros(2 * guard + n * hp * wp * ld, dtype=tdt, device='cuda')
    t = flat[guard:guard + n * hp * wp * ld].view(n, hp, wp, ld)
    inner = t[:, pad:pad + h, pad:pad + w]
    if ld > c:
        inner[...] = SENTINEL
    inner[..., c_off:c_off + c] = data_nchw.permute(0, 2, 3, 1).to(tdt)
    return flat, t, View(C.c_void_p(t.data_ptr()), n, h, w, pad, ld, c_off, c)


_REFS = {}


def reference(c):
    """Operands and float64 reference of a case, computed once and left unchanged; the exactness premise asserted before any launch."""
    if c.name not in _REFS:
        x, dz = R.int_operands(len(c.name) * 131 + c.w, c.n, c.civ, c.ci, c.cov, c.co, c.h, c.w, c.ho, c.wo)
        dw, db, A = R.wgrad_ref64(x[:, :c.ci], dz[:, :c.co], c.k, c.cpad)
        R.check_exact_premise(A, dz)
        R.check_exact_premise(A, dz, times=2)               # the accumulate run
        assert float(dw.abs().max()) > 0 and float(db.abs().max()) > 0
        _REFS[c.name] = (x, dz, dw.float(), db.float())     # integers below 2**24: the fp32 copies are exact
    return _REFS[c.name]


def assert_exact(got, ref, what):
    ref = ref.to(got.device)
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        first = tuple(bad[0].tolist())
        raise AssertionError('%s: %d of %d elements differ; first at %s: got %r, reference %r' %
                             (what, bad.shape[0], ref.numel(), first, float(got[first]), float(ref[first])))


def assert_plan(L, c, dtn, zv, xv):
    name = C.create_string_buffer(64)
    splits = C.c_int32(-1)
    check(L.dbx_conv_wgrad_plan(_lib.DTYPE_ID[dtn], C.byref(zv), C.byref(xv), c.k, c.k, name, 64, C.byref(splits)))
    assert name.value.decode() == NAMES[c.path] % dtn, (c.name, name.value.decode())
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    want, work = expected_plan(c, dtn, cus)
    assert splits.value == want, (c.name, splits.value, want, cus)
    if c.premise == 'short':
        assert want > 1 and 0 < work[-1] < work[0], (c.name, work)
    elif c.premise == 'short_or_empty':
        assert want > 1 and work[-1] < work[0], (c.name, work)
    elif c.premise == 'empty':
        assert want > 1 and work[-1] == 0 and work[0] > 0, (c.name, work)
    elif c.premise == 'ragged':
        assert want > 1 and c.wp % 32 != 0, (c.name, work)
    else:
        assert c.premise is None
    return want


def scratch_for(L, dt, c, zv, xv):
    nbytes = L.dbx_conv_wgrad_scratch_bytes(dt, C.byref(zv), C.byref(xv), c.k, c.k)
    return torch.full((nbytes,), 255, dtype=torch.uint8, device='cuda')       # NaN bytes: an unwritten slab cannot pass for zeros


def launch(L, dt, c, zv, xv, dw, db, sc, accumulate=0):
    check(L.dbx_conv_wgrad(dt, C.byref(zv), C.byref(xv), c.k, c.k, c.cpad, c.co, c.ci, ptr(dw), ptr(db), ptr(sc), accumulate, stream_ptr()))


def run_exact(c, dtn, slices=None):
    """Steps 1 - 6 of the module docstring on the case's random integer operands; slices = ((x c_off, x ld), (dz c_off, dz ld))."""
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    x, dz, rdw, rdb = reference(c)                         # the premise is asserted in here, before anything touches the GPU
    (xo, xl), (zo, zl) = slices if slices else ((0, None), (0, None))
    fx, tx, xv = make_frame(x, c.xpad, tdt, xo, xl)         # keep the tensors alive: the Views only carry raw pointers
    fz, tz, zv = make_frame(dz, c.zpad, tdt, zo, zl)
    fx0, fz0 = fx.clone(), fz.clone()
    assert_plan(L, c, dtn, zv, xv)
    sc = scratch_for(L, dt, c, zv, xv)
    dw = torch.full((c.co, c.ci, c.k, c.k), 7.0, device='cuda')
    db = torch.full((c.co,), 7.0, device='cuda')
    launch(L, dt, c, zv, xv, dw, db, sc)
    assert_exact(dw, rdw, '%s %s dw' % (c.name, dtn))
    assert_exact(db, rdb, '%s %s db' % (c.name, dtn))
    first_dw, first_db = dw.clone(), db.clone()
    launch(L, dt, c, zv, xv, dw, db, sc, accumulate=1)
    assert_exact(dw, 2 * rdw, '%s %s dw after accumulate' % (c.name, dtn))
    assert_exact(db, 2 * rdb, '%s %s db after accumulate' % (c.name, dtn))
    dw2 = torch.full_like(dw, -3.0)
    db2 = torch.full_like(db, -3.0)
    launch(L, dt, c, zv, xv, dw2, db2, sc)
    assert torch.equal(dw2, first_dw) and torch.equal(db2, first_db), '%s %s: second launch differs from the first' % (c.name, dtn)
    assert torch.equal(fx, fx0) and torch.equal(fz, fz0), '%s %s: an operand frame changed' % (c.name, dtn)


@pytest.mark.parametrize('run', RUNS, ids=_ids)
def test_wgrad_path_is_exact_on_integer_operands(run):
    run_exact(*run)


def slices_for(c):
    """Slice geometry per path: the LDS-DMA kernels (all9, wide2) get 128-byte multiples (c_off 64 elements, ld c + 128), the
    register-staged ones the ABI's minimum of 16 bytes (c_off 8 elements, ld c + 24)."""
    if c.path in ('all9', 'wide2'):
        return ((64, c.civ + 128), (64, c.cov + 128))
    return ((8, c.civ + 24), (8, c.cov + 24))


@pytest.mark.parametrize('run', VARIANT_RUNS, ids=_ids)
def test_wgrad_path_is_exact_on_channel_slices_of_wider_frames(run):
    c, dtn = run
    run_exact(c, dtn, slices_for(c))


def impulse_places(c):
    """(x position, dz position) pairs, positions as (image, channel, y, x) of the unframed maps (dz has x's extent on these paths)."""
    n, h, w = c.n, c.h, c.w
    corners = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    pix = []
    for img in (0, n - 1):
        for (y, xx) in corners:
            pix.append(((img, y, xx), (img, y, xx)))                                   # same pixel: the centre tap (1x1: the tap)
            iy, ix = (1 if y == 0 else h - 2), (1 if xx == 0 else w - 2)
            pix.append(((img, iy, ix), (img, y, xx)))                                   # dz in the corner, x diagonally inside: a corner tap
            pix.append(((img, y, xx), (img, iy, ix)))                                   # ... and the other way round
    for img in range(n - 1):                                                            # across the seam: nothing may be counted
        pix.append(((img, h - 1, w - 1), (img + 1, 0, 0)))
        pix.append(((img + 1, 0, 0), (img, h - 1, w - 1)))
    ym = h // 2                                                                         # last column (of the last, maybe ragged, strip)
    pix.append(((n - 1, ym, w - 1), (n - 1, ym, w - 1)))
    pix.append(((n - 1, ym, w - 1), (n - 1, ym, w - 2)))
    pix.append(((n - 1, ym, w - 2), (n - 1, ym, w - 1)))
    pix.append(((n - 1, ym + 1, w - 1), (n - 1, ym, w - 1)))
    out = []
    for i, (xp, zp) in enumerate(pix):                     # first / last real channel in turn: first and last tile of either operand
        cx = (0, c.ci - 1)[i % 2]
        cz = (0, c.co - 1)[(i // 2) % 2]
        out.append(((xp[0], cx, xp[1], xp[2]), (zp[0], cz, zp[1], zp[2])))
    return out


@pytest.mark.parametrize('run', VARIANT_RUNS, ids=_ids)
def test_wgrad_path_counts_every_impulse_pixel_exactly_once(run):
    c, dtn = run
    assert (c.ho, c.wo) == (c.h, c.w)
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    fx, tx, xv = make_frame(torch.zeros(c.n, c.civ, c.h, c.w), c.xpad, tdt)
    fz, tz, zv = make_frame(torch.zeros(c.n, c.cov, c.ho, c.wo), c.zpad, tdt)
    assert_plan(L, c, dtn, zv, xv)
    sc = scratch_for(L, dt, c, zv, xv)
    dw = torch.empty(c.co, c.ci, c.k, c.k, device='cuda')
    db = torch.empty(c.co, device='cuda')
    places = impulse_places(c)
    hit = 0
    for xpos, zpos in places:
        edw, edb = R.impulse_expected(c.co, c.ci, c.k, c.cpad, xpos, zpos)
        assert int((edw != 0).sum()) <= 1
        hit += int((edw != 0).sum())
        tx[xpos[0], c.xpad + xpos[2], c.xpad + xpos[3], xpos[1]] = 1.0
        tz[zpos[0], c.zpad + zpos[2], c.zpad + zpos[3], zpos[1]] = 1.0
        dw.fill_(7.0)
        db.fill_(7.0)
        launch(L, dt, c, zv, xv, dw, db, sc)
        tx[xpos[0], c.xpad + xpos[2], c.xpad + xpos[3], xpos[1]] = 0.0
        tz[zpos[0], c.zpad + zpos[2], c.zpad + zpos[3], zpos[1]] = 0.0
        assert_exact(dw, edw.float(), '%s %s dw, impulse x at %s, dz at %s (image, channel, y, x)' % (c.name, dtn, xpos, zpos))
        assert_exact(db, edb.float(), '%s %s db, impulse x at %s, dz at %s' % (c.name, dtn, xpos, zpos))
    assert hit >= 8 and hit < len(places)                  # both kinds occur: a tap that must be 1, pairs that must give nothing
    assert float(fx.abs().sum()) == 0 and float(fz.abs().sum()) == 0


@pytest.mark.parametrize('dtn', ['bf16', 'f16'])
def test_wgrad_slice_of_a_sliced_x_lands_exactly_in_its_column_range(dtn):
    """dbx_conv_wgrad_slice with x a real channel slice of a wider frame (sentinels around it), into columns [40, 40 + ci) of a wider dw
    pre-filled with 7.0: the range exact, everything else untouched."""
    c = [k for k in CASES if k.name == 'all9-compact-w30'][0]
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    x, dz, rdw, rdb = reference(c)
    (xo, xl), (zo, zl) = slices_for(c)
    fx, tx, xv = make_frame(x, c.xpad, tdt, xo, xl)
    fz, tz, zv = make_frame(dz, c.zpad, tdt, zo, zl)
    fx0, fz0 = fx.clone(), fz.clone()
    assert_plan(L, c, dtn, zv, xv)
    sc = scratch_for(L, dt, c, zv, xv)
    ctot, coff = c.ci + 72, 40
    wide = torch.full((c.co, ctot, c.k, c.k), 7.0, device='cuda')
    db = torch.full((c.co,), 7.0, device='cuda')
    check(L.dbx_conv_wgrad_slice(dt, C.byref(zv), C.byref(xv), c.k, c.k, c.cpad, c.co, c.ci, ptr(wide), ctot, coff, ptr(db), ptr(sc), 0,
                                 stream_ptr()))
    assert_exact(wide[:, coff:coff + c.ci].contiguous(), rdw, 'column range of the wide dw')
    assert_exact(db, rdb, 'db')
    assert bool((wide[:, :coff] == 7.0).all()) and bool((wide[:, coff + c.ci:] == 7.0).all())
    check(L.dbx_conv_wgrad_slice(dt, C.byref(zv), C.byref(xv), c.k, c.k, c.cpad, c.co, c.ci, ptr(wide), ctot, coff, ptr(db), ptr(sc), 1,
                                 stream_ptr()))
    assert_exact(wide[:, coff:coff + c.ci].contiguous(), 2 * rdw, 'column range of the wide dw after accumulate')
    assert bool((wide[:, :coff] == 7.0).all()) and bool((wide[:, coff + c.ci:] == 7.0).all())
    assert torch.equal(fx, fx0) and torch.equal(fz, fz0)


# ------------------------------------------------------------------------------------------------ dz = a max pooling's backward
def _pool_setup(L, dt, tdt, n, h, w, c):
    """Integer activations without ties (every 2x2 window a permutation of 1..4, one window in eight all zero: gate bit clear), the
    arg-max nibbles from dbx_maxpool2x2_idx, an integer pooled gradient and the un-pooled gradient they imply (float64-exact)."""
    g = torch.Generator(device='cpu').manual_seed(h * 7 + w)
    perm = torch.rand(n, c, h // 2, w // 2, 4, generator=g).argsort(-1).float() + 1.0
    dead = torch.rand(n, c, h // 2, w // 2, 1, generator=g) < 0.125
    perm = torch.where(dead, torch.zeros_like(perm), perm)
    act = perm.view(n, c, h // 2, w // 2, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h, w)
    dy = torch.randint(-3, 4, (n, c, h // 2, w // 2), generator=g).float()
    up = dy.repeat_interleave(2, 2).repeat_interleave(2, 3)
    dz = torch.where(act == 4.0, up, torch.zeros_like(up))                          # the window's maximum, where the ReLU passed
    assert torch.equal(F.max_pool2d(act, 2), torch.where(dead[..., 0], torch.zeros(()), torch.full((), 4.0)))
    fa, ta, av = make_frame(act, 1, tdt)
    fp, tp, pv = make_frame(torch.zeros(n, c, h // 2, w // 2), 0, tdt)
    idx = torch.zeros(L.dbx_maxpool_idx_bytes(n, h, w, c) + 16, dtype=torch.uint8, device='cuda')
    check(L.dbx_maxpool2x2_idx(dt, C.byref(av), C.byref(pv), ptr(idx), stream_ptr()))
    return dy, dz, idx


@pytest.mark.parametrize('dtn', ['bf16', 'f16'])
def test_wgrad_pool_dz_is_exact_on_integer_operands(dtn):
    """dbx_conv_wgrad_pool_dz on the valid 64 / 64 / 64 geometry (padded width 64: two strips) against the float64 reference of the
    un-pooled gradient built on the CPU; the nibbles come from dbx_maxpool2x2_idx."""
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    n, h, w, c = 2, 8, 62, 64
    dy, dz, idx = _pool_setup(L, dt, tdt, n, h, w, c)
    x = R.int_operands(3, n, c, c, c, c, h, w, h, w)[0]
    rdw, rdb, A = R.wgrad_ref64(x, dz, 3, 1)
    R.check_exact_premise(A, dz, times=2)
    assert float(rdw.abs().max()) > 0
    fdy, tdy, dyv = make_frame(dy, 0, tdt)
    fx, tx, xv = make_frame(x, 1, tdt)
    zshape = View(None, n, h, w, 1, c, 0, c)                                         # shape only: the map is not in memory
    assert L.dbx_conv_wgrad_pool_dz_ok(dt, C.byref(zshape), C.byref(xv), 3, 3) == 1
    name = C.create_string_buffer(64)
    check(L.dbx_conv_wgrad_plan(dt, C.byref(zshape), C.byref(xv), 3, 3, name, 64, None))
    assert name.value.decode() == NAMES['strip'] % dtn
    sc = torch.full((L.dbx_conv_wgrad_scratch_bytes(dt, C.byref(zshape), C.byref(xv), 3, 3),), 255, dtype=torch.uint8, device='cuda')
    dw = torch.full((c, c, 3, 3), 7.0, device='cuda')
    db = torch.full((c,), 7.0, device='cuda')
    check(L.dbx_conv_wgrad_pool_dz(dt, C.byref(dyv), ptr(idx), c, C.byref(zshape), C.byref(xv), 3, 3, 1, c, c, ptr(dw), ptr(db), ptr(sc), 0, 0,
                                   stream_ptr()))
    assert_exact(dw, rdw.float(), 'pooled-dz dw')
    assert_exact(db, rdb.float(), 'pooled-dz db')
    check(L.dbx_conv_wgrad_pool_dz(dt, C.byref(dyv), ptr(idx), c, C.byref(zshape), C.byref(xv), 3, 3, 1, c, c, ptr(dw), ptr(db), ptr(sc), 1, 0,
                                   stream_ptr()))
    assert_exact(dw, 2 * rdw.float(), 'pooled-dz dw after accumulate')
    assert_exact(db, 2 * rdb.float(), 'pooled-dz db after accumulate')


@pytest.mark.parametrize('dtn', ['bf16', 'f16'])
def test_wgrad_pool_dz_refuses_channel_counts_that_are_no_multiple_of_64(dtn):
    """A 72-channel dz (a multiple of 8, not of 64): the kernel's masked lanes would load dy and nibbles past the pixel's channels, so
    the query says no and the call returns an error before any launch.  The query is asserted first and every buffer is real and
    zero, so nothing runs out of bounds whatever the outcome."""
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    n, h, w, c, cx = 2, 8, 62, 72, 64
    fdy, tdy, dyv = make_frame(torch.zeros(n, c, h // 2, w // 2), 0, tdt)
    fx, tx, xv = make_frame(torch.zeros(n, cx, h, w), 1, tdt)
    fz, tz, zv = make_frame(torch.zeros(n, c, h, w), 1, tdt)
    idx = torch.zeros(L.dbx_maxpool_idx_bytes(n, h, w, c) + 4096, dtype=torch.uint8, device='cuda')
    name = C.create_string_buffer(64)
    check(L.dbx_conv_wgrad_plan(dt, C.byref(zv), C.byref(xv), 3, 3, name, 64, None))
    assert name.value.decode() == NAMES['strip'] % dtn                                 # the strip kernel's shape: only the channel count is wrong
    assert L.dbx_conv_wgrad_pool_dz_ok(dt, C.byref(zv), C.byref(xv), 3, 3) == 0
    # 64 of the 72 channels as a view: a multiple of 64, but co != dz->c is the call's to refuse; 64 channels at offset 16 leave the pixel
    v64 = View(C.c_void_p(tz.data_ptr()), n, h, w, 1, c, 0, 64)
    assert L.dbx_conv_wgrad_pool_dz_ok(dt, C.byref(View(C.c_void_p(tz.data_ptr()), n, h, w, 1, c, 16, 64)), C.byref(xv), 3, 3) == 0
    sc = torch.zeros(L.dbx_conv_wgrad_scratch_bytes(dt, C.byref(zv), C.byref(xv), 3, 3), dtype=torch.uint8, device='cuda')
    dw = torch.full((c, cx, 3, 3), 7.0, device='cuda')
    db = torch.full((c,), 7.0, device='cuda')
    rc = L.dbx_conv_wgrad_pool_dz(dt, C.byref(dyv), ptr(idx), c, C.byref(zv), C.byref(xv), 3, 3, 1, c, cx, ptr(dw), ptr(db), ptr(sc), 0, 0, stream_ptr())
    assert rc != 0 and b'multiple of 64' in L.dbx_last_error()
    dy64 = View(C.c_void_p(tdy.data_ptr()), n, h // 2, w // 2, 0, c, 0, 64)
    rc = L.dbx_conv_wgrad_pool_dz(dt, C.byref(dy64), ptr(idx), c, C.byref(v64), C.byref(xv), 3, 3, 1, 56, cx, ptr(dw), ptr(db), ptr(sc), 0, 0, stream_ptr())
    assert rc != 0 and b'co == dz->c' in L.dbx_last_error()
    torch.cuda.synchronize()
    assert bool((dw == 7.0).all()) and bool((db == 7.0).all())                        # nothing ran
