"""Every path of the heads' FIRST stage against the float64 reference of tests/heads1_ref.py, bit for bit.

Kernels and the case that pins each path (the restated plans of heads1_ref are asserted first, against dbx_heads_forward_fusable,
dbx_conv_plan, dbx_conv_wgrad_plan and the libraries' own *_scratch_bytes wherever the library answers):
  A  dbx_heads_forward_fused / _heads  conv3x3_p8_kernel<T,1,1> with the second weights (fusable == 2, plain images) and
                                       conv3x3_ws_kernel<T,1,1,2,4> (DBX_CONV_WFRAG, mode-4 images), then heads2_finish_kernel, on
                                       f-nh4 (24 p8 tiles of 7 / 8 units, last unit 20 pixels; exactly 192 ws items), f-nh1-k5 (k > 4 with one
                                       head), f-nh2 (last unit 2 pixels), f-nh3 (odd head count, two seams), f-roundup (the p8 schedule's
                                       round-up branch).  DBX_WS_NFX is read once per process: only the default NFX = 4 form (128-pixel
                                       tiles) of the ws kernel is covered here; the NFX = 8 form stays with the forced-variant runs.
  B  dbx_heads1_wgrad_gen              wgrad_wide2_kernel<T,true> on b-min (32 padded columns), b-ragged-seam (h wp = 407, splits of 10
                                       steps crossing both seams, a short last split), b-empty-split (16 splits, the last empty), b-nh1,
                                       b-nh3, b-pad2; the fp32 instantiation on the same cases; refusal below 32 padded columns.
  C  dbx_heads1_dgrad_gen              heads1_dgrad_gen_kernel<T> on c-partial (99 pixels: two waves without a pixel), c-256, c-513
                                       (npix % 256 == 1), c-nh4, c-two-tiles (ntiles in (ncu, 2 ncu): some workgroups walk two tiles -- the
                                       ring running from one tile into the next, the d_out fetch wrapping to the next tile's head 0,
                                       set_tile past the end), c-three-tiles (ntiles in (2 ncu, 3 ncu), nh = 1); the fp32 instantiation on
                                       the four small cases.  Both multi-tile sizes follow the device's CU count.

Per case: the premise of a zero tolerance from the reference alone; inputs and outputs between guard bands, outputs starting at 7,
halos at -5 (x, y) or 1000 (gate), the neighbouring channels of a slice at 1000 (inputs) / 7 (outputs); x of B is channels [512, 768)
of a 768-channel frame, dW1 columns [44, 300) of 300, y of C a 256-channel slice (c_off 512 of 768; c_off 64 of 320 on the two large
cases, whose 768-channel float64 images would take a gigabyte of host memory), gate c_off 0 of ld 256; d_out slots 8 or 16 wide with
[8, 16) at 1000; b2 beyond sum k at 1000; scratch exactly the library's own size, pre-filled with NaN bytes, with a tail that must
stay intact; WHOLE buffers compared; inputs unchanged; a second launch into fresh buffers bitwise equal; a quarter of W2 handed over
as numbers T cannot hold.  Contents: dense, impulse (f-nh4, f-nh3, b-ragged-seam, c-two-tiles), rounding (f-nh4, b-min, c-256).

The second-weight images are compared element by element with the ABI's layout (head i's k_i rows at rows 0 .. k_i - 1, columns
512 i .., zero elsewhere): the plain one directly, the fragment-order ones through heads1_ref.frag_index_1x1; the 2**24-pixel bound of
dbx_heads1_wgrad_gen is checked through its query on either side and through the refused call.

Cost, measured on an MI355X host with 16 threads, references included: the 122 tests of this file take 30.8 s, most of it the
float64 host images and their comparison.  The slowest five: c-three-tiles hash-bf16 1.74 s and none-bf16 1.58 s, f-roundup kind 2
bf16 1.23 s, the c-two-tiles impulse case hash-bf16 1.04 s, c-two-tiles hash-bf16 1.04 s (the first dtype of a case pays for its
reference).  The three-tile case stays at nh = 1: its reference, not the GPU, is what a wider one would cost (heads1_ref's docstring)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads1_ref as R                                   # noqa: E402
from framed_buf import Buf, assert_holds                # noqa: E402

from densebox_amd import _lib                           # noqa: E402
from densebox_amd._lib import View, ConvDesc, check, stream_ptr   # noqa: E402

pytestmark = pytest.mark.gpu
_FORCING = ('DBX_CONV_VARIANT', 'DBX_P8', 'DBX_P8_HEADS', 'DBX_WGRAD_VARIANT', 'DBX_HEADS_GEN')
if any(k in os.environ for k in _FORCING) or any(k.startswith('DBX_WS') for k in os.environ):
    pytest.skip('this process forces a kernel selection', allow_module_level=True)

TDT = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}
SENTINEL, HALO, FILL, TAIL = 1000.0, -5.0, 7.0, 4096     # all exact in bf16, f16 and fp32
BIAS, DROPHASH, WFRAG = _lib.EPI_BIAS, _lib.EPI_DROPHASH, _lib.CONV_WFRAG
CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
DG = R.dg_cases(CUS)


def flat(name, rows, ld, tdt, fill, interior=None):
    """A plain [rows][ld] array between guard bands."""
    return Buf(name, rows, 1, 1, 0, ld, tdt, fill, None if interior is None else np.asarray(interior, dtype=np.float64).reshape(rows, 1, 1, ld))


class Planes(Buf):
    """A fp32 [N][k][H * W] tensor between guard bands: a failure names image, output channel and pixel."""

    def __init__(self, name, n, k, hw, fill):
        Buf.__init__(self, name, n, 1, 1, 0, k * hw, torch.float32, HALO, np.full((n, 1, 1, k * hw), fill))
        self.hw = hw

    def where(self, i):
        if i < self.guard or i >= self.guard + self.body.size:
            return Buf.where(self, i)
        j = i - self.guard
        return 'image %d output channel %d pixel %d' % (j // self.ld, j % self.ld // self.hw, j % self.hw)


class Rows(Buf):
    """A fp32 [rows][ld] matrix between guard bands: a failure names row and column."""

    def __init__(self, name, rows, ld, fill):
        Buf.__init__(self, name, rows, 1, 1, 0, ld, torch.float32, HALO, np.full((rows, 1, 1, ld), fill))

    def where(self, i):
        if i < self.guard or i >= self.guard + self.body.size:
            return Buf.where(self, i)
        return 'row %d (head %d, hidden channel %d) column %d' % ((i - self.guard) // self.ld, (i - self.guard) // self.ld // 512, (i - self.guard) // self.ld % 512,
                                                                  (i - self.guard) % self.ld)


def nan_scratch(nbytes):
    return torch.full((nbytes + TAIL,), 0xFF, dtype=torch.uint8, device='cuda')


def assert_tail(scratch, nbytes, what):
    assert bool((scratch[nbytes:] == 0xFF).all()), what + ': the tail behind the scratch was written'


def slots(d_out, slot):
    """[P][nh][8] -> [P][nh * slot] with the channels [8, slot) of every slot at the sentinel."""
    P, nh, _ = d_out.shape
    a = np.full((P, nh, slot), SENTINEL)
    a[:, :, :8] = d_out
    return a.reshape(P, nh * slot)


def w2_bufs(m, dtn):
    return [flat('W2[%d]' % i, a.shape[0], 512, torch.float32, SENTINEL, a).upload() for i, a in enumerate(R.w2_raw(m['w2'], m['un'], dtn))]


def assert_w2_premise(m, dtn):
    """The values handed over round to the reference's W2, and in a 16-bit type a quarter of them are no numbers of T."""
    raw = R.w2_raw(m['w2'], m['un'], dtn)
    for a, b in zip(raw, m['w2']):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a) and np.array_equal(R.round_np(a, dtn), b)
    if dtn != 'f32':
        assert all(0.15 < float((R.round_np(a, dtn) != a).mean()) < 0.35 for a in raw)


# ================================================================================================ A: the fused forward
class Forward:
    def __init__(self, case, kind, dtn, m, ref):
        self.L, self.case, self.kind, self.dtn, self.m, self.ref = _lib.lib(), case, kind, dtn, m, ref
        self.dt, self.tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
        L, dt, tdt = self.L, self.dt, self.tdt
        n, h, w, ks = case.n, case.h, case.w, case.ks
        self.nh, self.ktot, self.P = len(ks), sum(ks), n * h * w
        nh, co = self.nh, 512 * self.nh
        self.d = ConvDesc(dt, 1, 1, 0, 768, co, BIAS | DROPHASH | (WFRAG if kind == 1 else 0), R.SEED)
        self.x = Buf('x', n, h, w, 1, 768, tdt, HALO, m['x'].reshape(n, h, w, 768)).upload()
        self.b1 = flat('b1', 1, co, torch.float32, SENTINEL, m['b1']).upload()
        self.b2 = flat('b2', 1, 64, torch.float32, SENTINEL, np.concatenate([m['b2'], np.full(64 - self.ktot, SENTINEL)])).upload()
        self.w1 = flat('W1', co, 768, torch.float32, SENTINEL, m['w1']).upload()
        raw = R.w2_raw(m['w2'], m['un'], dtn)
        self.w2 = w2_bufs(m, dtn)
        self.w1img = torch.zeros(L.dbx_conv_packed_elems(C.byref(ConvDesc(dt, 1, 1, 0, 768, co, 0, 0))) * 2, dtype=torch.uint8, device='cuda')
        check(L.dbx_pack_weight(dt, 4 if kind == 1 else 0, C.c_void_p(self.w1.ptr()), co, 768, 1, 1, C.c_void_p(self.w1img.data_ptr()), co, 768, 0, 0, stream_ptr()))
        if kind == 1:
            torch.cuda.synchronize()
            img = self.w1img.view(tdt).cpu()               # (dbx_conv_packed_elems adds the slack the ws kernel's weight stream over-runs: zeros)
            assert torch.equal(img[:co * 768], torch.from_numpy(R.frag_image_1x1(m['w1'].astype(np.float64))).to(tdt)) and not bool(img[co * 768:].any()), \
                'the fragment-order W1 image'
        rows = 256 if kind == 1 else 64
        self.w2img = torch.zeros(L.dbx_conv_packed_elems(C.byref(ConvDesc(dt, 1, 1, 0, co, rows, 0, 0))) * 2, dtype=torch.uint8, device='cuda')
        for i, (b, k) in enumerate(zip(self.w2, ks)):
            check(L.dbx_pack_weight(dt, 4 if kind == 1 else 0, C.c_void_p(b.ptr()), k, 512, 1, 1, C.c_void_p(self.w2img.data_ptr()), rows, co, 0, 512 * i, stream_ptr()))
        torch.cuda.synchronize()
        # the ABI's layout of the second weights: head i's k_i rows at rows 0 .. k_i - 1, columns 512 i ..; everything else zero
        img = self.w2img.view(tdt)
        want = np.zeros((rows, co))
        for i, (a, k) in enumerate(zip(raw, ks)):
            want[:k, 512 * i:512 * (i + 1)] = R.round_np(a, dtn)
        if kind == 2:
            assert img.numel() == rows * co and torch.equal(img.view(rows, co).cpu(), torch.from_numpy(want).to(tdt)), 'the plain W2 image'
        else:                                               # element by element, through the restated dbx_frag_index
            img = img.cpu()
            assert torch.equal(img[:rows * co], torch.from_numpy(R.frag_image_1x1(want)).to(tdt)) and not bool(img[rows * co:].any()), 'the fragment-order W2 image'
        self.images = [self.w1img.clone(), self.w2img.clone()]
        self.sbytes = int(L.dbx_heads_forward_fused_scratch_bytes(nh, self.P))
        assert self.sbytes == 2 * nh * self.P * 8 * 4 + 256
        self.karr = (C.c_int32 * nh)(*ks)
        hw = h * w
        per_head = [o.reshape(n, hw, k).transpose(0, 2, 1) for o, k in zip(ref['out'], ks)]                    # [n][k][hw]
        self.want_out = np.concatenate(per_head, axis=1).reshape(n, self.ktot * hw)
        self.want_heads = [a.reshape(n, k * hw) for a, k in zip(per_head, ks)]

    def fresh(self):
        case, n = self.case, self.case.n
        hw = case.h * case.w
        self.hid = Buf('hid', n, case.h, case.w, 0, 512 * self.nh, self.tdt, HALO, FILL).upload()
        self.out = Planes('out', n, self.ktot, hw, FILL).upload()
        self.heads = [Planes('out[%d]' % i, n, k, hw, FILL).upload() for i, k in enumerate(case.ks)]
        self.scratch = nan_scratch(self.sbytes)

    def args(self):
        return (C.byref(self.d), C.byref(self.x.view()), C.c_void_p(self.w1img.data_ptr()), C.c_void_p(self.b1.ptr()), C.byref(self.hid.view()),
                C.c_void_p(self.w2img.data_ptr()), C.c_void_p(self.b2.ptr()), self.karr, self.nh)

    def run(self, per_head):
        self.fresh()
        if per_head:
            outs = (C.c_void_p * self.nh)(*[b.ptr() for b in self.heads])
            check(self.L.dbx_heads_forward_fused_heads(*self.args(), outs, C.c_void_p(self.scratch.data_ptr()), stream_ptr()))
        else:
            check(self.L.dbx_heads_forward_fused(*self.args(), C.c_void_p(self.out.ptr()), C.c_void_p(self.scratch.data_ptr()), stream_ptr()))
        torch.cuda.synchronize()
        what = '%s kind %d %s%s' % (self.case.name, self.kind, self.dtn, ' (per-head outputs)' if per_head else '')
        for b in [self.x, self.b1, self.b2, self.w1] + self.w2:
            assert_holds(b, what=what + ': input')
        assert torch.equal(self.w1img, self.images[0]) and torch.equal(self.w2img, self.images[1]), what + ': a weight image changed'
        assert_tail(self.scratch, self.sbytes, what)
        n, h, w = self.case.n, self.case.h, self.case.w
        assert_holds(self.hid, self.hid.with_interior(self.ref['hid'].reshape(n, h, w, -1)), what=what)
        assert_holds(self.out, None if per_head else self.out.with_interior(self.want_out.reshape(n, 1, 1, -1)), what=what)
        for b, a in zip(self.heads, self.want_heads):
            assert_holds(b, b.with_interior(a.reshape(n, 1, 1, -1)) if per_head else None, what=what)
        return [self.hid.dev.clone(), self.out.dev.clone()] + [b.dev.clone() for b in self.heads]


def fwd_reference(case, content, dtn):
    m = R.make_fwd(case, content, CUS)
    key = dtn if content == 'rounding' else 'any'
    refs = m.setdefault('refs', {})
    if key not in refs:
        hid, exact, out, absum = R.fwd_ref(m['pre'], m['keep'], m['w2'], m['b2'], case.ks, dtn)
        refs[key] = dict(hid=hid, exact=exact, out=out, absum=absum)
    return m, refs[key]


def run_fwd(name, kind, dtn, content='dense'):
    case, L = R.FWD[name], _lib.lib()
    plan = R.fwd_plan(case, CUS)
    assert plan['shape_ok'] and kind in plan['kinds'], '%s: at %d CUs the restated rules give %s' % (name, CUS, plan)
    if CUS == 256:
        s = plan['p8']
        assert (s['mt'], s['base'], s['extra'], s['rounded'], s['items'], s['last'], plan['ws_items']) == R.FWD_AT_256[name], plan
    # ---- the library's own answers
    dt, nh = _lib.DTYPE_ID[dtn], len(case.ks)
    xv = View(None, case.n, case.h, case.w, 1, 768, 0, 768)
    hv = View(None, case.n, case.h, case.w, 0, 512 * nh, 0, 512 * nh)
    karr = (C.c_int32 * nh)(*case.ks)
    d0 = ConvDesc(dt, 1, 1, 0, 768, 512 * nh, BIAS | DROPHASH, R.SEED)
    assert L.dbx_heads_forward_fusable(C.byref(d0), C.byref(xv), C.byref(hv), karr, nh) == plan['fusable'], plan
    cp = _lib.ConvPlan()
    dk = ConvDesc(dt, 1, 1, 0, 768, 512 * nh, BIAS | DROPHASH | (WFRAG if kind == 1 else 0), R.SEED)
    check(L.dbx_conv_plan(C.byref(dk), C.byref(xv), C.byref(hv), C.byref(cp)))
    want = ('conv3x3_ws_kernel<%s,1,1,1>' if kind == 1 else 'conv3x3_p8_kernel<%s,1,1>') % dtn
    assert (cp.name.decode(), cp.w_frag) == (want, 1 if kind == 1 else 0), (cp.name, cp.w_frag, plan)
    # ---- premise, from the reference alone
    m, ref = fwd_reference(case, content, dtn)
    R.assert_integers(m['x'], m['w1'], m['b1'], m['b2'], *m['w2'])
    R.assert_sum_premise(m['absum'], 'hid')
    R.assert_sum_premise(ref['absum'], 'out')
    assert_w2_premise(m, dtn)
    if content == 'rounding':
        R.assert_rounding_premise(ref['exact'], dtn, 'hid')
    else:
        R.assert_representable(ref['exact'], dtn, 'hid')
    assert 0.49 < 1.0 - float(m['keep'].mean()) < 0.51, 'about half of the hidden map is dropped'
    f = Forward(case, kind, dtn, m, ref)
    a = f.run(False)
    b = f.run(True)
    assert torch.equal(a[0], b[0]), 'hid differs between the two output forms'
    a2 = f.run(False)
    b2 = f.run(True)
    assert all(torch.equal(p, q) for p, q in zip(a + b, a2 + b2)), 'the second launch differs from the first'
    # the per-head form is bitwise the channel slices of the [N][sum k][H][W] form
    g = a[1].numel() - case.n * f.ktot * case.h * case.w
    full = a[1][g // 2:a[1].numel() - g // 2].view(case.n, f.ktot, case.h * case.w)
    off = 0
    for i, k in enumerate(case.ks):
        t = b[2 + i]
        gg = (t.numel() - case.n * k * case.h * case.w) // 2
        assert torch.equal(t[gg:t.numel() - gg].view(case.n, k, -1), full[:, off:off + k]), 'head %d' % i
        off += k


@pytest.mark.parametrize('name,kind,dtn', [(n, k, t) for n in R.FWD for k in (2, 1) for t in R.DTN16])
def test_fused_forward_is_exact(name, kind, dtn):
    run_fwd(name, kind, dtn)


@pytest.mark.parametrize('name,kind,dtn', [(n, k, t) for n in ('f-nh4', 'f-nh3') for k in (2, 1) for t in R.DTN16])
def test_fused_forward_puts_every_impulse_in_its_pixel(name, kind, dtn):
    case = R.FWD[name]
    px = set(R.fwd_impulse_pixels(case, CUS))
    hw = case.h * case.w
    assert {0, hw - 1, hw, case.n * hw - 1, case.w - 1, hw - case.w} <= px
    run_fwd(name, kind, dtn, 'impulse')


@pytest.mark.parametrize('kind,dtn', [(k, t) for k in (2, 1) for t in R.DTN16])
def test_fused_forward_rounds_the_hidden_map_once_to_nearest_even(kind, dtn):
    run_fwd('f-nh4', kind, dtn, 'rounding')


# ================================================================================================ B: dbx_heads1_wgrad_gen
WG_PREMISE = {
    'b-min': lambda c, p: c.w + 2 * c.pad == 32 and p['ok'],
    'b-ragged-seam': lambda c, p: (c.h * (c.w + 2 * c.pad)) % 32 != 0 and p['short'] > 0 and p['empty'] == 0 and
    any(s * p['steps_per_split'] % p['spi'] != 0 and s * p['steps_per_split'] // p['spi'] != (min((s + 1) * p['steps_per_split'], p['steps_total']) - 1) // p['spi']
        for s in range(p['splits'])),
    'b-empty-split': lambda c, p: p['empty'] >= 1 and p['splits'] % 8 == 0 and p['short'] > 0,
    'b-nh1': lambda c, p: len(c.ks) == 1 and p['ntile'] == 2,
    'b-nh3': lambda c, p: len(c.ks) == 3 and p['ntile'] == 6,
    'b-pad2': lambda c, p: c.pad == 2 and p['ok'],
}


class WGrad:
    def __init__(self, case, dtn, drop, m, ref):
        self.L, self.case, self.dtn, self.m, self.ref = _lib.lib(), case, dtn, m, ref
        self.dt, self.tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
        n, h, w, nh = case.n, case.h, case.w, len(case.ks)
        self.nh = nh
        self.d_out = Buf('d_out', n, h, w, 0, case.slot * nh, self.tdt, SENTINEL, slots(m['d_out'], case.slot).reshape(n, h, w, -1)).upload()
        xin = np.full((n * h * w, 768), SENTINEL)
        xin[:, 512:] = m['x']
        self.x = Buf('x', n, h, w, case.pad, 768, self.tdt, HALO, xin.reshape(n, h, w, 768)).upload()
        self.w2 = w2_bufs(m, dtn)
        self.use_hash, self.seed = (1, R.SEED) if drop == 'hash' else (0, 0)
        self.karr = (C.c_int32 * nh)(*case.ks)
        self.wp = (C.c_void_p * nh)(*[b.ptr() for b in self.w2])
        self.xv = self.x.view(c=256, c_off=512)
        dz = View(None, n, h, w, case.pad, 512 * nh, 0, 512 * nh)
        self.sbytes = max(int(self.L.dbx_conv_wgrad_scratch_bytes(self.dt, C.byref(dz), C.byref(self.xv), 1, 1)), 1024)
        self.dz = dz

    def fresh(self):
        co = 512 * self.nh
        self.dw = Rows('dW1', co, 300, FILL).upload()
        self.db = Planes('db1 (output channel = hidden channel)', 1, co, 1, FILL).upload()
        self.scratch = nan_scratch(self.sbytes)

    def call(self):
        return self.L.dbx_heads1_wgrad_gen(self.dt, C.byref(self.d_out.view()), C.byref(self.xv), self.wp, self.karr, self.nh, self.use_hash, self.seed, 256,
                                           C.c_void_p(self.dw.ptr()), 300, 44, C.c_void_p(self.db.ptr()), C.c_void_p(self.scratch.data_ptr()), stream_ptr())

    def verify(self, what, written=True):
        torch.cuda.synchronize()
        for b in [self.d_out, self.x] + self.w2:
            assert_holds(b, what=what + ': input')
        assert_tail(self.scratch, self.sbytes, what)
        co = 512 * self.nh
        assert_holds(self.dw, self.dw.with_interior(self.ref.dw.reshape(co, 1, 1, 256), c_off=44) if written else None, what=what)
        assert_holds(self.db, self.db.with_interior(self.ref.db.reshape(1, 1, 1, co)) if written else None, what=what)
        return [self.dw.dev.clone(), self.db.dev.clone()]


def run_wg(name, dtn, drop, content='dense'):
    case, L = R.WG[name], _lib.lib()
    pl = R.wgrad_plan_ref(case, CUS)
    assert WG_PREMISE[name](case, pl), '%s: at %d CUs the restated rule gives %s' % (name, CUS, pl)
    if CUS == 256:
        assert (pl['spi'], pl['steps_total'], pl['splits'], pl['steps_per_split']) == R.WG_AT_256[name], pl
    m = R.make_wg(case, drop, content, CUS)
    ref = R.wg_reference(m, dtn)
    R.assert_integers(m['d_out'], m['x'], *m['w2'])
    R.assert_sum_premise(ref.absw, 'dW1')
    R.assert_sum_premise(ref.absb, 'db1')
    assert_w2_premise(m, dtn)
    if content == 'rounding':
        R.assert_rounding_premise(ref.exact, dtn, 'd_hid')
    else:
        R.assert_representable(ref.exact, dtn, 'd_hid')
    call = WGrad(case, dtn, drop, m, ref)
    assert L.dbx_heads1_wgrad_gen_ok(call.dt, C.byref(call.xv), call.nh) == 1
    if dtn != 'f32':
        kname, splits = C.create_string_buffer(64), C.c_int32(0)
        check(L.dbx_conv_wgrad_plan(call.dt, C.byref(call.dz), C.byref(call.xv), 1, 1, kname, 64, C.byref(splits)))
        assert (kname.value.decode(), splits.value) == ('wgrad_wide2_kernel<%s>' % dtn, pl['splits']), (kname.value, splits.value, pl)
        assert call.sbytes == pl['scratch'], (call.sbytes, pl)
    what = 'dbx_heads1_wgrad_gen %s %s %s %s' % (name, dtn, drop, content)
    call.fresh()
    check(call.call())
    first = call.verify(what)
    call.fresh()
    check(call.call())
    second = call.verify(what + ' (second call)')
    assert all(torch.equal(a, b) for a, b in zip(first, second)), 'the second call differs from the first'


@pytest.mark.parametrize('name,drop,dtn', [(n, d, t) for n in R.WG for d in ('none', 'hash') for t in ('bf16', 'f16', 'f32')])
def test_wgrad_gen_is_exact(name, drop, dtn):
    run_wg(name, dtn, drop)


@pytest.mark.parametrize('drop,dtn', [(d, t) for d in ('none', 'hash') for t in ('bf16', 'f16', 'f32')])
def test_wgrad_gen_takes_every_impulse_from_its_pixel(drop, dtn):
    case = R.WG['b-ragged-seam']
    px, hw = set(R.wg_impulse_pixels(case, CUS)), case.h * case.w
    assert {0, hw - 1, hw, 2 * hw - 1, 2 * hw, case.n * hw - 1} <= px
    run_wg('b-ragged-seam', dtn, drop, 'impulse')


@pytest.mark.parametrize('drop,dtn', [(d, t) for d in ('none', 'hash') for t in R.DTN16])
def test_wgrad_gen_rounds_the_hidden_gradient_once_to_nearest_even(drop, dtn):
    run_wg('b-min', dtn, drop, 'rounding')


@pytest.mark.parametrize('dtn', R.DTN16)
def test_wgrad_gen_refuses_a_frame_of_fewer_than_32_columns(dtn):
    case = R.WG['b-min']._replace(name='b-narrow', w=29)
    m = R.make_wg(case, 'hash', 'dense', CUS)
    call = WGrad(case, dtn, 'hash', m, R.wg_reference(m, dtn))
    assert case.w + 2 * case.pad == 31 and not R.wgrad_plan_ref(case, CUS)['ok']
    assert call.L.dbx_heads1_wgrad_gen_ok(call.dt, C.byref(call.xv), call.nh) == 0
    call.fresh()
    assert call.call() != 0 and b'32 columns' in call.L.dbx_last_error()
    call.verify('refused call', written=False)
    assert bool((call.scratch == 0xFF).all()), 'a refused call wrote its scratch'


@pytest.mark.parametrize('dtn', R.DTN16)
def test_wgrad_gen_refuses_2_to_24_pixels_and_more(dtn):
    """The generator multiplies the compact pixel index with a 24-bit multiply: fewer than 2**24 pixels.  The query on either side of the
    bound (it follows no pointer), then the call itself on a 4096 x 4096 view laid over small buffers: refused before anything is
    read or written."""
    L, dt, tdt = _lib.lib(), _lib.DTYPE_ID[dtn], TDT[dtn]
    for n, h, w, ok in ((1, 4096, 4095, 1), (1, 4096, 4096, 0), (2, 2048, 4096, 0), (4095, 64, 64, 1), (4096, 64, 64, 0), (64, 60, 60, 1)):
        assert (n * h * w < 2 ** 24) == bool(ok)
        for nh in (1, 4):
            xv = View(None, n, h, w, 1, 768, 512, 256)
            assert L.dbx_heads1_wgrad_gen_ok(dt, C.byref(xv), nh) == ok, (n, h, w, nh)
            assert L.dbx_heads1_wgrad_gen_ok(_lib.F32, C.byref(xv), nh) == 1          # (the fp32 instantiation multiplies in 64 bits)
    d_out = flat('d_out', 64, 8, tdt, SENTINEL, np.zeros((64, 8))).upload()
    x = flat('x', 64, 256, tdt, SENTINEL, np.ones((64, 256))).upload()
    w2 = flat('W2', 8, 512, torch.float32, SENTINEL, np.ones((8, 512))).upload()
    dw, db = Rows('dW1', 512, 300, FILL).upload(), Planes('db1', 1, 512, 1, FILL).upload()
    scratch = nan_scratch(1024)
    dv = View(C.c_void_p(d_out.ptr()), 1, 4096, 4096, 0, 8, 0, 8)
    xv = View(C.c_void_p(x.ptr()), 1, 4096, 4096, 1, 256, 0, 256)
    rc = L.dbx_heads1_wgrad_gen(dt, C.byref(dv), C.byref(xv), (C.c_void_p * 1)(w2.ptr()), (C.c_int32 * 1)(8), 1, 1, R.SEED, 256, C.c_void_p(dw.ptr()), 300, 44,
                                C.c_void_p(db.ptr()), C.c_void_p(scratch.data_ptr()), stream_ptr())
    assert rc != 0 and b'2**24 pixels' in L.dbx_last_error(), L.dbx_last_error()
    torch.cuda.synchronize()
    for b in (d_out, x, w2, dw, db):
        assert_holds(b, what='refused call')
    assert bool((scratch == 0xFF).all()), 'a refused call wrote its scratch'


# ================================================================================================ C: dbx_heads1_dgrad_gen
DG_PREMISE = {
    'c-partial': lambda P, p: P < 256 and P <= 128 and p['ntiles'] == 1,
    'c-256': lambda P, p: P == 256 and p['ntiles'] == 1,
    'c-513': lambda P, p: P % 256 == 1 and p['ntiles'] == 3,
    'c-nh4': lambda P, p: p['ntiles'] == 2 and P % 256 != 0,
    'c-two-tiles': lambda P, p: CUS < p['ntiles'] < 2 * CUS and P % 256 != 0 and (p['most'], p['least']) == (2, 1) and p['grid'] == CUS,
    'c-three-tiles': lambda P, p: 2 * CUS < p['ntiles'] < 3 * CUS and P % 256 != 0 and (p['most'], p['least']) == (3, 2) and p['grid'] == CUS,
}


class DGrad:
    def __init__(self, case, dtn, drop, m, ref):
        self.L, self.case, self.dtn, self.m, self.ref = _lib.lib(), case, dtn, m, ref
        self.dt, self.tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
        L, dt = self.L, self.dt
        n, h, w, nh = case.n, case.h, case.w, len(case.ks)
        self.nh = nh
        self.d_out = Buf('d_out', n, h, w, 0, case.slot * nh, self.tdt, SENTINEL, slots(m['d_out'], case.slot).reshape(n, h, w, -1)).upload()
        self.gate = Buf('gate', n, h, w, case.gpad, 256, self.tdt, SENTINEL, m['gate'].reshape(n, h, w, 256)).upload()
        self.w2 = w2_bufs(m, dtn)
        self.w1 = [flat('W1[%d]' % i, 512, 768, torch.float32, SENTINEL, m['w1'][i]).upload() for i in range(nh)]
        es = _lib.ESIZE[dt]
        self.img = torch.zeros(L.dbx_conv_packed_elems(C.byref(ConvDesc(dt, 1, 1, 0, 512 * nh, 256, 0, 0))) * es, dtype=torch.uint8, device='cuda')
        for i, b in enumerate(self.w1):                    # W1^T restricted to the input channels [512, 768): fragment order (16-bit) / plain rows (fp32)
            check(L.dbx_pack_weight(dt, 5 if es == 2 else 1, C.c_void_p(b.ptr()), 512, 768, 1, 1, C.c_void_p(self.img.data_ptr()), 256, 512 * nh, -512, 512 * i, stream_ptr()))
        torch.cuda.synchronize()
        self.img0 = self.img.clone()
        self.use_hash, self.seed = (1, R.SEED) if drop == 'hash' else (0, 0)
        self.karr = (C.c_int32 * nh)(*case.ks)
        self.wp = (C.c_void_p * nh)(*[b.ptr() for b in self.w2])
        self.want = None

    def run(self, what):
        case = self.case
        n, h, w = case.n, case.h, case.w
        y = Buf('y', n, h, w, case.ypad, case.y_ld, self.tdt, HALO, FILL).upload()
        check(self.L.dbx_heads1_dgrad_gen(self.dt, C.byref(self.d_out.view()), self.wp, self.karr, self.nh, self.use_hash, self.seed, C.c_void_p(self.img.data_ptr()),
                                          C.byref(y.view(c=256, c_off=case.y_off)), C.byref(self.gate.view()), stream_ptr()))
        torch.cuda.synchronize()
        for b in [self.d_out, self.gate] + self.w2 + self.w1:
            assert_holds(b, what=what + ': input')
        assert torch.equal(self.img, self.img0), what + ': the weight image changed'
        if self.want is None:
            self.want = y.with_interior(self.ref.d_x.reshape(n, h, w, 256), c_off=case.y_off)
        assert_holds(y, self.want, what=what)
        return y.dev


def run_dg(name, dtn, drop, content='dense'):
    case = DG[name]
    P = case.n * case.h * case.w
    pl = R.dgrad_plan_ref(P, CUS)
    assert DG_PREMISE[name](P, pl), '%s: at %d CUs: %d pixels, %s' % (name, CUS, P, pl)
    m = R.make_dg(case, drop, content, CUS)
    ref = R.dg_reference(m, dtn)
    R.assert_integers(m['d_out'], m['w1t'], m['gate'], *m['w2'])
    R.assert_sum_premise(ref.absum, 'd_x')
    assert_w2_premise(m, dtn)
    g = m['gate']
    assert (g == 0).any() and (g < 0).any() and 0.3 < float((g > 0).mean()) < 0.5, 'the gate holds zeros, negatives and positives'
    if content == 'rounding':
        R.assert_rounding_premise(ref.exact, dtn, 'd_x')
    else:
        R.assert_representable(ref.exact, dtn, 'd_x')
    call = DGrad(case, dtn, drop, m, ref)
    what = 'dbx_heads1_dgrad_gen %s %s %s %s' % (name, dtn, drop, content)
    first = call.run(what)
    second = call.run(what + ' (second call)')
    assert torch.equal(first, second), 'the second call differs from the first'


@pytest.mark.parametrize('name,drop,dtn', [(n, d, t) for n in R.DG_SMALL for d in ('none', 'hash') for t in ('bf16', 'f16', 'f32')])
def test_dgrad_gen_is_exact_on_the_small_cases(name, drop, dtn):
    run_dg(name, dtn, drop)


@pytest.mark.parametrize('drop,dtn', [(d, t) for d in ('none', 'hash') for t in R.DTN16])
def test_dgrad_gen_is_exact_where_workgroups_walk_one_or_two_tiles(drop, dtn):
    run_dg('c-two-tiles', dtn, drop)


@pytest.mark.parametrize('drop,dtn', [(d, t) for d in ('none', 'hash') for t in R.DTN16])
def test_dgrad_gen_takes_every_impulse_from_its_pixel(drop, dtn):
    case = DG['c-two-tiles']
    px, P = set(R.dg_impulse_pixels(case, CUS)), case.n * case.h * case.w
    assert {0, 255, 256, 256 * CUS - 1, 256 * CUS, P - 1} <= px
    run_dg('c-two-tiles', dtn, drop, 'impulse')


@pytest.mark.parametrize('drop,dtn', [(d, t) for d in ('none', 'hash') for t in R.DTN16])
def test_dgrad_gen_is_exact_where_workgroups_walk_two_or_three_tiles(drop, dtn):
    run_dg('c-three-tiles', dtn, drop)


@pytest.mark.parametrize('drop,dtn', [(d, t) for d in ('none', 'hash') for t in R.DTN16])
def test_dgrad_gen_rounds_once_to_nearest_even(drop, dtn):
    run_dg('c-256', dtn, drop, 'rounding')
