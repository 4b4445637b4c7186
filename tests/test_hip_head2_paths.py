"""Every path of the stage-2 heads backward (csrc/aux_ops.hip) against the float64 reference of tests/heads_ref.py, bit for bit.

Kernels and the case that pins each path (plans asserted through dbx_head2_backward_up_plan, the library's own read-only query, and
against their restatement in heads_ref.plan_ref):
  head2_backward_up_kernel<T,KJ>  one workgroup per row   [up-one-half: KJ 1 / 2 / 4 / 8 in four launches, k = 3 under KJ = 4]
                                  two half-row workgroups [up-two-halves-ring: columns [0, 16) and [14, 33), boundary 15; 9 source rows
                                                           against the LDS ring of 8: flushes at 4 and 8 rows plus the tail]
                                  a workgroup walking more than one image [up-stride-2h: the k = 4 launch has 16 groups for 17 images,
                                                           workgroup 0 walks images 0 and 16 (10 rows, the others 5: odd against the
                                                           pipeline depth 2); up-stride-1h: one launch of four heads, 16 groups]
                                  the workload's split    [up-workload: 60 -> 30, 31 + 31 columns, boundary 30; interval comparison]
                                  d_hid->ptr == NULL      [up-nostore: W2 rounded to T, no hidden gradient stored; mask refused]
  head2_wgrad_reduce_kernel       per-head partial-block counts 34 / 32 / 34 in one call [up-stride-2h]; the four-way unrolled loop
                                  (64 blocks > 48) [up-reduce-unrolled]
  the two passes inside dbx_head2_backward_up   [up-fallback: a 65-pixel row; up-one-half in f32]
  head2_wgrad_kernel<T,DG>, head2_dgrad_kernel  at the 512-workgroup cap [wgrad-cap: 513 rows, 6 pixels per workgroup cutting the
                                  5-pixel rows and the images, 84 empty workgroups; nh = 3 leaves a quarter of the lanes idle], and
                                  on the first two geometries, through dbx_head2_dgrad, dbx_head2_wgrad and dbx_head2_backward --
                                  each compared with the reference, not with one another.

Per case: the premise of a zero tolerance from the reference alone (heads_ref.assert_premise); d_out on a frame of pad 1 with
16-channel slots whose channels [k, 8) are zero and [8, 16) hold 1000, hid on pad 0, d_g44 on pad 1; guard bands round every buffer,
outputs starting at 7; the scratch exactly dbx_head2_wgrad_scratch_bytes plus a tail that must stay intact; WHOLE buffers compared
(halo and guards included), inputs unchanged, guard floats behind each [k][512] / [k] gradient; a second call into fresh buffers
bitwise equal.  Dropout as none / hash / mask.  On the non-dyadic workload geometry d_g44 must lie in the derived interval
[round_T(ref - E), round_T(ref + E)] (heads_ref.interval: wider than one value at 0.09 - 0.57 % of the outputs); everything else is
exact.  Impulse variants (one per up path): single ones in d_out at the corners of the first and last image, either side of every
image seam a workgroup crosses, either side of the ownership boundary and in column W - 1, under W2 without zeros -- a failure names
the buffer, pixel and channel.

Cost.  References: NumPy float64 on the CPU, one per (case, dropout form, content), shared by the dtypes; only up-workload takes more
than 0.1 s (about 1 s).  On an MI355X host with 16 threads the 103 tests of this file took 16.0 s in all, references included; the
slowest five: up-nostore up-workload-hash-bf16 0.89 s, -hash-f16 0.86 s, up-workload-hash-bf16 0.72 s, up-nostore
up-workload-none-bf16 0.72 s, -none-f16 0.70 s (7200 pixels x 2048 channels: building and comparing the 30 MB buffers on the host).
tests/test_heads_ref.py (CPU, 56 tests) takes 28 s, of which the up-workload references and their no-store forms are 17 s."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads_ref as R                                   # noqa: E402
from framed_buf import Buf, assert_holds                # noqa: E402

from densebox_amd import _lib                           # noqa: E402
from densebox_amd._lib import View, check, stream_ptr   # noqa: E402

pytestmark = pytest.mark.gpu
if 'DBX_HEAD2_UP' in os.environ or 'DBX_HEAD2_UP_SPLIT' in os.environ:
    pytest.skip('this process forces a kernel selection', allow_module_level=True)

TDT = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}
SENTINEL, FILL, SLOT, TAIL = 1000.0, 7.0, 16, 4096          # 1000 and 7 are exact in bf16, f16 and fp32
DROPS = ['none', 'hash', 'mask']


class Call:
    """Device buffers of one case, the four entry points on them, and the comparison with the reference."""

    def __init__(self, case, dtn, drop, m, nostore=False):
        self.L, self.case, self.dtn, self.drop, self.m, self.nostore = _lib.lib(), case, dtn, drop, m, nostore
        self.dt, self.tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
        n, h, w, ks = case.n, case.h, case.w, case.ks
        self.nh = nh = len(ks)
        dslots = np.full((n * h * w, nh, SLOT), SENTINEL)
        dslots[:, :, :8] = m['d_out']
        self.d_out = Buf('d_out', n, h, w, 1, SLOT * nh, self.tdt, SENTINEL, dslots.reshape(n, h, w, SLOT * nh)).upload()
        self.hid = Buf('hid', n, h, w, 0, 512 * nh, self.tdt, SENTINEL, m['hid'].reshape(n, h, w, 512 * nh)).upload()
        self.w2 = [Buf('W2[%d]' % i, k, 1, 1, 0, 512, torch.float32, SENTINEL, a.reshape(k, 1, 1, 512)).upload()
                   for i, (k, a) in enumerate(zip(ks, m.get('w2_raw', m['w2'])))]
        self.mask = None
        if drop == 'mask':
            self.mask = Buf('mask', n * h * w, 1, 1, 0, 512 * nh, torch.uint8, 255, m['mask'].reshape(n * h * w, 1, 1, 512 * nh)).upload()
        self.use_hash, self.seed = (1, R.SEED) if drop == 'hash' else (0, 0)
        self.sbytes = int(self.L.dbx_head2_wgrad_scratch_bytes(nh, n * h))
        assert self.sbytes == min(n * h, 512) * (nh * 8 * 512 + 32) * 4
        self.karr = (C.c_int32 * nh)(*ks)
        self.wp = (C.c_void_p * nh)(*[b.ptr() for b in self.w2])
        self.fresh()

    def fresh(self):
        case, nh, ref = self.case, self.nh, self.m['ref']
        n, h, w = case.n, case.h, case.w
        self.d_hid = Buf('d_hid', n, h, w, 0, 512 * nh, self.tdt, FILL).upload()
        self.d_g44 = Buf('d_g44', n, case.hs, case.ws, 1, 512 * nh, self.tdt, FILL).upload() if case.hs else None
        self.dw = [Buf('dW2[%d]' % i, k, 1, 1, 0, 512, torch.float32, FILL).upload() for i, k in enumerate(case.ks)]
        self.db = [Buf('db2[%d]' % i, 1, 1, 1, 0, k, torch.float32, FILL).upload() for i, k in enumerate(case.ks)]
        self.scratch = torch.full((self.sbytes + TAIL,), 0xA5, dtype=torch.uint8, device='cuda')
        self.dwp = (C.c_void_p * nh)(*[b.ptr() for b in self.dw])
        self.dbp = (C.c_void_p * nh)(*[b.ptr() for b in self.db])
        self.want_hid = self.d_hid.with_interior(ref.d_hid.reshape(n, h, w, 512 * nh))
        self.want_dw = [b.with_interior(a.reshape(-1, 1, 1, 512)) for b, a in zip(self.dw, ref.dw)]
        self.want_db = [b.with_interior(a.reshape(1, 1, 1, -1)) for b, a in zip(self.db, ref.db)]

    def mask_args(self):
        return (C.c_void_p(self.mask.ptr()) if self.mask else None), 512 * self.nh, self.use_hash, self.seed

    # ---- the entry points
    def dgrad(self):
        return self.L.dbx_head2_dgrad(self.dt, C.byref(self.d_out.view()), self.wp, self.karr, self.nh, C.byref(self.d_hid.view()), *self.mask_args(),
                                      stream_ptr())

    def wgrad(self):
        return self.L.dbx_head2_wgrad(self.dt, C.byref(self.d_out.view()), C.byref(self.hid.view()), self.karr, self.nh, self.dwp, self.dbp,
                                      C.c_void_p(self.scratch.data_ptr()), stream_ptr())

    def backward(self):
        return self.L.dbx_head2_backward(self.dt, C.byref(self.d_out.view()), C.byref(self.hid.view()), self.wp, self.karr, self.nh,
                                         C.byref(self.d_hid.view()), *self.mask_args(), self.dwp, self.dbp, C.c_void_p(self.scratch.data_ptr()),
                                         stream_ptr())

    def backward_up(self):
        return self.L.dbx_head2_backward_up(self.dt, C.byref(self.d_out.view()), C.byref(self.hid.view()), self.wp, self.karr, self.nh,
                                            C.byref(self.d_hid.view(null=self.nostore)), *self.mask_args(), self.dwp, self.dbp,
                                            C.c_void_p(self.scratch.data_ptr()), C.byref(self.d_g44.view()), stream_ptr())

    # ---- comparison
    def verify(self, what, hid=False, wgrad=False, g44=False):
        """Outputs named True hold the reference, the others still their fill; inputs, guards and the scratch tail are untouched."""
        torch.cuda.synchronize()
        for b in [self.d_out, self.hid] + self.w2 + ([self.mask] if self.mask else []):
            assert_holds(b, what=what + ': input')
        assert bool((self.scratch[self.sbytes:] == 0xA5).all()), what + ': the tail behind the scratch was written'
        assert_holds(self.d_hid, self.want_hid if hid else None, what=what)
        for b, want in zip(self.dw + self.db, self.want_dw + self.want_db):
            assert_holds(b, want if wgrad else None, what=what)
        if self.d_g44 is not None:
            case, m = self.case, self.m
            if not g44:
                assert_holds(self.d_g44, what=what)
            elif case.dyadic:
                assert_holds(self.d_g44, self.d_g44.with_interior(R.round_np(m['g44'], self.dtn)), what=what)
            else:
                lo, hi, share = R.interval(m['g44'], m['g44_abs'], self.dtn)
                assert share < 0.01
                assert_holds(self.d_g44, lo=self.d_g44.with_interior(lo), hi=self.d_g44.with_interior(hi), what=what)

    def outputs(self):
        return [b.dev.clone() for b in [self.d_hid] + self.dw + self.db + ([self.d_g44] if self.d_g44 is not None else [])]


def query(case, dtn):
    L = _lib.lib()
    nh = len(case.ks)
    hv = View(None, case.n, case.h, case.w, 0, 512 * nh, 0, 512 * nh)
    gv = View(None, case.n, case.hs, case.ws, 1, 512 * nh, 0, 512 * nh)
    out = _lib.Head2UpPlan()
    check(L.dbx_head2_backward_up_plan(_lib.DTYPE_ID[dtn], C.byref(hv), C.byref(gv), (C.c_int32 * nh)(*case.ks), nh, C.byref(out)))
    half = [R.Half(*[getattr(out.half[i], f) for f in R.Half._fields]) for i in range(2)]
    launches = [R.Launch(*[getattr(out.launch[i], f) for f in R.Launch._fields]) for i in range(out.launches)]
    assert L.dbx_head2_backward_up_fused(_lib.DTYPE_ID[dtn], C.byref(hv), C.byref(gv)) == out.fused
    return R.Plan(out.fused, out.halves, half, launches)


# what each up case is there for, asserted on the LIBRARY's plan (16-bit types)
PREMISE = {
    'up-one-half': lambda p, c: p.fused == 1 and p.halves == 1 and [l.kj for l in p.launches] == [1, 2, 4, 8] and 3 in c.ks,
    'up-two-halves-ring': lambda p, c: p.fused == 1 and p.halves == 2 and p.half[0][:4] == (0, 16, 0, 15) and p.half[1][:4] == (14, 19, 15, 33)
    and c.hs > 8 and [(l.kj, l.heads) for l in p.launches] == [(1, 1), (4, 2), (8, 1)],
    'up-stride-2h': lambda p, c: p.halves == 2 and [(l.kj, l.groups, l.blocks) for l in p.launches] == [(1, 17, 34), (4, 16, 32), (8, 17, 34)]
    and p.launches[1].groups < c.n and ((c.n + 15) // 16 * c.h) % 2 == 0 and c.h % 2 == 1,
    'up-stride-1h': lambda p, c: p.halves == 1 and [(l.kj, l.heads, l.groups, l.blocks) for l in p.launches] == [(4, 4, 16, 16)] and 16 < c.n,
    'up-reduce-unrolled': lambda p, c: p.halves == 2 and [(l.groups, l.blocks) for l in p.launches] == [(32, 64)] * 2 and 32 < c.n
    and all(l.blocks > 48 for l in p.launches),
    'up-workload': lambda p, c: p.halves == 2 and p.half[0][:4] == (0, 31, 0, 30) and p.half[1][:4] == (29, 31, 30, 60)
    and [(l.kj, l.heads) for l in p.launches] == [(1, 1), (4, 2), (8, 1)],
    'up-fallback': lambda p, c: p.fused == 0 and p.launches == [] and c.w > 64,
}


def assert_plan(case, dtn):
    plan = query(case, dtn)
    assert plan == R.plan_ref(case, dtn), (plan, R.plan_ref(case, dtn))
    if dtn == 'f32':
        assert plan.fused == 0 and plan.launches == []
    else:
        assert PREMISE[case.name](plan, case), (case.name, plan)
    return plan


def premise(case, m):
    R.assert_premise(m['ref'], m.get('g44'), m.get('g44_abs'), case.dyadic, (case.n, case.h, case.w, case.hs, case.ws))


def run_up(case, dtn, drop, content='dense', nostore=False):
    m = R.make(case, drop, content, w2_dtn=dtn if nostore else None)
    premise(case, m)
    plan = assert_plan(case, dtn)
    if nostore:                                             # the rounding is pinned: the reference with the fp32 W2 differs
        assert plan.fused == 1 and (R.round_np(m['ref_raw'].d_hid, dtn) != m['ref'].d_hid).any()
    call = Call(case, dtn, drop, m, nostore)
    check(call.backward_up())
    call.verify('dbx_head2_backward_up', hid=not nostore, wgrad=True, g44=True)
    first = call.outputs()
    call.fresh()
    check(call.backward_up())
    call.verify('dbx_head2_backward_up (second call)', hid=not nostore, wgrad=True, g44=True)
    assert all(torch.equal(a, b) for a, b in zip(first, call.outputs())), 'the second call differs from the first'


UP = ['up-one-half', 'up-two-halves-ring', 'up-stride-2h', 'up-stride-1h', 'up-reduce-unrolled', 'up-workload']


@pytest.mark.parametrize('name,drop,dtn', [(n, d, t) for n in UP for d in DROPS for t in ('bf16', 'f16')])
def test_backward_up_one_pass(name, drop, dtn):
    run_up(R.CASES[name], dtn, drop)


@pytest.mark.parametrize('name,drop,dtn', [(n, d, t) for n in ('up-two-halves-ring', 'up-workload') for d in ('hash', 'none') for t in ('bf16', 'f16')])
def test_backward_up_without_a_stored_hidden_gradient(name, drop, dtn):
    """d_hid->ptr == NULL, the default 16-bit training form: W2 rounded to the compute dtype, d_hid never written."""
    run_up(R.CASES[name], dtn, drop, nostore=True)


@pytest.mark.parametrize('dtn', ['bf16', 'f16'])
def test_backward_up_without_d_hid_refuses_a_byte_mask(dtn):
    case = R.CASES['up-two-halves-ring']
    m = R.make(case, 'mask')
    call = Call(case, dtn, 'mask', m, nostore=True)
    rc = call.backward_up()
    assert rc == -1 and b'without d_hid' in call.L.dbx_last_error()
    call.verify('refused call')
    assert bool((call.scratch == 0xA5).all())


@pytest.mark.parametrize('name,drop,dtn', [('up-fallback', d, t) for d in DROPS for t in ('bf16', 'f16')] + [('up-one-half', d, 'f32') for d in DROPS])
def test_backward_up_two_passes(name, drop, dtn):
    run_up(R.CASES[name], dtn, drop)


@pytest.mark.parametrize('name,drop,dtn', [(n, d, t) for n in ('up-stride-1h', 'up-stride-2h', 'up-fallback') for d in ('none', 'hash')
                                           for t in ('bf16', 'f16')])
def test_backward_up_impulses(name, drop, dtn):
    case = R.CASES[name]
    px = R.impulse_pixels(case)
    n, h, w = case.n, case.h, case.w
    assert {(0, 0, 0), (0, h - 1, w - 1), (n - 1, 0, 0), (n - 1, h - 1, w - 1)} <= set(px) and any(x == w - 1 and 0 < y < h - 1 for _, y, x in px)
    plan = R.plan_ref(case, dtn)
    if plan.fused:
        g = min(l.groups for l in plan.launches)
        assert g < n and {(0, h - 1, w - 1), (g, 0, 0)} <= set(px)          # the seam workgroup 0 crosses
        if plan.halves == 2:
            b = plan.half[0].own_hi
            assert {(0, 1, b - 1), (0, 1, b)} <= set(px)
    else:
        assert {(0, h - 1, w - 1), (1, 0, 0)} <= set(px)
    run_up(case, dtn, drop, content='impulse')


ENTRY = ['up-one-half', 'up-two-halves-ring', 'wgrad-cap-3h', 'wgrad-cap-1h']


@pytest.mark.parametrize('name,drop,dtn', [(n, d, t) for n in ENTRY for d in DROPS for t in ('bf16', 'f16', 'f32')])
def test_separate_entry_points(name, drop, dtn):
    """dbx_head2_dgrad, dbx_head2_wgrad and dbx_head2_backward, each against the reference (the up-sampling geometry plays no part)."""
    case = R.CASES[name]._replace(hs=None, ws=None)
    m = R.make(case, drop)
    R.assert_premise(m['ref'])
    if name.startswith('wgrad-cap'):                         # 513 rows: the library caps at 512 workgroups (its scratch says so)
        blocks, per, empty = R.wgrad_blocks(case)
        nh = len(case.ks)
        assert (blocks, per, empty) == (512, 6, 84) and case.n * case.h == 513 and per > case.w
        assert _lib.lib().dbx_head2_wgrad_scratch_bytes(nh, case.n * case.h) == 512 * (nh * 4096 + 32) * 4 == \
            _lib.lib().dbx_head2_wgrad_scratch_bytes(nh, 512)
    call = Call(case, dtn, drop, m)
    check(call.dgrad())
    call.verify('dbx_head2_dgrad', hid=True)
    first = call.outputs()
    call.fresh()
    check(call.dgrad())
    call.verify('dbx_head2_dgrad (second call)', hid=True)
    assert all(torch.equal(a, b) for a, b in zip(first, call.outputs()))
    if drop == 'none':                                      # (the weight gradient alone knows no dropout)
        call.fresh()
        check(call.wgrad())
        call.verify('dbx_head2_wgrad', wgrad=True)
        first = call.outputs()
        call.fresh()
        check(call.wgrad())
        call.verify('dbx_head2_wgrad (second call)', wgrad=True)
        assert all(torch.equal(a, b) for a, b in zip(first, call.outputs()))
    call.fresh()
    check(call.backward())
    call.verify('dbx_head2_backward', hid=True, wgrad=True)
    first = call.outputs()
    call.fresh()
    check(call.backward())
    call.verify('dbx_head2_backward (second call)', hid=True, wgrad=True)
    assert all(torch.equal(a, b) for a, b in zip(first, call.outputs()))
