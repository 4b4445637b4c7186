"""Kernel-level GPU parity through the C ABI: conv forward / weight-gradient kernels in f16 and bf16 against a torch
fp32 computation on the SAME rounded operands (so the only difference is fp32 summation order), for every tile/variant
the dispatcher can pick (register-staged v1, LDS-DMA ring, small-Cin, per-tap wgrad, all-taps 3x3 wgrad)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from densebox_amd import _lib
from densebox_amd._lib import View, ConvDesc, check, ptr, stream_ptr

pytestmark = pytest.mark.gpu
TDT = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}


def framed(x_nchw, pad, tdt):
    """NCHW fp32 -> zero-framed NHWC tensor (with zero guard bands) + the View."""
    n, c, h, w = x_nchw.shape
    hp, wp = h + 2 * pad, w + 2 * pad
    guard = max(8 * wp, 576 + 4 * wp) * c
    flat = torch.zeros(2 * guard + n * hp * wp * c, dtype=tdt, device='cuda')
    t = flat[guard:guard + n * hp * wp * c].view(n, hp, wp, c)
    t[:, pad:pad + h, pad:pad + w] = x_nchw.permute(0, 2, 3, 1).to(tdt)
    return flat, t, View(C.c_void_p(t.data_ptr()), n, h, w, pad, c, 0, c)


def pack(L, dt, w, cin_pad, cout_pad, mode=0):
    d = ConvDesc(dt, w.shape[2], w.shape[3], 0, cin_pad, cout_pad, 0)
    out = torch.zeros(L.dbx_conv_packed_elems(C.byref(d)) * _lib.ESIZE[dt], dtype=torch.uint8, device='cuda')
    check(L.dbx_pack_weight(dt, mode, ptr(w), w.shape[0], w.shape[1], w.shape[2], w.shape[3], ptr(out), cout_pad, cin_pad, 0, 0,
                            stream_ptr()))
    return out


CONV_CASES = [  # n, h, w, cin, cout, k, pad; the kernel names are what dbx_conv_plan reports at 256 CUs (tests/test_hip_conv_paths.py asserts them)
    (2, 20, 28, 64, 64, 3, 1), (3, 17, 23, 128, 256, 3, 1), (1, 30, 30, 512, 512, 3, 1),      # conv3x3_band_kernel<128,64>
    (2, 15, 15, 768, 1024, 1, 0),     # conv_igemm_dma_kernel<256,256>
    (2, 14, 14, 64, 64, 5, 0),        # conv_igemm_dma_kernel<256,64>
    (1, 33, 9, 256, 128, 3, 1),       # conv3x3_band_kernel<256,128>
    (10, 53, 100, 64, 64, 3, 1),      # ragged 8x32 tiles of the weights-stationary 64->64 kernel: conv3x3_c64p_kernel<256,64>
    (10, 240, 240, 64, 128, 3, 1),    # conv2_1 at batch 64: conv3x3_c64p_kernel<256,64>, one 64-cout slice per workgroup (conv3x3_band_kernel<512,128> under DBX_C64P_WIDE=0)
    (10, 240, 240, 128, 64, 3, 1),    # >= 1024 tiles of 512 pixels: conv3x3_band_kernel<512,64> (conv2_1's data gradient)
    (1, 64, 64, 512, 512, 3, 1),      # single-image maps: conv3x3_band_kernel<144,64>, one workgroup per CU, 5-deep ring (conv4 of a 512 x 512 image; <192,64> under DBX_BAND144=0)
    (1, 128, 128, 256, 256, 3, 1),    # ... conv3x3_band_kernel<144,128>, 4-deep ring (conv3; <192,128> under DBX_BAND144=0)
    (1, 64, 60, 256, 512, 3, 1),      # conv3x3_band_kernel<144,64>
    (1, 256, 256, 64, 128, 3, 1),     # 261 tiles of 256 pixels -> 232 of 288: conv3x3_band_kernel<288,128> (conv2_1 of a 512 x 512 image)
]


_V1_RUN = {}


def _v1_outcomes(tmp_path_factory):
    """The library reads DBX_CONV_VARIANT once per process, so the `v1` cases (register-staged kernel forced everywhere) run in ONE child
    pytest with DBX_CONV_VARIANT=1, started by the first of them; returns {test name: 'passed' | 'skipped' | 'failure: ...'} from its
    JUnit report, plus '_run': (exit code, output tail).  The child starts at most once per session: a time-out or any other exception
    is recorded before it propagates, and the remaining cases then fail on that record instead of starting the child again."""
    if not _V1_RUN:
        import subprocess
        import sys
        import xml.etree.ElementTree as ET
        report = tmp_path_factory.mktemp('v1') / 'v1.xml'
        try:
            r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-m', 'gpu', '-k',
                                'test_conv_forward_kernel and v1', '--junitxml', str(report)], capture_output=True, text=True,
                               env=dict(os.environ, DBX_CONV_VARIANT='1'), timeout=1800)
        except BaseException as e:
            _V1_RUN['_run'] = (None, 'the DBX_CONV_VARIANT=1 child did not complete: %r' % e)
            raise
        if report.exists():
            for tc in ET.parse(str(report)).iter('testcase'):
                outcome = 'passed'
                for el in tc:
                    if el.tag in ('failure', 'error'):
                        outcome = '%s: %s' % (el.tag, (el.get('message') or '')[:1000])
                    elif el.tag == 'skipped':
                        outcome = 'skipped'
                _V1_RUN[tc.get('name')] = outcome
        _V1_RUN['_run'] = (r.returncode, r.stdout[-3000:] + r.stderr[-2000:])
    return _V1_RUN


@pytest.mark.parametrize('variant', ['dma', 'v1'])
@pytest.mark.parametrize('dtn', ['bf16', 'f16'])
@pytest.mark.parametrize('case', CONV_CASES)
def test_conv_forward_kernel(case, dtn, variant, monkeypatch, request, tmp_path_factory):
    if variant == 'v1' and os.environ.get('DBX_CONV_VARIANT') != '1':
        # kernel selection is per process: this case's check runs in the DBX_CONV_VARIANT=1 child and must have passed there
        got = _v1_outcomes(tmp_path_factory)
        assert got.get(request.node.name) == 'passed', (request.node.name, got.get(request.node.name), got['_run'])
        return
    if variant == 'dma' and os.environ.get('DBX_CONV_VARIANT') == '1':
        pytest.skip('this process forces the register-staged v1 kernel')
    n, h, w, ci, co, k, pad = case
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    g = torch.Generator(device='cpu').manual_seed(hash(case) % 1000)
    x = torch.randn(n, ci, h, w, generator=g).cuda()
    wt = (torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5).cuda()
    b = torch.randn(co, generator=g).cuda()
    xr, wr = x.to(tdt).float(), wt.to(tdt).float()
    ref = F.relu(F.conv2d(xr, wr, b, padding=pad))
    ho, wo = ref.shape[2], ref.shape[3]
    fx, tx, xv = framed(x, 1, tdt)            # keep the tensors alive: the Views only carry raw pointers
    fy, ty, yv = framed(torch.zeros(n, co, ho, wo), 1, tdt)
    d = ConvDesc(dt, k, k, pad, ci, co, _lib.EPI_BIAS | _lib.EPI_RELU)
    check(L.dbx_conv_forward(C.byref(d), C.byref(xv), ptr(pack(L, dt, wt, ci, co)), ptr(b), C.byref(yv), None, None, 0, stream_ptr()))
    got = ty[:, 1:1 + ho, 1:1 + wo].permute(0, 3, 1, 2).float()
    tol = (2e-2 if dtn == 'bf16' else 3e-3)          # output rounding to the 16-bit type dominates
    assert torch.allclose(got, ref, rtol=tol, atol=tol), (got - ref).abs().max().item()
    if variant == 'dma' and n == 1 and (h, w) in ((64, 64), (128, 128), (256, 256)) and not os.environ.get('DBX_CONV_VARIANT'):
        plan = _lib.ConvPlan()
        check(L.dbx_conv_plan(C.byref(d), C.byref(xv), C.byref(yv), C.byref(plan)))
        small = b',192,' if os.environ.get('DBX_BAND144') == '0' else b',144,'          # (round 6: 144-pixel tiles on six waves)
        assert b'conv3x3_band_kernel' in plan.name and (b',288,' if h == 256 else small) in plan.name, plan.name
    # the zero frame must be untouched
    assert float(ty[:, 0].abs().sum()) == 0 and float(ty[:, :, 0].abs().sum()) == 0
    assert float(ty[:, -1].abs().sum()) == 0 and float(ty[:, :, -1].abs().sum()) == 0


P8_CASES = [  # n, h, w, cin, cout, epilogue kind: the 8-phase implicit-GEMM kernel (conv3x3_p8.hpp), sizes the default plan gives it
    (16, 60, 60, 256, 256, 'relu'),     # 225 tiles of 8 units, one cout tile
    (20, 60, 60, 128, 256, 'gate'),     # 282 tiles: 7- and 8-unit tiles mixed, persistent workgroups with a second tile
    (64, 30, 30, 512, 512, 'relu'),     # conv4 at batch 64: two cout tiles (an XCD keeps to one), 256 tiles of 7 / 8 units
    (12, 50, 90, 128, 256, 'plain'),    # W != H, a ragged last unit (54000 pixels)
    (33, 30, 30, 256, 512, 'gate'),     # 29700 pixels x 2 cout tiles: ragged last unit, image seams inside tiles
    # 128-cout layers: 512-pixel x 128-cout tiles of 14 / 15 / 16 units (conv3x3_p8w_kernel)
    (8, 120, 120, 128, 128, 'relu'),    # 225 tiles of 16 units
    (10, 120, 120, 128, 128, 'gate'),   # 282 tiles of 15 / 16 units, a second tile per workgroup, channel-slice views
    (64, 60, 60, 256, 128, 'gate'),     # conv3_1's data gradient at batch 64: 512 tiles of 14 / 15 units
    (9, 100, 130, 128, 128, 'plain'),   # W != H, ragged last unit
]


@pytest.mark.parametrize('dtn', ['f16', 'bf16'])
@pytest.mark.parametrize('case', P8_CASES)
def test_conv_p8_kernel(case, dtn):
    """conv3x3_p8_kernel against fp32 torch on the rounded operands (bias + ReLU forward, the ReLU-gated data-gradient epilogue, plain),
    the zero frame untouched, and a second launch bitwise equal (the phase program has hand-counted waits: a race shows as a difference)."""
    if os.environ.get('DBX_CONV_VARIANT') or os.environ.get('DBX_P8') == '0':
        pytest.skip('this process forces another kernel')
    n, h, w, ci, co, kind = case
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    g = torch.Generator(device='cpu').manual_seed(hash(case) % 1000)
    x = torch.randn(n, ci, h, w, generator=g).cuda()
    wt = (torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (ci * 9)) ** 0.5).cuda()
    b = torch.randn(co, generator=g).cuda()
    gt = torch.randn(n, co, h, w, generator=g).cuda()
    xr, wr = x.to(tdt).float(), wt.to(tdt).float()
    epi = {'relu': _lib.EPI_BIAS | _lib.EPI_RELU, 'gate': _lib.EPI_GATE, 'plain': _lib.EPI_BIAS}[kind]
    ref = F.conv2d(xr, wr, b if kind != 'gate' else None, padding=1)
    if kind == 'relu':
        ref = F.relu(ref)
    if kind == 'gate':
        ref = ref * (gt.to(tdt).float() > 0)
    # the gated cases read x from a channel slice of a wider frame and write y into one (the fusion concat's slots): c_off / ld of the views
    xo, yo = (64, 128) if kind == 'gate' else (0, 0)
    xw = torch.zeros(n, xo + ci + (64 if xo else 0), h, w, device='cuda')
    xw[:, xo:xo + ci] = x
    fx, tx, xv_all = framed(xw, 1, tdt)
    xv = View(xv_all.ptr, n, h, w, 1, xv_all.ld, xo, ci)
    fg, tg, gv = framed(gt, 1, tdt)
    d = ConvDesc(dt, 3, 3, 1, ci, co, epi)
    plan = _lib.ConvPlan()

    def out_view():
        fy, ty, yv_all = framed(torch.zeros(n, yo + co + (64 if yo else 0), h, w), 1, tdt)
        return fy, ty, View(yv_all.ptr, n, h, w, 1, yv_all.ld, yo, co)
    fy, ty, yv = out_view()
    check(L.dbx_conv_plan(C.byref(d), C.byref(xv), C.byref(yv), C.byref(plan)))
    assert plan.kernel == _lib.K_P8 and (b'conv3x3_p8w_kernel' if co == 128 else b'conv3x3_p8_kernel') in plan.name and not plan.w_frag, plan.name
    wp = pack(L, dt, wt, ci, co)
    outs, keep = [], []
    for _ in range(2):
        fy, ty, yv = out_view()
        check(L.dbx_conv_forward(C.byref(d), C.byref(xv), ptr(wp), ptr(b), C.byref(yv), C.byref(gv) if kind == 'gate' else None, None, 0, stream_ptr()))
        torch.cuda.synchronize()
        outs.append(ty); keep.append(fy)
    if yo:
        assert float(outs[0][..., :yo].abs().sum()) == 0 and float(outs[0][..., yo + co:].abs().sum()) == 0     # neighbouring channel slots untouched
    got = outs[0][:, 1:1 + h, 1:1 + w, yo:yo + co].permute(0, 3, 1, 2).float()
    tol = (2e-2 if dtn == 'bf16' else 3e-3)
    assert torch.allclose(got, ref, rtol=tol, atol=tol), (got - ref).abs().max().item()
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    ty = outs[0]
    assert float(ty[:, 0].abs().sum()) == 0 and float(ty[:, :, 0].abs().sum()) == 0
    assert float(ty[:, -1].abs().sum()) == 0 and float(ty[:, :, -1].abs().sum()) == 0


P8_POOL_CASES = [  # n, h, w, channels, y slot (c_off, extra channels behind): the layers with a MaxPool2d behind them (DenseBox.py:191, :204)
    (16, 60, 60, 256, 0, 0),       # conv3_4-like, 225 tiles of 8 units
    (20, 60, 60, 256, 512, 0),     # ... writing fusion[:, 512:768] (the engine's call): 7- and 8-unit tiles, a second tile per workgroup
    (17, 50, 66, 256, 0, 64),      # W != H, image seams inside tiles, ragged last unit (56100 pixels)
    (8, 120, 120, 128, 0, 0),      # conv2_2-like: the 512 x 128 tiles (conv3x3_p8w_kernel)
    (9, 100, 132, 128, 0, 0),      # ... ragged last unit, W != H
]


@pytest.mark.parametrize('dtn', ['f16', 'bf16'])
@pytest.mark.parametrize('case', P8_POOL_CASES)
def test_conv_p8_pool_epilogue(case, dtn):
    """The 2x2 max-pool in the 8-phase kernels' epilogue (dbx_conv_forward_pool_idx on conv2_2 / conv3_4 shapes): the full map is bitwise the
    un-pooled call's, the pooled map and the arg-max nibbles bitwise what dbx_maxpool2x2_idx makes of that map, write_full = 0 leaves the
    full map untouched, neighbouring channel slots and the frames stay as they were."""
    if os.environ.get('DBX_CONV_VARIANT') or os.environ.get('DBX_P8') == '0' or os.environ.get('DBX_P8_POOL') == '0':
        pytest.skip('this process forces another kernel')
    n, h, w, c, yo, yx = case
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    g = torch.Generator(device='cpu').manual_seed(h * w + c)
    x = torch.randn(n, c, h, w, generator=g).cuda()
    wt = (torch.randn(c, c, 3, 3, generator=g) * (2.0 / (c * 9)) ** 0.5).cuda()
    b = torch.randn(c, generator=g).cuda() * 0.3
    fx, tx, xv = framed(x, 1, tdt)
    wp = pack(L, dt, wt, c, c)
    d = ConvDesc(dt, 3, 3, 1, c, c, _lib.EPI_BIAS | _lib.EPI_RELU)

    def out_view():
        fy, ty, yv_all = framed(torch.zeros(n, yo + c + yx, h, w), 1, tdt)
        return fy, ty, View(yv_all.ptr, n, h, w, 1, yv_all.ld, yo, c)

    def pooled():
        fp, tp, pv = framed(torch.zeros(n, c, h // 2, w // 2), 1, tdt)
        return fp, tp, pv
    nb = L.dbx_maxpool_idx_bytes(n, h, w, c)
    fy, ty, yv = out_view()
    assert L.dbx_conv_pool_fusable(C.byref(d), C.byref(xv), C.byref(yv)) == 1
    plan = _lib.ConvPlan()
    check(L.dbx_conv_plan(C.byref(d), C.byref(xv), C.byref(yv), C.byref(plan)))
    assert plan.kernel == _lib.K_P8, plan.name
    # the two calls
    check(L.dbx_conv_forward(C.byref(d), C.byref(xv), ptr(wp), ptr(b), C.byref(yv), None, None, 0, stream_ptr()))
    fp, tp, pv = pooled()
    idx = torch.zeros(nb + 16, dtype=torch.uint8, device='cuda')
    check(L.dbx_maxpool2x2_idx(dt, C.byref(yv), C.byref(pv), ptr(idx), stream_ptr()))
    # one call, both maps + nibbles
    fy2, ty2, yv2 = out_view()
    fp2, tp2, pv2 = pooled()
    idx2 = torch.zeros(nb + 16, dtype=torch.uint8, device='cuda')
    check(L.dbx_conv_forward_pool_idx(C.byref(d), C.byref(xv), ptr(wp), ptr(b), C.byref(yv2), C.byref(pv2), 1, ptr(idx2), stream_ptr()))
    torch.cuda.synchronize()
    assert float(tp.float().abs().sum()) > 0 and int((idx & 3).sum()) > 0 and int((idx & 4).sum()) > 0
    assert torch.equal(fy.view(torch.int16), fy2.view(torch.int16))
    assert torch.equal(fp.view(torch.int16), fp2.view(torch.int16))
    assert torch.equal(idx, idx2), int((idx != idx2).sum())
    ref = F.max_pool2d(F.relu(F.conv2d(x.to(tdt).float(), wt.to(tdt).float(), b, padding=1)), 2)
    got = tp2[:, 1:1 + h // 2, 1:1 + w // 2].permute(0, 3, 1, 2).float()
    tol = 2e-2 if dtn == 'bf16' else 3e-3
    assert torch.allclose(got, ref, rtol=tol, atol=tol), (got - ref).abs().max().item()
    # the pooled map only (conv2_2 in a training step with nibbles, and in inference); without nibbles too
    fy3, ty3, yv3 = out_view()
    fp3, tp3, pv3 = pooled()
    idx3 = torch.zeros(nb + 16, dtype=torch.uint8, device='cuda')
    check(L.dbx_conv_forward_pool_idx(C.byref(d), C.byref(xv), ptr(wp), ptr(b), C.byref(yv3), C.byref(pv3), 0, ptr(idx3), stream_ptr()))
    fy4, ty4, yv4 = out_view()
    fp4, tp4, pv4 = pooled()
    check(L.dbx_conv_forward_pool(C.byref(d), C.byref(xv), ptr(wp), ptr(b), C.byref(yv4), C.byref(pv4), 1, stream_ptr()))
    torch.cuda.synchronize()
    assert float(fy3.float().abs().sum()) == 0 and torch.equal(fp3.view(torch.int16), fp.view(torch.int16)) and torch.equal(idx3, idx)
    assert torch.equal(fy4.view(torch.int16), fy.view(torch.int16)) and torch.equal(fp4.view(torch.int16), fp.view(torch.int16))
    # the pooling backward driven by the fused call's nibbles equals the activation-reading one on the stored map
    dy = torch.randn(n, c, h // 2, w // 2, generator=g).cuda()
    fdy, tdy, dyv = framed(dy, 0, tdt)
    fa, ta, dxa = framed(torch.zeros(n, c, h, w), 1, tdt)
    fb, tb, dxb = framed(torch.zeros(n, c, h, w), 1, tdt)
    yplain = View(yv.ptr, n, h, w, 1, yv.ld, yo, c)
    check(L.dbx_maxpool2x2_bwd(dt, C.byref(yplain), C.byref(dyv), C.byref(dxa), 0, 1, stream_ptr()))
    check(L.dbx_maxpool2x2_bwd_idx(dt, ptr(idx2), C.byref(dyv), C.byref(dxb), 0, 1, stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(fa.view(torch.int16), fb.view(torch.int16)) and float(tb.float().abs().sum()) > 0
    if yo or yx:
        assert float(ty2[..., :yo].abs().sum()) == 0 and float(ty2[..., yo + c:].abs().sum()) == 0
    for t in (ty2, tp2, tp3):
        assert float(t[:, 0].abs().sum()) == 0 and float(t[:, :, 0].abs().sum()) == 0
        assert float(t[:, -1].abs().sum()) == 0 and float(t[:, :, -1].abs().sum()) == 0
    # odd sizes: no fused path
    fo, to, ov = framed(torch.zeros(2, c, h + 1, w), 1, tdt)
    assert L.dbx_conv_pool_fusable(C.byref(d), C.byref(ov), C.byref(ov)) == 0


WG_CASES = [  # n, h, w, cin (view), cin real, cout, k, pad
    (2, 20, 28, 64, 64, 64, 3, 1), (2, 24, 24, 8, 3, 64, 3, 1), (3, 17, 23, 64, 64, 128, 3, 1), (2, 12, 12, 128, 128, 128, 3, 1),
    (1, 30, 30, 256, 256, 512, 3, 1), (2, 15, 15, 768, 768, 512, 1, 0), (2, 16, 16, 512, 512, 8, 1, 0),
    (3, 41, 77, 64, 64, 64, 3, 1), (2, 30, 126, 64, 64, 128, 3, 1), (5, 20, 62, 128, 100, 64, 3, 1),      # column-strip walk: ragged last strip
    # all-nine-taps LDS-DMA ring kernel (wgrad_all9_kernel): image seams of the compact walk, several splits and ci tiles
    (5, 30, 30, 512, 512, 512, 3, 1), (3, 60, 60, 128, 128, 256, 3, 1), (2, 120, 120, 64, 64, 128, 3, 1), (7, 30, 33, 192, 192, 128, 3, 1),
    # wide 1x1 LDS-DMA ring kernel (wgrad_wide2_kernel): compact walk with image seams, two ci tiles / one ci tile
    (5, 30, 30, 512, 512, 1024, 1, 0), (2, 60, 60, 256, 256, 512, 1, 0),
]


@pytest.mark.parametrize('dtn', ['bf16', 'f16'])
@pytest.mark.parametrize('case', WG_CASES)
def test_conv_wgrad_kernel(case, dtn):
    n, h, w, civ, ci, co, k, pad = case
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    g = torch.Generator(device='cpu').manual_seed(hash(case) % 1000)
    x = torch.zeros(n, civ, h, w)
    x[:, :ci] = torch.randn(n, ci, h, w, generator=g)
    cov = max(co, 8)
    dz = torch.zeros(n, cov, h, w)
    dz[:, :co] = torch.randn(n, co, h, w, generator=g)
    x, dz = x.cuda(), dz.cuda()
    xr = x.to(tdt).float().requires_grad_(False)
    dzr = dz.to(tdt).float()
    wref = torch.zeros(co, ci, k, k, device='cuda', requires_grad=True)
    bref = torch.zeros(co, device='cuda', requires_grad=True)
    out = F.conv2d(xr[:, :ci], wref, bref, padding=pad)
    out.backward(dzr[:, :co])
    fx, tx, xv = framed(x, 1, tdt)            # keep the tensors alive: the Views only carry raw pointers
    fz, tz, dzv = framed(dz, 1, tdt)
    dw = torch.empty(co, ci, k, k, device='cuda')
    db = torch.empty(co, device='cuda')
    sc = torch.empty(L.dbx_conv_wgrad_scratch_bytes(dt, C.byref(dzv), C.byref(xv), k, k), dtype=torch.uint8, device='cuda')
    check(L.dbx_conv_wgrad(dt, C.byref(dzv), C.byref(xv), k, k, pad, co, ci, ptr(dw), ptr(db), ptr(sc), 0, stream_ptr()))
    scale = wref.grad.abs().max().item()
    assert (dw - wref.grad).abs().max().item() <= 2e-4 * scale + 1e-4, ((dw - wref.grad).abs().max().item(), scale)
    assert torch.allclose(db, bref.grad, rtol=1e-4, atol=1e-3)
    # accumulate flag
    check(L.dbx_conv_wgrad(dt, C.byref(dzv), C.byref(xv), k, k, pad, co, ci, ptr(dw), ptr(db), ptr(sc), 1, stream_ptr()))
    assert (dw - 2 * wref.grad).abs().max().item() <= 4e-4 * scale + 2e-4


@pytest.mark.parametrize('dtn', ['bf16', 'f16'])
def test_conv_forward_split_destination(dtn):
    """dbx_conv_forward_split == two separate 1x1 GEMMs (second destination ReLU-gated), bit for bit."""
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    n, h, w, ci, c1, c2 = 2, 13, 17, 512, 512, 256
    g = torch.Generator(device='cpu').manual_seed(7)
    x = torch.randn(n, ci, h, w, generator=g).cuda()
    wt = (torch.randn(c1 + c2, ci, 1, 1, generator=g) * (1.0 / ci) ** 0.5).cuda()
    gate_src = torch.randn(n, c2, h, w, generator=g).cuda()
    fx, tx, xv = framed(x, 1, tdt)
    fg, tg, gv = framed(gate_src, 2, tdt)
    wp = pack(L, dt, wt, ci, c1 + c2)
    row_bytes = ci * _lib.ESIZE[dt]
    # reference: two launches
    fa, ta, av = framed(torch.zeros(n, c1, h, w), 0, tdt)
    fb, tb, bv = framed(torch.zeros(n, c2, h, w), 1, tdt)
    d1 = ConvDesc(dt, 1, 1, 0, ci, c1, 0)
    check(L.dbx_conv_forward(C.byref(d1), C.byref(xv), ptr(wp), None, C.byref(av), None, None, 0, stream_ptr()))
    d2 = ConvDesc(dt, 1, 1, 0, ci, c2, _lib.EPI_GATE)
    check(L.dbx_conv_forward(C.byref(d2), C.byref(xv), ptr(wp[c1 * row_bytes:]), None, C.byref(bv), C.byref(gv), None, 0, stream_ptr()))
    # split launch
    fa2, ta2, av2 = framed(torch.zeros(n, c1, h, w), 0, tdt)
    fb2, tb2, bv2 = framed(torch.zeros(n, c2, h, w), 1, tdt)
    d = ConvDesc(dt, 1, 1, 0, ci, c1 + c2, 0)
    check(L.dbx_conv_forward_split(C.byref(d), C.byref(xv), ptr(wp), None, C.byref(av2), None, C.byref(bv2), C.byref(gv), c1,
                                   _lib.EPI_GATE, stream_ptr()))
    assert torch.equal(ta, ta2) and torch.equal(tb, tb2)
    assert float(ta2.float().abs().sum()) > 0 and float(tb2.float().abs().sum()) > 0
    # and against torch on the rounded operands
    ref = F.conv2d(x.to(tdt).float(), wt.to(tdt).float())
    got1 = ta2.permute(0, 3, 1, 2).float()
    got2 = tb2[:, 1:1 + h, 1:1 + w].permute(0, 3, 1, 2).float()
    tol = 2e-2 if dtn == 'bf16' else 3e-3
    assert torch.allclose(got1, ref[:, :c1], rtol=tol, atol=tol)
    assert torch.allclose(got2, ref[:, c1:] * (gate_src.to(tdt).float() > 0), rtol=tol, atol=tol)
    # argument validation: the split must sit on a 256-channel tile boundary
    bad = View(C.c_void_p(ta2.data_ptr()), n, h, w, 0, c1, 0, 128)
    assert L.dbx_conv_forward_split(C.byref(d), C.byref(xv), ptr(wp), None, C.byref(bad), None, C.byref(bv2), C.byref(gv), 128,
                                    _lib.EPI_GATE, stream_ptr()) != 0


@pytest.mark.parametrize('dtn', ['bf16', 'f16', 'f32'])
@pytest.mark.parametrize('ks', [(1, 4), (1, 4, 4, 8), (2, 4, 4)])
def test_head2_wgrad_kernel(ks, dtn):
    """One streaming pass == per-head einsum of d_out x hid on the rounded operands (fp32 accumulation order differs)."""
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    nh, n, h, w, slot = len(ks), 3, 11, 19, 8
    g = torch.Generator(device='cpu').manual_seed(3 + nh)
    hid = torch.randn(n, 512 * nh, h, w, generator=g).cuda()
    dout = torch.zeros(n, slot * nh, h, w)
    for i, k in enumerate(ks):
        dout[:, slot * i:slot * i + k] = torch.randn(n, k, h, w, generator=g)
    dout = dout.cuda()
    fh, th, hv = framed(hid, 0, tdt)
    fd, td, dv = framed(dout, 1, tdt)
    dws = [torch.full((k, 512), -7.0, device='cuda') for k in ks]
    dbs = [torch.full((k,), -7.0, device='cuda') for k in ks]
    sc = torch.empty(L.dbx_head2_wgrad_scratch_bytes(nh, n * h), dtype=torch.uint8, device='cuda')
    check(L.dbx_head2_wgrad(dt, C.byref(dv), C.byref(hv), (C.c_int32 * nh)(*ks), nh, (C.c_void_p * nh)(*[t.data_ptr() for t in dws]),
                            (C.c_void_p * nh)(*[t.data_ptr() for t in dbs]), ptr(sc), stream_ptr()))
    hr, dr = hid.to(tdt).double(), dout.to(tdt).double()
    for i, k in enumerate(ks):
        ref_w = torch.einsum('nkhw,nchw->kc', dr[:, slot * i:slot * i + k], hr[:, 512 * i:512 * (i + 1)])
        ref_b = dr[:, slot * i:slot * i + k].sum(dim=(0, 2, 3))
        scale = ref_w.abs().max().item()
        assert (dws[i].double() - ref_w).abs().max().item() <= 2e-5 * scale + 1e-5
        assert (dbs[i].double() - ref_b).abs().max().item() <= 1e-4
    # repeatable bit for bit
    dw0 = [t.clone() for t in dws]
    check(L.dbx_head2_wgrad(dt, C.byref(dv), C.byref(hv), (C.c_int32 * nh)(*ks), nh, (C.c_void_p * nh)(*[t.data_ptr() for t in dws]),
                            (C.c_void_p * nh)(*[t.data_ptr() for t in dbs]), ptr(sc), stream_ptr()))
    assert all(torch.equal(a, b) for a, b in zip(dw0, dws))


# ---------------------------------------------------------------- register-streamed-weights 3x3 kernel (conv3x3_ws.hpp)
# (n, h, w, cin, cout): every case must be picked by dbx_conv_plan as DBX_K_WS -- wide layers with >= 192 tiles.
# 30x30 (one frame row = one 32-pixel fragment), odd sizes (tiles and fragments straddle rows and images), 128 couts
# (two wave rows, 512-pixel tiles), 7- and 8-fragment tiles in one launch, image seams inside tiles.
WS_CASES = [(32, 30, 30, 512, 512), (16, 60, 60, 256, 256), (40, 30, 30, 256, 512), (20, 61, 53, 128, 256), (10, 120, 97, 128, 128), (33, 45, 45, 192, 256)]


def _ws_desc(L, dt, xv, yv, cin, cout, epi):
    """The plan prefers the ws kernel where it measured faster than the band kernel (un-gated 512 -> 512 and 256 -> 256 layers,
    128-cout layers with >= 256 input channels); DBX_CONV_WFRAG forces it on any problem it can run, which is what these tests do."""
    d = ConvDesc(dt, 3, 3, 1, cin, cout, epi)
    plan = _lib.ConvPlan()
    check(L.dbx_conv_plan(C.byref(d), C.byref(xv), C.byref(yv), C.byref(plan)))
    wm = 1 if cout % 256 == 0 else 2
    nogate = not (epi & _lib.EPI_GATE)
    pref = (wm == 2 and cin >= 256) or (nogate and wm == 1 and ((cin >= 512 and cout >= 512) or (cin == 256 and cout == 256)))
    if plan.kernel == _lib.K_P8:         # round 5: the plan gives the wide 3x3 layers to the 8-phase kernel where that one qualifies; ws stays reachable
        assert not plan.w_frag           # through DBX_CONV_WFRAG (what these tests do) and keeps the 128-cout / small problems
    else:
        assert (plan.kernel == _lib.K_WS and plan.w_frag == 1) == pref, (plan.kernel, plan.name)
        if pref:
            assert plan.name.decode().startswith('conv3x3_ws_kernel<')
    return ConvDesc(dt, 3, 3, 1, cin, cout, epi | _lib.CONV_WFRAG)


@pytest.mark.parametrize('dtn', ['bf16', 'f16'])
@pytest.mark.parametrize('case', WS_CASES)
def test_conv_ws_forward(case, dtn):
    n, h, w, ci, co = case
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    g = torch.Generator(device='cpu').manual_seed(sum(case))
    x = torch.randn(n, ci, h, w, generator=g).cuda()
    wt = (torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (ci * 9)) ** 0.5).cuda()
    b = torch.randn(co, generator=g).cuda()
    ref = F.relu(F.conv2d(x.to(tdt).float(), wt.to(tdt).float(), b, padding=1))
    fx, tx, xv = framed(x, 1, tdt)
    fy, ty, yv = framed(torch.zeros(n, co, h, w), 1, tdt)
    d = _ws_desc(L, dt, xv, yv, ci, co, _lib.EPI_BIAS | _lib.EPI_RELU)
    check(L.dbx_conv_forward(C.byref(d), C.byref(xv), ptr(pack(L, dt, wt, ci, co, mode=4)), ptr(b), C.byref(yv), None, None, 0, stream_ptr()))
    got = ty[:, 1:1 + h, 1:1 + w].permute(0, 3, 1, 2).float()
    tol = (2e-2 if dtn == 'bf16' else 3e-3)
    assert torch.allclose(got, ref, rtol=tol, atol=tol), (got - ref).abs().max().item()
    assert float(ty[:, 0].abs().sum()) == 0 and float(ty[:, :, 0].abs().sum()) == 0
    assert float(ty[:, -1].abs().sum()) == 0 and float(ty[:, :, -1].abs().sum()) == 0
    # the band kernel on row-major weights computes the same sums in another order: equal up to output rounding
    fy2, ty2, yv2 = framed(torch.zeros(n, co, h, w), 1, tdt)
    d0 = ConvDesc(dt, 3, 3, 1, ci, co, _lib.EPI_BIAS | _lib.EPI_RELU)
    check(L.dbx_conv_forward(C.byref(d0), C.byref(xv), ptr(pack(L, dt, wt, ci, co)), ptr(b), C.byref(yv2), None, None, 0, stream_ptr()))
    assert (ty.float() - ty2.float()).abs().max().item() <= tol * (1.0 + ref.abs().max().item())


@pytest.mark.parametrize('dtn', ['bf16', 'f16'])
@pytest.mark.parametrize('case', [(56, 30, 30, 256, 512), (30, 60, 60, 128, 256)])
def test_conv_ws_dgrad_gate_and_sliced_views(case, dtn):
    """Data gradient through the ws kernel (pack mode 5, ReLU gate), written into a channel slice of a wider frame and read
    from a channel slice (the fusion concat's conv3_4 slot): dx = conv_transpose(dz, w) * (gate > 0)."""
    n, h, w, ci, co = case                      # forward layer ci -> co; the dgrad maps co -> ci channels
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    g = torch.Generator(device='cpu').manual_seed(sum(case) + 1)
    dz = torch.randn(n, co, h, w, generator=g).cuda()
    wt = (torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (co * 9)) ** 0.5).cuda()
    gate = torch.randn(n, ci, h, w, generator=g).cuda()
    ref = F.conv_transpose2d(dz.to(tdt).float(), wt.to(tdt).float(), padding=1) * (gate.to(tdt).float() > 0)
    # dz lives in channels [64, 64 + co) of a wider frame; dx goes to channels [128, 128 + ci) of a 128 + ci + 64 wide frame
    wide = torch.zeros(n, 64 + co + 64, h, w, device='cuda')
    wide[:, 64:64 + co] = dz
    fz, tz, zv_all = framed(wide, 1, tdt)
    zv = View(zv_all.ptr, n, h, w, 1, zv_all.ld, 64, co)
    fd, td, dv_all = framed(torch.zeros(n, 128 + ci + 64, h, w), 1, tdt)
    dv = View(dv_all.ptr, n, h, w, 1, dv_all.ld, 128, ci)
    fg, tg, gv = framed(gate, 1, tdt)
    d = _ws_desc(L, dt, zv, dv, co, ci, _lib.EPI_GATE)
    check(L.dbx_conv_forward(C.byref(d), C.byref(zv), ptr(pack(L, dt, wt, co, ci, mode=5)), None, C.byref(dv), C.byref(gv), None, 0,
                             stream_ptr()))
    got = td[:, 1:1 + h, 1:1 + w, 128:128 + ci].permute(0, 3, 1, 2).float()
    tol = (2e-2 if dtn == 'bf16' else 3e-3)
    assert torch.allclose(got, ref, rtol=tol, atol=tol), (got - ref).abs().max().item()
    assert float(td[..., :128].abs().sum()) == 0 and float(td[..., 128 + ci:].abs().sum()) == 0     # neighbours untouched
    assert float(td[:, 0].abs().sum()) == 0 and float(td[:, :, -1].abs().sum()) == 0                # frame untouched


def test_pack_fragment_order_matches_documented_index():
    """dbx_pack_weight modes 4/5 against the index formula of include/densebox_hip.h, built with numpy."""
    L = _lib.lib()
    dt = _lib.DTYPE_ID['f16']
    for co, ci, mode, ks in [(256, 128, 4, 3), (128, 192, 4, 3), (256, 128, 5, 3), (128, 256, 5, 3), (512, 256, 4, 1), (256, 512, 5, 1)]:
        g = torch.Generator(device='cpu').manual_seed(co + ci + mode)
        taps = ks * ks
        wt = torch.randn(co, ci, ks, ks, generator=g)
        rows, k = (co, ci) if mode == 4 else (ci, co)
        got = pack(L, dt, wt.cuda(), k, rows, mode=mode).view(torch.float16).cpu().numpy()
        w16 = wt.to(torch.float16).numpy().reshape(co, ci, taps)
        bn = 256 if rows % 256 == 0 else 128
        exp = np.zeros(rows * taps * k, dtype=np.float16)
        r_, t_, k_ = np.meshgrid(np.arange(rows), np.arange(taps), np.arange(k), indexing='ij')
        if ks == 3:
            kc = k // 64
            ky, kx = t_ // 3, t_ % 3
            blk = ((((r_ // bn) * (3 * kc) + 3 * (k_ // 64) + ky) * 12 + kx * 4 + (k_ % 64) // 16) * (bn // 32) + (r_ % bn) // 32)
        else:
            blk = ((((r_ // bn) * (k // 128) + k_ // 128) * 8 + (k_ % 128) // 16) * (bn // 32) + (r_ % bn) // 32)
        idx = (blk * 64 + 32 * ((k_ % 16) // 8) + r_ % 32) * 8 + k_ % 8
        src = w16[r_, k_, t_] if mode == 4 else w16[k_, r_, taps - 1 - t_]
        exp[idx.ravel()] = src.ravel()
        assert np.array_equal(got[:exp.size], exp), (co, ci, mode, ks)


# ---------------------------------------------------------------- 1x1 GEMMs on the ws kernel (the heads' 768 -> 512 nh conv and its data gradient)
@pytest.mark.parametrize('dtn', ['bf16', 'f16'])
def test_conv_ws_1x1_forward_bias_and_hash_dropout(dtn):
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    n, h, w, ci, co = 16, 60, 57, 768, 1024
    g = torch.Generator(device='cpu').manual_seed(3)
    x = torch.randn(n, ci, h, w, generator=g).cuda()
    wt = (torch.randn(co, ci, 1, 1, generator=g) * (1.0 / ci) ** 0.5).cuda()
    b = torch.randn(co, generator=g).cuda()
    ref = F.conv2d(x.to(tdt).float(), wt.to(tdt).float(), b)
    fx, tx, xv = framed(x, 1, tdt)                                   # framed input (the fusion tensor has a 1-pixel frame)
    tol = (2e-2 if dtn == 'bf16' else 3e-3)
    outs = {}
    for frag in (True, False):
        for epi in (_lib.EPI_BIAS, _lib.EPI_BIAS | _lib.EPI_DROPHASH):
            fy, ty, yv = framed(torch.zeros(n, co, h, w), 0, tdt)    # un-framed output (the hidden map)
            d = ConvDesc(dt, 1, 1, 0, ci, co, epi, 0x1234)
            plan = _lib.ConvPlan()
            check(L.dbx_conv_plan(C.byref(d), C.byref(xv), C.byref(yv), C.byref(plan)))
            if plan.kernel == _lib.K_P8:     # round 5: the plan gives the bias + hash-dropout GEMM to the 8-phase kernel (plain weights: the frag = False arm)
                assert epi & _lib.EPI_DROPHASH and plan.name.decode().endswith(',1,1>') and not plan.w_frag
            else:
                assert plan.kernel == _lib.K_WS and plan.name.decode().startswith('conv3x3_ws_kernel<') and ',1,1,' in plan.name.decode()
            if frag:
                d = ConvDesc(dt, 1, 1, 0, ci, co, epi | _lib.CONV_WFRAG, 0x1234)
            check(L.dbx_conv_forward(C.byref(d), C.byref(xv), ptr(pack(L, dt, wt, ci, co, mode=4 if frag else 0)), ptr(b), C.byref(yv),
                                     None, None, 0, stream_ptr()))
            outs[(frag, epi)] = ty.permute(0, 3, 1, 2).float()
    plain = outs[(True, _lib.EPI_BIAS)]
    assert torch.allclose(plain, ref, rtol=tol, atol=tol), (plain - ref).abs().max().item()
    # hash dropout: the same keep bits as the kernel that takes plain weights (the 8-phase kernel, or the LDS-ring kernel under DBX_P8=0): same
    # seed, pixel and channel counters, kept values doubled
    a, bb = outs[(True, _lib.EPI_BIAS | _lib.EPI_DROPHASH)], outs[(False, _lib.EPI_BIAS | _lib.EPI_DROPHASH)]
    assert torch.allclose(a, bb, rtol=tol, atol=tol)
    big = ref.abs() > 0.1
    assert torch.equal((a != 0)[big], (bb != 0)[big])
    keep = (a != 0)[big].float().mean().item()
    assert 0.45 < keep < 0.55, keep
    assert torch.allclose(a[big & (a != 0)], 2 * ref[big & (a != 0)], rtol=2 * tol, atol=2 * tol)


@pytest.mark.parametrize('dtn', ['bf16', 'f16'])
def test_conv_ws_1x1_split_destination(dtn):
    """The fusion concat's data gradient on the ws kernel == the LDS-ring kernel's dbx_conv_forward_split (row-major weights)."""
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    n, h, w, ci, c1, c2 = 16, 60, 60, 1024, 512, 256
    g = torch.Generator(device='cpu').manual_seed(11)
    x = torch.randn(n, ci, h, w, generator=g).cuda()
    wt = (torch.randn(c1 + c2, ci, 1, 1, generator=g) * (1.0 / ci) ** 0.5).cuda()
    gate_src = torch.randn(n, c2, h, w, generator=g).cuda()
    fx, tx, xv = framed(x, 1, tdt)
    fg, tg, gv = framed(gate_src, 1, tdt)
    res = []
    for frag in (False, True):
        fa, ta, av = framed(torch.zeros(n, c1, h, w), 0, tdt)
        fb, tb, bv = framed(torch.zeros(n, c2, h, w), 1, tdt)
        d = ConvDesc(dt, 1, 1, 0, ci, c1 + c2, _lib.CONV_WFRAG if frag else 0)
        check(L.dbx_conv_forward_split(C.byref(d), C.byref(xv), ptr(pack(L, dt, wt, ci, c1 + c2, mode=4 if frag else 0)), None, C.byref(av),
                                       None, C.byref(bv), C.byref(gv), c1, _lib.EPI_GATE, stream_ptr()))
        res.append((ta.float(), tb.float()))
    tol = (2e-2 if dtn == 'bf16' else 3e-3)
    ref = F.conv2d(x.to(tdt).float(), wt.to(tdt).float())
    assert torch.allclose(res[1][0].permute(0, 3, 1, 2), ref[:, :c1], rtol=tol, atol=tol)
    assert torch.allclose(res[1][1][:, 1:-1, 1:-1].permute(0, 3, 1, 2), ref[:, c1:] * (gate_src.to(tdt).float() > 0), rtol=tol, atol=tol)
    assert torch.allclose(res[0][0], res[1][0], rtol=tol, atol=tol) and torch.allclose(res[0][1], res[1][1], rtol=tol, atol=tol)
    assert float(res[1][1][:, 0].abs().sum()) == 0 and float(res[1][1][:, :, -1].abs().sum()) == 0     # frame of y2 untouched


def test_forced_kernel_variants_in_subprocesses():
    """The library picks kernels per process (environment read once): re-run the kernel tests with (a) the register-streamed-weights
    kernel disabled, so that the LDS band kernels it replaced on the wide layers (256x256 / 256x128 tiles) keep their direct oracle
    comparison, and (b) the row3 / all-taps weight-gradient kernels.  (The register-staged v1 conv kernel forced everywhere: the `v1`
    cases of test_conv_forward_kernel, each checked in the one child _v1_outcomes starts.)"""
    import subprocess
    import sys
    here = os.path.abspath(__file__)
    for env, sel in (({'DBX_WS': '0'}, 'test_conv_forward_kernel and dma'),
                     ({'DBX_WGRAD_VARIANT': '20'}, 'test_conv_wgrad_kernel')):      # the row3 / all-taps kernels behind wgrad_all9
        r = subprocess.run([sys.executable, '-m', 'pytest', here, '-x', '-q', '-m', 'gpu', '-k', sel], capture_output=True, text=True,
                           env=dict(os.environ, **env), timeout=1800)
        assert r.returncode == 0, (env, r.stdout[-3000:])
        assert ' passed' in r.stdout and 'skipped' not in r.stdout.splitlines()[-1], (env, r.stdout[-500:])


@pytest.mark.parametrize('dtn', ['bf16', 'f16', 'f32'])
@pytest.mark.parametrize('drop', ['none', 'hash', 'mask'])
def test_head2_backward_fused_equals_separate_calls(dtn, drop):
    """dbx_head2_backward (one pass: weight/bias gradients + data gradient) is bitwise dbx_head2_wgrad + dbx_head2_dgrad."""
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    ks = [1, 4, 4, 8]
    nh, n, h, w = len(ks), 3, 11, 13
    g = torch.Generator(device='cpu').manual_seed(5)
    hid = torch.relu(torch.randn(n, 512 * nh, h, w, generator=g)).cuda()
    dout = torch.zeros(n, 8 * nh, h, w)
    for i, k in enumerate(ks):
        dout[:, 8 * i:8 * i + k] = torch.randn(n, k, h, w, generator=g)
    dout = dout.cuda()
    w2 = [(torch.randn(k, 512, generator=g) * 0.05).cuda().contiguous() for k in ks]
    fh, th, hv = framed(hid, 1, tdt)
    fo, to, dv = framed(dout, 0, tdt)
    mask = (torch.rand(n * h * w, 512 * nh, generator=g) < 0.5).to(torch.uint8).cuda() if drop == 'mask' else None
    use_hash, seed = (1, 0xBEEF) if drop == 'hash' else (0, 0)
    sc = torch.empty(L.dbx_head2_wgrad_scratch_bytes(nh, n * h), dtype=torch.uint8, device='cuda')
    karr = (C.c_int32 * nh)(*ks)
    wp = (C.c_void_p * nh)(*[t.data_ptr() for t in w2])

    def outs():
        fd, td, dhv = framed(torch.zeros(n, 512 * nh, h, w), 1, tdt)
        dws = [torch.full((k, 512), 7.0, device='cuda') for k in ks]
        dbs = [torch.full((k,), 7.0, device='cuda') for k in ks]
        return fd, td, dhv, dws, dbs
    fd1, td1, dhv1, dw1, db1 = outs()
    check(L.dbx_head2_wgrad(dt, C.byref(dv), C.byref(hv), karr, nh, (C.c_void_p * nh)(*[t.data_ptr() for t in dw1]),
                            (C.c_void_p * nh)(*[t.data_ptr() for t in db1]), ptr(sc), stream_ptr()))
    check(L.dbx_head2_dgrad(dt, C.byref(dv), wp, karr, nh, C.byref(dhv1), ptr(mask), 512 * nh, use_hash, seed, stream_ptr()))
    fd2, td2, dhv2, dw2, db2 = outs()
    check(L.dbx_head2_backward(dt, C.byref(dv), C.byref(hv), wp, karr, nh, C.byref(dhv2), ptr(mask), 512 * nh, use_hash, seed,
                               (C.c_void_p * nh)(*[t.data_ptr() for t in dw2]), (C.c_void_p * nh)(*[t.data_ptr() for t in db2]),
                               ptr(sc), stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(fd1, fd2) and float(td2.float().abs().sum()) > 0
    assert all(torch.equal(a, b) for a, b in zip(dw1, dw2)) and all(torch.equal(a, b) for a, b in zip(db1, db2))


@pytest.mark.parametrize('dtn', ['bf16', 'f16', 'f32'])
@pytest.mark.parametrize('drop', ['hash', 'mask', 'none'])
@pytest.mark.parametrize('geom', [(3, 60, 60, 30, 30), (2, 23, 37, 12, 19), (2, 9, 24, 5, 12), (11, 7, 31, 4, 16), (2, 10, 64, 9, 32), (2, 10, 64, 9, 33), (1, 12, 70, 6, 35)])
def test_head2_backward_up_equals_backward_then_transposed_upsampling(geom, drop, dtn):
    """dbx_head2_backward_up == dbx_head2_backward followed by dbx_upsample_bilinear_bwd (no gate): d_hid and d_g44 bit for bit, the
    weight/bias gradients up to the order of the fp32 sums; repeatable bit for bit.  60x60 -> 30x30 and 23x37 -> 12x19 run as two
    half-row workgroups per slice, 9x24 -> 5x12 and 7x31 -> 4x16 as one; f32, the 64-wide maps (a half would be 33 columns) and the
    70-wide one take the two passes inside the entry point."""
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    n, h, w, hs, ws = geom
    ks = [1, 4, 4, 8] if n < 3 else [2, 4]
    nh = len(ks)
    g = torch.Generator(device='cpu').manual_seed(11 + h)
    hid = torch.randn(n, 512 * nh, h, w, generator=g).cuda()
    dout = torch.zeros(n, 8 * nh, h, w)
    for i, k in enumerate(ks):
        dout[:, 8 * i:8 * i + k] = torch.randn(n, k, h, w, generator=g)
    dout = dout.cuda()
    w2 = [(torch.randn(k, 512, generator=g) * 0.05).cuda().contiguous() for k in ks]
    fh, th, hv = framed(hid, 0, tdt)
    fo, to, dv = framed(dout, 0, tdt)
    mask = (torch.rand(n * h * w, 512 * nh, generator=g) < 0.5).to(torch.uint8).cuda() if drop == 'mask' else None
    use_hash, seed = (1, 0xC0DE) if drop == 'hash' else (0, 0)
    sc = torch.empty(L.dbx_head2_wgrad_scratch_bytes(nh, n * h), dtype=torch.uint8, device='cuda')
    karr = (C.c_int32 * nh)(*ks)
    wp = (C.c_void_p * nh)(*[t.data_ptr() for t in w2])

    def outs():
        fd, td, dhv = framed(torch.zeros(n, 512 * nh, h, w), 0, tdt)
        fg, tg, dgv = framed(torch.zeros(n, 512 * nh, hs, ws), 1, tdt)
        dws = [torch.full((k, 512), 7.0, device='cuda') for k in ks]
        dbs = [torch.full((k,), 7.0, device='cuda') for k in ks]
        return fd, td, dhv, fg, tg, dgv, dws, dbs

    def fused(o):
        fd, td, dhv, fg, tg, dgv, dws, dbs = o
        check(L.dbx_head2_backward_up(dt, C.byref(dv), C.byref(hv), wp, karr, nh, C.byref(dhv), ptr(mask), 512 * nh, use_hash, seed,
                                      (C.c_void_p * nh)(*[t.data_ptr() for t in dws]), (C.c_void_p * nh)(*[t.data_ptr() for t in dbs]),
                                      ptr(sc), C.byref(dgv), stream_ptr()))
        torch.cuda.synchronize()
    o1 = outs()
    fd1, td1, dhv1, fg1, tg1, dgv1, dw1, db1 = o1
    check(L.dbx_head2_backward(dt, C.byref(dv), C.byref(hv), wp, karr, nh, C.byref(dhv1), ptr(mask), 512 * nh, use_hash, seed,
                               (C.c_void_p * nh)(*[t.data_ptr() for t in dw1]), (C.c_void_p * nh)(*[t.data_ptr() for t in db1]),
                               ptr(sc), stream_ptr()))
    check(L.dbx_upsample_bilinear_bwd(dt, C.byref(dhv1), C.byref(dgv1), None, stream_ptr()))
    torch.cuda.synchronize()
    o2 = outs()
    fused(o2)
    fd2, td2, dhv2, fg2, tg2, dgv2, dw2, db2 = o2
    assert float(td2.float().abs().sum()) > 0 and float(tg2.float().abs().sum()) > 0
    assert torch.equal(fd1, fd2)
    assert torch.equal(fg1, fg2), (fg1.float() - fg2.float()).abs().max().item()
    for a, b in zip(dw1 + db1, dw2 + db2):
        assert (a - b).abs().max().item() <= 2e-5 * a.abs().max().item() + 1e-5
    o3 = outs()
    fused(o3)
    assert torch.equal(fg2, o3[3]) and all(torch.equal(a, b) for a, b in zip(dw2 + db2, o3[6] + o3[7]))


@pytest.mark.parametrize('dtn', ['bf16', 'f16'])
@pytest.mark.parametrize('shape', [(3, 40, 72), (2, 18, 34), (16, 64, 128)])
def test_conv_forward_pool_equals_conv_then_maxpool(shape, dtn):
    """dbx_conv_forward_pool (conv1_2 + pool1 in one kernel): the pooled map is bitwise dbx_maxpool2x2 of the full map it
    writes; where dbx_conv_forward runs the same halo-tile kernel (>= 256 tiles) the full map is bitwise equal too, elsewhere
    equal up to summation order; write_full = 0 leaves the full map untouched."""
    n, h, w = shape
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    g = torch.Generator(device='cpu').manual_seed(h * w)
    x = torch.randn(n, 64, h, w, generator=g).cuda()
    wt = (torch.randn(64, 64, 3, 3, generator=g) * (2.0 / 576) ** 0.5).cuda()
    b = torch.randn(64, generator=g).cuda()
    fx, tx, xv = framed(x, 1, tdt)
    wp = pack(L, dt, wt, 64, 64)
    d = ConvDesc(dt, 3, 3, 1, 64, 64, _lib.EPI_BIAS | _lib.EPI_RELU)
    fy, ty, yv = framed(torch.zeros(n, 64, h, w), 1, tdt)
    fp, tp, pv = framed(torch.zeros(n, 64, h // 2, w // 2), 1, tdt)
    assert L.dbx_conv_pool_fusable(C.byref(d), C.byref(xv), C.byref(yv)) == 1
    check(L.dbx_conv_forward(C.byref(d), C.byref(xv), ptr(wp), ptr(b), C.byref(yv), None, None, 0, stream_ptr()))
    check(L.dbx_maxpool2x2(dt, C.byref(yv), C.byref(pv), stream_ptr()))
    fy2, ty2, yv2 = framed(torch.zeros(n, 64, h, w), 1, tdt)
    fp2, tp2, pv2 = framed(torch.zeros(n, 64, h // 2, w // 2), 1, tdt)
    check(L.dbx_conv_forward_pool(C.byref(d), C.byref(xv), ptr(wp), ptr(b), C.byref(yv2), C.byref(pv2), 1, stream_ptr()))
    fp4, tp4, pv4 = framed(torch.zeros(n, 64, h // 2, w // 2), 1, tdt)
    check(L.dbx_maxpool2x2(dt, C.byref(yv2), C.byref(pv4), stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(fp4, fp2) and float(tp2.float().abs().sum()) > 0
    plan = _lib.ConvPlan()
    check(L.dbx_conv_plan(C.byref(d), C.byref(xv), C.byref(yv), C.byref(plan)))
    if plan.kernel == _lib.K_C64:
        assert torch.equal(fy, fy2) and torch.equal(fp, fp2)
    else:
        assert (ty.float() - ty2.float()).abs().max().item() <= (2e-2 if dtn == 'bf16' else 3e-3) * (1 + ty.float().abs().max().item())
    assert (n, h, w) != (16, 64, 128) or plan.kernel == _lib.K_C64
    ref = F.max_pool2d(F.relu(F.conv2d(x.to(tdt).float(), wt.to(tdt).float(), b, padding=1)), 2)
    got = tp2[:, 1:1 + h // 2, 1:1 + w // 2].permute(0, 3, 1, 2).float()
    tol = 2e-2 if dtn == 'bf16' else 3e-3
    assert torch.allclose(got, ref, rtol=tol, atol=tol)
    fy3, ty3, yv3 = framed(torch.zeros(n, 64, h, w), 1, tdt)
    fp3, tp3, pv3 = framed(torch.zeros(n, 64, h // 2, w // 2), 1, tdt)
    check(L.dbx_conv_forward_pool(C.byref(d), C.byref(xv), ptr(wp), ptr(b), C.byref(yv3), C.byref(pv3), 0, stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(fp2, fp3) and float(fy3.float().abs().sum()) == 0
    # ... with the arg-max nibbles (training): same pooled map, the full map not needed; the nibbles are bitwise the ones
    # dbx_maxpool2x2_idx takes from the full map, and the pooling backward driven by them equals the activation-reading backward
    nb = L.dbx_maxpool_idx_bytes(n, h, w, 64)
    idx = torch.zeros(nb + 16, dtype=torch.uint8, device='cuda')
    fy5, ty5, yv5 = framed(torch.zeros(n, 64, h, w), 1, tdt)
    fp5, tp5, pv5 = framed(torch.zeros(n, 64, h // 2, w // 2), 1, tdt)
    check(L.dbx_conv_forward_pool_idx(C.byref(d), C.byref(xv), ptr(wp), ptr(b), C.byref(yv5), C.byref(pv5), 0, ptr(idx), stream_ptr()))
    idx2 = torch.zeros(nb + 16, dtype=torch.uint8, device='cuda')
    fp6, tp6, pv6 = framed(torch.zeros(n, 64, h // 2, w // 2), 1, tdt)
    check(L.dbx_maxpool2x2_idx(dt, C.byref(yv2), C.byref(pv6), ptr(idx2), stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(fp2, fp5) and float(fy5.float().abs().sum()) == 0 and int(idx[-16:].sum()) == 0
    assert torch.equal(idx, idx2) and int((idx & 3).sum()) > 0 and int((idx & 4).sum()) > 0
    dy = torch.randn(n, 64, h // 2, w // 2, generator=g).cuda()
    fdy, tdy, dyv = framed(dy, 0, tdt)
    fa, ta, dxa = framed(torch.zeros(n, 64, h, w), 1, tdt)
    fb, tb, dxb = framed(torch.zeros(n, 64, h, w), 1, tdt)
    check(L.dbx_maxpool2x2_bwd(dt, C.byref(yv2), C.byref(dyv), C.byref(dxa), 0, 1, stream_ptr()))
    check(L.dbx_maxpool2x2_bwd_idx(dt, ptr(idx), C.byref(dyv), C.byref(dxb), 0, 1, stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(fa, fb) and float(tb.float().abs().sum()) > 0
    # both outputs at once (write_full = 1 + nibbles)
    idx3 = torch.zeros(nb + 16, dtype=torch.uint8, device='cuda')
    fy7, ty7, yv7 = framed(torch.zeros(n, 64, h, w), 1, tdt)
    fp7, tp7, pv7 = framed(torch.zeros(n, 64, h // 2, w // 2), 1, tdt)
    check(L.dbx_conv_forward_pool_idx(C.byref(d), C.byref(xv), ptr(wp), ptr(b), C.byref(yv7), C.byref(pv7), 1, ptr(idx3), stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(fy7, fy2) and torch.equal(fp7, fp2) and torch.equal(idx3, idx)
    # odd sizes: no fused path (the caller runs conv + maxpool)
    fo, to, ov = framed(torch.zeros(n, 64, h + 1, w), 1, tdt)
    assert L.dbx_conv_pool_fusable(C.byref(d), C.byref(ov), C.byref(ov)) == 0


@pytest.mark.parametrize('dtn', ['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('shape', [(2, 64, 12, 20), (1, 128, 15, 9), (3, 8, 6, 7), (2, 256, 60, 60)])
def test_maxpool_idx_backward_equals_activation_backward_and_aten(shape, dtn):
    """dbx_maxpool2x2_idx / dbx_maxpool2x2_bwd_idx (training: the backward reads arg-max nibbles instead of the un-pooled map) against
    dbx_maxpool2x2 / dbx_maxpool2x2_bwd (bitwise, with and without accumulation and ReLU gate) and against ATen's max_pool2d backward
    on the CPU (first maximum wins) -- on activations quantised to a few levels so that ties and all-zero windows are everywhere;
    odd heights / widths (floor mode: the ragged row / column gets no gradient)."""
    n, c, h, w = shape
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    g = torch.Generator(device='cpu').manual_seed(n * c + h)
    x = F.relu(torch.round(torch.randn(n, c, h, w, generator=g) * 2) / 2)
    dy = torch.round(torch.randn(n, c, h // 2, w // 2, generator=g) * 8) / 8
    fx, tx, xv = framed(x.cuda(), 1, tdt)
    fpa, tpa, pva = framed(torch.zeros(n, c, h // 2, w // 2), 1, tdt)
    fpb, tpb, pvb = framed(torch.zeros(n, c, h // 2, w // 2), 1, tdt)
    nb = L.dbx_maxpool_idx_bytes(n, h, w, c)
    assert nb == n * (h // 2) * (w // 2) * (c // 2)
    idx = torch.full((nb + 16,), 0xAB, dtype=torch.uint8, device='cuda')
    check(L.dbx_maxpool2x2(dt, C.byref(xv), C.byref(pva), stream_ptr()))
    check(L.dbx_maxpool2x2_idx(dt, C.byref(xv), C.byref(pvb), ptr(idx), stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(fpa, fpb) and bool((idx[nb:] == 0xAB).all())
    fdy, tdy, dyv = framed(dy.cuda(), 0, tdt)
    xc = x.clone().requires_grad_(True)
    pooled = F.max_pool2d(xc, 2)
    for acc in (0, 1):
        for gate in (0, 1):
            init = (torch.round(torch.randn(n, c, h, w, generator=g) * 4) / 4) if acc else torch.zeros(n, c, h, w)
            fa, ta, dxa = framed(init.cuda(), 1, tdt)
            fb, tb, dxb = framed(init.cuda(), 1, tdt)
            check(L.dbx_maxpool2x2_bwd(dt, C.byref(xv), C.byref(dyv), C.byref(dxa), acc, gate, stream_ptr()))
            check(L.dbx_maxpool2x2_bwd_idx(dt, ptr(idx), C.byref(dyv), C.byref(dxb), acc, gate, stream_ptr()))
            torch.cuda.synchronize()
            assert torch.equal(fa, fb), (acc, gate)
            gref, = torch.autograd.grad(pooled, xc, dy * (pooled > 0).float() if gate else dy, retain_graph=True)
            got = tb[:, 1:1 + h, 1:1 + w].permute(0, 3, 1, 2).float().cpu()
            assert torch.equal(got, gref + init), (acc, gate)       # every value is exactly representable in the 16-bit types


@pytest.mark.parametrize('dtn', ['bf16', 'f16'])
@pytest.mark.parametrize('shape', [(2, 24, 40), (3, 37, 61), (20, 64, 96)])
def test_conv_dgrad_wgrad1_equals_dgrad_then_wgrad(shape, dtn):
    """dbx_conv_dgrad_wgrad1 (conv1_2's data gradient with conv1_1's weight gradient folded into the epilogue) against the two
    separate calls it replaces and against torch: dW1, db1 agree up to fp32 summation order."""
    n, h, w = shape
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    g = torch.Generator(device='cpu').manual_seed(h + w)
    dz = torch.randn(n, 64, h, w, generator=g).cuda()
    w2 = (torch.randn(64, 64, 3, 3, generator=g) * (2.0 / 576) ** 0.5).cuda()           # conv1_2 weights [co2][ci2 = co1]
    a11 = torch.randn(n, 64, h, w, generator=g).cuda()                                  # conv1_1 output (ReLU gate)
    x0 = torch.zeros(n, 8, h, w)
    x0[:, :3] = torch.randn(n, 3, h, w, generator=g)
    x0 = x0.cuda()
    fz, tz, zv = framed(dz, 1, tdt)
    fg, tg, gv = framed(a11, 1, tdt)
    fx, tx, xv = framed(x0, 1, tdt)
    wp = pack(L, dt, w2, 64, 64, mode=1)
    d = ConvDesc(dt, 3, 3, 1, 64, 64, _lib.EPI_GATE)
    assert L.dbx_conv_dgrad_wgrad1_fusable(C.byref(d), C.byref(zv), C.byref(gv), C.byref(xv)) == 1
    # the two calls
    fd, td, dv = framed(torch.zeros(n, 64, h, w), 1, tdt)
    check(L.dbx_conv_forward(C.byref(d), C.byref(zv), ptr(wp), None, C.byref(dv), C.byref(gv), None, 0, stream_ptr()))
    dw_a = torch.empty(64, 3, 3, 3, device='cuda'); db_a = torch.empty(64, device='cuda')
    sc = torch.empty(L.dbx_conv_wgrad_scratch_bytes(dt, C.byref(dv), C.byref(xv), 3, 3), dtype=torch.uint8, device='cuda')
    check(L.dbx_conv_wgrad(dt, C.byref(dv), C.byref(xv), 3, 3, 1, 64, 3, ptr(dw_a), ptr(db_a), ptr(sc), 0, stream_ptr()))
    # fused
    dw_b = torch.full((64, 3, 3, 3), 5.0, device='cuda'); db_b = torch.full((64,), 5.0, device='cuda')
    sc2 = torch.empty(L.dbx_conv_dgrad_wgrad1_scratch_bytes(), dtype=torch.uint8, device='cuda')
    check(L.dbx_conv_dgrad_wgrad1(C.byref(d), C.byref(zv), ptr(wp), C.byref(gv), C.byref(xv), 3, ptr(dw_b), ptr(db_b), ptr(sc2), 0, stream_ptr()))
    torch.cuda.synchronize()
    # (the two-call path computes d on whichever conv kernel the plan picks for this size, in its own summation order: single
    # elements of d may round to the neighbouring 16-bit value, so the sums agree to a few 16-bit ulps of one term, not to fp32)
    scale = dw_a.abs().max().item()
    rel = 1e-3 if dtn == 'bf16' else 2e-4
    assert (dw_a - dw_b).abs().max().item() <= rel * scale + 1e-4, ((dw_a - dw_b).abs().max().item(), scale)
    assert (db_a - db_b).abs().max().item() <= rel * db_a.abs().max().item() + 2e-3, (db_a - db_b).abs().max().item()
    # torch: d = conv_transpose(dz, w2) * (a11 > 0), rounded to the 16-bit type like the stored map
    dref = (F.conv_transpose2d(dz.to(tdt).float(), w2.to(tdt).float(), padding=1) * (a11.to(tdt).float() > 0)).to(tdt).float()
    w1 = torch.zeros(64, 3, 3, 3, device='cuda', requires_grad=True); b1 = torch.zeros(64, device='cuda', requires_grad=True)
    F.conv2d(x0[:, :3].to(tdt).float(), w1, b1, padding=1).backward(dref)
    tol = 2e-2 if dtn == 'bf16' else 3e-3
    assert (dw_b - w1.grad).abs().max().item() <= tol * scale
    # accumulate, and repeatability bit for bit
    dw_c = dw_b.clone(); db_c = db_b.clone()
    check(L.dbx_conv_dgrad_wgrad1(C.byref(d), C.byref(zv), ptr(wp), C.byref(gv), C.byref(xv), 3, ptr(dw_c), ptr(db_c), ptr(sc2), 1, stream_ptr()))
    dw_d = torch.empty_like(dw_b); db_d = torch.empty_like(db_b)
    check(L.dbx_conv_dgrad_wgrad1(C.byref(d), C.byref(zv), ptr(wp), C.byref(gv), C.byref(xv), 3, ptr(dw_d), ptr(db_d), ptr(sc2), 0, stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(dw_d, dw_b) and torch.equal(db_d, db_b)
    assert (dw_c - 2 * dw_b).abs().max().item() <= 1e-5 * scale + 1e-6


@pytest.mark.parametrize('dtn', ['bf16', 'f16', 'f32'])
@pytest.mark.parametrize('shape', [(3, 64, 15, 15, 30, 30), (2, 40, 12, 16, 25, 33), (2, 512, 30, 30, 60, 60), (1, 8, 7, 9, 7, 9),
                                   (1, 2048, 30, 30, 60, 60), (2, 1024, 15, 17, 29, 33)])      # column-walk kernel: wide maps, odd row count
def test_upsample_bilinear_forward_backward(shape, dtn):
    """dbx_upsample_bilinear(_bwd) == F.interpolate(mode='bilinear', align_corners=True) and its autograd transpose (with the
    optional ReLU gate), on the 2x case, the odd-size case of a 100x132 input and the identity."""
    n, c, hi, wi, ho, wo = shape
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    g = torch.Generator(device='cpu').manual_seed(sum(shape))
    x = torch.randn(n, c, hi, wi, generator=g).cuda()
    fx, tx, xv = framed(x, 1, tdt)
    fy, ty, yv = framed(torch.zeros(n, c, ho, wo), 1, tdt)
    check(L.dbx_upsample_bilinear(dt, C.byref(xv), C.byref(yv), stream_ptr()))
    xr = x.to(tdt).float().requires_grad_(True)
    ref = F.interpolate(xr, size=(ho, wo), mode='bilinear', align_corners=True)
    got = ty[:, 1:1 + ho, 1:1 + wo].permute(0, 3, 1, 2).float()
    tol = {'bf16': 1e-2, 'f16': 2e-3, 'f32': 1e-5}[dtn]
    assert torch.allclose(got, ref.detach(), rtol=tol, atol=tol), (got - ref).abs().max().item()
    assert float(ty[:, 0].float().abs().sum()) == 0 and float(ty[:, :, 0].float().abs().sum()) == 0
    dy = torch.randn(n, c, ho, wo, generator=g).cuda()
    gate = torch.randn(n, c, hi, wi, generator=g).cuda()
    fdy, tdy, dyv = framed(dy, 1, tdt)
    fg, tg, gv = framed(gate, 1, tdt)
    for use_gate in (False, True):
        fdx, tdx, dxv = framed(torch.zeros(n, c, hi, wi), 1, tdt)
        check(L.dbx_upsample_bilinear_bwd(dt, C.byref(dyv), C.byref(dxv), C.byref(gv) if use_gate else None, stream_ptr()))
        (gref,) = torch.autograd.grad(ref, xr, dy.to(tdt).float(), retain_graph=True)
        if use_gate:
            gref = gref * (gate.to(tdt).float() > 0)
        gotd = tdx[:, 1:1 + hi, 1:1 + wi].permute(0, 3, 1, 2).float()
        assert torch.allclose(gotd, gref, rtol=tol, atol=tol * (1 + gref.abs().max().item())), (gotd - gref).abs().max().item()


@pytest.mark.parametrize('dtn', ['bf16', 'f16'])
def test_pack_multi_equals_pack_weight_all_layouts(dtn):
    """dbx_pack_multi (one launch for a table of jobs; LDS-tile path for 16-bit weights, element-wise path otherwise) writes exactly
    what dbx_pack_weight writes, for the plain and fragment-order images of both orientations, side-by-side placement and the
    negative offsets that cut a channel range out of a wider tensor."""
    L = _lib.lib()
    dt = _lib.DTYPE_ID[dtn]
    es = 2
    g = torch.Generator(device='cpu').manual_seed(3)
    # (co, ci, k, mode, rows_pad, cin_pad, row_off, k_off)
    cases = [(256, 128, 3, 0, 256, 128, 0, 0), (256, 128, 3, 1, 128, 256, 0, 0), (256, 128, 3, 4, 256, 128, 0, 0), (256, 128, 3, 5, 128, 256, 0, 0),
             (512, 768, 1, 4, 1024, 768, 512, 0), (512, 768, 1, 5, 512, 1024, 0, 512), (512, 768, 1, 1, 256, 1024, -512, 512),
             (512, 768, 1, 5, 256, 1024, -512, 0), (64, 64, 5, 0, 64, 64, 0, 0), (64, 3, 3, 0, 64, 8, 0, 0), (4, 512, 1, 0, 64, 2048, 1, 512),
             (1, 64, 1, 1, 64, 8, 0, 0)]
    jobs, refs, outs, keep = [], [], [], []
    for co, ci, k, mode, rows_pad, cin_pad, row_off, k_off in cases:
        w = torch.randn(co, ci, k, k, generator=g).cuda()
        d = ConvDesc(dt, k, k, 0, cin_pad, rows_pad, 0)
        elems = L.dbx_conv_packed_elems(C.byref(d))
        ref = torch.zeros(elems * es, dtype=torch.uint8, device='cuda')
        out = torch.zeros_like(ref)
        check(L.dbx_pack_weight(dt, mode, ptr(w), co, ci, k, k, ptr(ref), rows_pad, cin_pad, row_off, k_off, stream_ptr()))
        ktot = (k * k * cin_pad * es + 127) // 128 * 128 // es
        jobs.append((w.data_ptr(), out.data_ptr(), co, ci, k * k, mode, rows_pad if mode >= 4 else ktot, cin_pad, row_off, k_off, rows_pad))
        refs.append(ref); outs.append(out); keep.append(w)
    rec = np.zeros(len(jobs), dtype=[('src', '<u8'), ('dst', '<u8'), ('co', '<i4'), ('ci', '<i4'), ('taps', '<i4'), ('mode', '<i4'),
                                     ('ktot', '<i8'), ('cin_pad', '<i4'), ('row_off', '<i4'), ('k_off', '<i4'), ('rows_lim', '<i4')])
    for i, j in enumerate(jobs):
        rec[i] = j
    tab = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    check(L.dbx_pack_multi(dt, ptr(tab), len(jobs), max(j[2] * j[3] * j[4] for j in jobs), stream_ptr()))
    torch.cuda.synchronize()
    for case, ref, out in zip(cases, refs, outs):
        assert torch.equal(ref, out), case
        assert int(ref.view(torch.int16).ne(0).sum()) > 0, case


@pytest.mark.parametrize('dtn', ['bf16', 'f16'])
def test_conv_wgrad_slice_writes_a_column_range(dtn):
    """dbx_conv_wgrad_slice: the gradient of one tensor of a channel concat lands in its column range of the wider OIHW gradient,
    bit-identical to dbx_conv_wgrad of that tensor alone, and leaves the other columns alone."""
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    n, h, w, ci, co, ctot, coff = 3, 30, 30, 256, 512, 768, 512
    g = torch.Generator(device='cpu').manual_seed(11)
    x = torch.randn(n, ci, h, w, generator=g).cuda()
    dz = torch.randn(n, co, h, w, generator=g).cuda()
    fx, tx, xv = framed(x, 1, tdt)
    fz, tz, dzv = framed(dz, 1, tdt)
    sc = torch.empty(L.dbx_conv_wgrad_scratch_bytes(dt, C.byref(dzv), C.byref(xv), 1, 1), dtype=torch.uint8, device='cuda')
    dw = torch.empty(co, ci, 1, 1, device='cuda'); db = torch.empty(co, device='cuda')
    check(L.dbx_conv_wgrad(dt, C.byref(dzv), C.byref(xv), 1, 1, 0, co, ci, ptr(dw), ptr(db), ptr(sc), 0, stream_ptr()))
    wide = torch.full((co, ctot, 1, 1), 7.0, device='cuda'); db2 = torch.empty(co, device='cuda')
    check(L.dbx_conv_wgrad_slice(dt, C.byref(dzv), C.byref(xv), 1, 1, 0, co, ci, ptr(wide), ctot, coff, ptr(db2), ptr(sc), 0, stream_ptr()))
    assert torch.equal(wide[:, coff:coff + ci], dw) and torch.equal(db, db2)
    assert float((wide[:, :coff] - 7.0).abs().max()) == 0.0
    assert L.dbx_conv_wgrad_slice(dt, C.byref(dzv), C.byref(xv), 1, 1, 0, co, ci, ptr(wide), ctot, coff + 1, ptr(db2), ptr(sc), 0, stream_ptr()) != 0


def test_fold_refine_equals_the_three_convs_and_the_upsampling():
    """dbx_fold_refine (eval-mode refine branch, DenseBox.py:464-471): conv6_1 (3x3) -> conv6_2 (5x5) -> bilinear up -> conv6_3 (1x1) as ONE
    un-padded 7x7 conv followed by the up-sampling of its single map (dbx_upsample_bilinear_nchw_f32), against the torch chain in fp64."""
    L = _lib.lib()
    g = torch.Generator(device='cpu').manual_seed(77)
    ci, cm = 5, 64
    w1 = torch.randn(cm, ci, 3, 3, generator=g) * 0.2; b1 = torch.randn(cm, generator=g) * 0.1
    w2 = torch.randn(cm, cm, 5, 5, generator=g) * 0.05; b2 = torch.randn(cm, generator=g) * 0.1
    w3 = torch.randn(1, cm, 1, 1, generator=g) * 0.3; b3 = torch.randn(1, generator=g)
    x = torch.randn(2, ci, 20, 26, generator=g)
    d = lambda t: t.double()
    ref = F.conv2d(F.interpolate(F.conv2d(F.conv2d(d(x), d(w1), d(b1)), d(w2), d(b2)), size=(40, 52), mode='bilinear', align_corners=True), d(w3), d(b3))
    dev = [t.cuda() for t in (w1, b1, w2, b2, w3, b3)]
    wf = torch.full((1, ci, 7, 7), float('nan'), device='cuda'); bf = torch.full((1,), float('nan'), device='cuda')
    vf = torch.full((cm, 5, 5), float('nan'), device='cuda')
    check(L.dbx_fold_refine(*[ptr(t) for t in dev], ci, cm, ptr(wf), ptr(bf), ptr(vf), stream_ptr()))
    torch.cuda.synchronize()
    assert torch.allclose(vf.double().cpu(), torch.einsum('n,nmab->mab', d(w3)[0, :, 0, 0], d(w2)), rtol=0, atol=1e-5)
    small = F.conv2d(x.cuda(), wf, bf)                                          # [2, 1, 14, 20]
    out = torch.empty((2, 1, 40, 52), device='cuda')
    check(L.dbx_upsample_bilinear_nchw_f32(ptr(small.contiguous()), 2, 14, 20, ptr(out), 40, 52, stream_ptr()))
    torch.cuda.synchronize()
    assert torch.allclose(out.double().cpu(), ref, rtol=0, atol=2e-4 * float(ref.abs().max())), float((out.double().cpu() - ref).abs().max())
    want = F.interpolate(small, size=(40, 52), mode='bilinear', align_corners=True)
    assert torch.allclose(out, want, rtol=0, atol=1e-5 * float(want.abs().max()))
    # the whole branch from the heads' fp32 NCHW outputs: cat -> pool4 -> folded conv (one kernel) -> up-sampling, odd map sizes included
    for hh, ww in ((40, 52), (33, 47), (14, 15)):
        lmk = torch.randn(2, 4, hh, ww, generator=g); sc = torch.randn(2, 1, hh, ww, generator=g)
        xin = F.max_pool2d(torch.cat((lmk, sc), dim=1), 2, 2)
        ref2 = F.conv2d(F.interpolate(F.conv2d(F.conv2d(d(xin), d(w1), d(b1)), d(w2), d(b2)), size=(hh, ww), mode='bilinear', align_corners=True), d(w3), d(b3))
        sm = torch.full((2, 1, hh // 2 - 6, ww // 2 - 6), float('nan'), device='cuda')
        lmk_d, sc_d = lmk.cuda(), sc.cuda()                                      # (kept alive: the call takes raw pointers)
        check(L.dbx_refine_eval(ptr(lmk_d), ptr(sc_d), 2, hh, ww, ptr(wf), ptr(bf), ptr(sm), stream_ptr()))
        out2 = torch.empty((2, 1, hh, ww), device='cuda')
        check(L.dbx_upsample_bilinear_nchw_f32(ptr(sm), 2, hh // 2 - 6, ww // 2 - 6, ptr(out2), hh, ww, stream_ptr()))
        torch.cuda.synchronize()
        assert torch.allclose(out2.double().cpu(), ref2, rtol=0, atol=2e-4 * float(ref2.abs().max())), (hh, ww, float((out2.double().cpu() - ref2).abs().max()))


@pytest.mark.parametrize('shape', [(3, 60, 60), (2, 40, 47), (1, 15, 14)])
def test_refine_backward_equals_autograd_through_the_three_convs(shape):
    """dbx_refine_backward (training: the refine branch's backward by its linear structure, csrc/refine_ops.hip) against torch autograd in
    fp64 through cat -> MaxPool2d -> conv6_1 -> conv6_2 -> Upsample(align_corners) -> conv6_3: every parameter gradient and the gradients
    of the landmark / score head outputs (incoming gradients added), odd map sizes included; two runs are bitwise equal."""
    n, h, w = shape
    L = _lib.lib()
    g = torch.Generator(device='cpu').manual_seed(n * 1000 + h)
    ci, cm = 5, 64
    P = [torch.randn(cm, ci, 3, 3, generator=g) * 0.2, torch.randn(cm, generator=g) * 0.1, torch.randn(cm, cm, 5, 5, generator=g) * 0.05,
         torch.randn(cm, generator=g) * 0.1, torch.randn(1, cm, 1, 1, generator=g) * 0.3, torch.randn(1, generator=g)]
    lmk = torch.randn(n, 4, h, w, generator=g); sc = torch.randn(n, 1, h, w, generator=g)
    d_ref = torch.randn(n, 1, h, w, generator=g); g_lm = torch.randn(n, 4, h, w, generator=g); g_sc = torch.randn(n, 1, h, w, generator=g)
    Pd = [p.double().requires_grad_(True) for p in P]
    lmd, scd = lmk.double().requires_grad_(True), sc.double().requires_grad_(True)
    x5 = F.max_pool2d(torch.cat((lmd, scd), dim=1), 2, 2)
    out = F.conv2d(F.interpolate(F.conv2d(F.conv2d(x5, Pd[0], Pd[1]), Pd[2], Pd[3]), size=(h, w), mode='bilinear', align_corners=True), Pd[4], Pd[5])
    ((out * d_ref.double()).sum() + (lmd * g_lm.double()).sum() + (scd * g_sc.double()).sum()).backward()
    dev = [p.cuda() for p in P]
    wf = torch.empty((1, ci, 7, 7), device='cuda'); bf = torch.empty((1,), device='cuda'); vf = torch.empty((cm, 5, 5), device='cuda')
    check(L.dbx_fold_refine(*[ptr(t) for t in dev], ci, cm, ptr(wf), ptr(bf), ptr(vf), stream_ptr()))
    ins = [t.cuda() for t in (d_ref, lmk, sc, g_lm, g_sc)]
    scratch = torch.empty(L.dbx_refine_backward_scratch_bytes(n, h, w), dtype=torch.uint8, device='cuda')

    def run():
        outs = [torch.full((n, 4, h, w), float('nan'), device='cuda'), torch.full((n, 1, h, w), float('nan'), device='cuda')]
        grads = [torch.full(p.shape, float('nan'), device='cuda') for p in P]
        check(L.dbx_refine_backward(ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), n, h, w, *[ptr(t) for t in dev], cm, ptr(wf), ptr(vf), ptr(ins[3]), ptr(ins[4]),
                                    ptr(outs[0]), ptr(outs[1]), *[ptr(t) for t in grads], ptr(scratch), stream_ptr()))
        torch.cuda.synchronize()
        return outs, grads
    (o_lm, o_sc), grads = run()
    (o_lm2, o_sc2), grads2 = run()
    assert torch.equal(o_lm, o_lm2) and torch.equal(o_sc, o_sc2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    for name, got, want in [('d landmark', o_lm, lmd.grad), ('d score', o_sc, scd.grad)] + [('dP%d' % i, grads[i], Pd[i].grad) for i in range(6)]:
        err = float((got.double().cpu() - want).abs().max()); scale = float(want.abs().max())
        assert err <= 1e-4 * scale, (name, err, scale)
    # no incoming gradients: null pointers mean zero
    o3 = [torch.empty((n, 4, h, w), device='cuda'), torch.empty((n, 1, h, w), device='cuda')]
    g3 = [torch.empty(p.shape, device='cuda') for p in P]
    check(L.dbx_refine_backward(ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), n, h, w, *[ptr(t) for t in dev], cm, ptr(wf), ptr(vf), None, None,
                                ptr(o3[0]), ptr(o3[1]), *[ptr(t) for t in g3], ptr(scratch), stream_ptr()))
    torch.cuda.synchronize()
    assert torch.allclose(o3[0].double().cpu(), lmd.grad - g_lm.double(), rtol=0, atol=1e-4 * float(lmd.grad.abs().max()))


@pytest.mark.parametrize('dtn', ['f32', 'bf16', 'f16'])
def test_nchw_to_framed_slots_equals_one_call_per_slot(dtn):
    """dbx_nchw_to_framed_slots (all heads' dL/dout in one launch) == dbx_nchw_to_framed into each slot view, bit for bit; a null source is zeros."""
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    n, h, w = 3, 11, 14
    slot = 8 if dtn != 'f32' else 32
    ks = [1, 4, 4, 8]
    g = torch.Generator(device='cpu').manual_seed(5)
    xs = [torch.randn(n, k, h, w, generator=g).cuda() for k in ks]
    fa, ta, va = framed(torch.full((n, 4 * slot, h, w), 7.0), 0, tdt)
    fb, tb, vb = framed(torch.full((n, 4 * slot, h, w), 7.0), 0, tdt)
    for i, (x, k) in enumerate(zip(xs, ks)):
        sv = View(va.ptr, n, h, w, 0, 4 * slot, slot * i, slot)
        check(L.dbx_nchw_to_framed(dt, ptr(x), k, C.byref(sv), stream_ptr()))
    check(L.dbx_nchw_to_framed_slots(dt, (C.c_void_p * 4)(*[x.data_ptr() for x in xs]), (C.c_int32 * 4)(*ks), 4, slot, C.byref(vb), stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(fa, fb) and float(tb.float().abs().sum()) > 0
    check(L.dbx_nchw_to_framed_slots(dt, (C.c_void_p * 4)(xs[0].data_ptr(), None, xs[2].data_ptr(), None), (C.c_int32 * 4)(*ks), 4, slot, C.byref(vb), stream_ptr()))
    torch.cuda.synchronize()
    assert float(tb[..., slot:2 * slot].float().abs().sum()) == 0 and float(tb[..., 3 * slot:].float().abs().sum()) == 0
    assert torch.equal(tb[..., :slot], ta[..., :slot]) and torch.equal(tb[..., 2 * slot:3 * slot], ta[..., 2 * slot:3 * slot])


@pytest.mark.parametrize('dtn', ['f16', 'bf16'])
@pytest.mark.parametrize('ks,n,h,w', [([1, 4, 4, 8], 3, 60, 60), ([1, 4], 5, 60, 60), ([1, 4, 4, 8], 2, 57, 83)])
def test_heads_forward_fused_equals_the_two_gemms(ks, n, h, w, dtn):
    """dbx_heads_forward_fused (both 1x1 convs of every head in one pass, DenseBox.py:158-162) against the two-call path: the hidden map
    is bitwise the one dbx_conv_forward writes (same kernel body, same dropout bits), the head outputs equal the second GEMM's to fp32
    summation order, and both equal torch fp32 on the rounded operands."""
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    nh, ktot = len(ks), sum(ks)
    g = torch.Generator(device='cpu').manual_seed(77)
    x = torch.relu(torch.randn(n, 768, h, w, generator=g)).cuda()
    w1 = (torch.randn(512 * nh, 768, 1, 1, generator=g) * 0.05).cuda()
    b1 = torch.randn(512 * nh, generator=g).cuda()
    w2 = [(torch.randn(k, 512, 1, 1, generator=g) * 0.05).cuda().contiguous() for k in ks]
    b2 = torch.zeros(64, device='cuda'); b2[:ktot] = torch.randn(ktot, generator=g).cuda()
    fx, tx, xv = framed(x, 1, tdt)
    seed = 0x1234ABCD
    d = ConvDesc(dt, 1, 1, 0, 768, 512 * nh, _lib.EPI_BIAS | _lib.EPI_DROPHASH | _lib.CONV_WFRAG, seed)
    karr = (C.c_int32 * nh)(*ks)
    fa, ta, hva = framed(torch.zeros(n, 512 * nh, h, w), 0, tdt)
    if not L.dbx_heads_forward_fusable(C.byref(d), C.byref(xv), C.byref(hva), karr, nh):
        pytest.skip('the 1x1 ws kernel does not take this problem')
    w1f = pack(L, dt, w1, 768, 512 * nh, mode=4)
    # second weights: fragment image (256 rows, head i at rows 0.., columns 512 i..) and the block-diagonal [64][512 nh] matrix
    d2f = ConvDesc(dt, 1, 1, 0, 512 * nh, 256, 0)
    w2f = torch.zeros(L.dbx_conv_packed_elems(C.byref(d2f)) * 2, dtype=torch.uint8, device='cuda')
    d2 = ConvDesc(dt, 1, 1, 0, 512 * nh, 64, 0)
    w2b = torch.zeros(L.dbx_conv_packed_elems(C.byref(d2)) * 2, dtype=torch.uint8, device='cuda')
    r = 0
    for i, (wt, k) in enumerate(zip(w2, ks)):
        check(L.dbx_pack_weight(dt, 4, ptr(wt), k, 512, 1, 1, ptr(w2f), 256, 512 * nh, 0, 512 * i, stream_ptr()))
        check(L.dbx_pack_weight(dt, 0, ptr(wt), k, 512, 1, 1, ptr(w2b), 64, 512 * nh, r, 512 * i, stream_ptr()))
        r += k
    out_a = torch.full((n, ktot, h, w), 7.0, device='cuda')
    sc = torch.empty(L.dbx_heads_forward_fused_scratch_bytes(nh, n * h * w), dtype=torch.uint8, device='cuda')
    check(L.dbx_heads_forward_fused(C.byref(d), C.byref(xv), ptr(w1f), ptr(b1), C.byref(hva), ptr(w2f), ptr(b2), karr, nh, ptr(out_a), ptr(sc),
                                    stream_ptr()))
    fb, tb, hvb = framed(torch.zeros(n, 512 * nh, h, w), 0, tdt)
    check(L.dbx_conv_forward(C.byref(d), C.byref(xv), ptr(w1f), ptr(b1), C.byref(hvb), None, None, 0, stream_ptr()))
    out_b = torch.full((n, ktot, h, w), 7.0, device='cuda')
    yv = View(C.c_void_p(out_b.data_ptr()), n, h, w, 0, ktot, 0, ktot)
    dd = ConvDesc(dt, 1, 1, 0, 512 * nh, 64, _lib.EPI_BIAS | _lib.EPI_F32_NCHW)
    check(L.dbx_conv_forward(C.byref(dd), C.byref(hvb), ptr(w2b), ptr(b2), C.byref(yv), None, None, 0, stream_ptr()))
    # one destination per head (dbx_heads_forward_fused_heads): bitwise the channel slices of the [N][sum k][H][W] form
    outs_h = [torch.full((n, k, h, w), 7.0, device='cuda') for k in ks]
    fc, tc, hvc = framed(torch.zeros(n, 512 * nh, h, w), 0, tdt)
    check(L.dbx_heads_forward_fused_heads(C.byref(d), C.byref(xv), ptr(w1f), ptr(b1), C.byref(hvc), ptr(w2f), ptr(b2), karr, nh,
                                          (C.c_void_p * nh)(*[o.data_ptr() for o in outs_h]), ptr(sc), stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(fa, fc) and torch.equal(torch.cat(outs_h, 1), out_a)
    assert torch.equal(fa, fb) and float(ta.float().abs().sum()) > 0
    scale = float(out_b.abs().max())
    assert float((out_a - out_b).abs().max()) <= 2e-5 * scale, (float((out_a - out_b).abs().max()), scale)
    hid = tb.permute(0, 3, 1, 2).float()
    ref = torch.cat([F.conv2d(hid[:, 512 * i:512 * (i + 1)], w2[i].to(tdt).float()) for i in range(nh)], 1) + b2[:ktot].view(1, -1, 1, 1)
    assert float((out_a - ref).abs().max()) <= 1e-4 * scale
    # about half of the hidden map is dropped, the rest doubled: the dropout bits are live
    frac = float((ta == 0).float().mean())
    assert 0.35 < frac < 0.85, frac


@pytest.mark.parametrize('dtn', ['f16', 'bf16'])
@pytest.mark.parametrize('ks,n,h,w', [([1, 4, 4, 8], 3, 60, 60), ([1, 4], 6, 60, 60), ([1, 4, 4, 8], 2, 57, 83)])
def test_heads_forward_fused_on_the_8phase_kernel(ks, n, h, w, dtn):
    """The same call on the 8-phase kernel (dbx_heads_forward_fusable == 2: plain packed weights, the second weights as a plain [64][512 nh]
    image with every head's rows at 0..): the hidden map against fp32 torch on the rounded operands with the SAME keep bits as the ws
    kernel's (the backward kernels regenerate them from the hash), the head outputs against the second conv of the hidden map it wrote
    (fp32 summation order), the per-head destinations bitwise the [N][sum k][H][W] form, and a second launch bitwise equal."""
    if os.environ.get('DBX_P8') == '0' or os.environ.get('DBX_P8_HEADS') == '0' or os.environ.get('DBX_CONV_VARIANT'):
        pytest.skip('this process keeps the heads forward off the 8-phase kernel')
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    nh, ktot = len(ks), sum(ks)
    g = torch.Generator(device='cpu').manual_seed(78)
    x = torch.relu(torch.randn(n, 768, h, w, generator=g)).cuda()
    w1 = (torch.randn(512 * nh, 768, 1, 1, generator=g) * 0.05).cuda()
    b1 = torch.randn(512 * nh, generator=g).cuda()
    w2 = [(torch.randn(k, 512, 1, 1, generator=g) * 0.05).cuda().contiguous() for k in ks]
    b2 = torch.zeros(64, device='cuda'); b2[:ktot] = torch.randn(ktot, generator=g).cuda()
    fx, tx, xv = framed(x, 1, tdt)
    seed = 0x1234ABCD
    d = ConvDesc(dt, 1, 1, 0, 768, 512 * nh, _lib.EPI_BIAS | _lib.EPI_DROPHASH, seed)
    karr = (C.c_int32 * nh)(*ks)
    fa, ta, hva = framed(torch.zeros(n, 512 * nh, h, w), 0, tdt)
    assert L.dbx_heads_forward_fusable(C.byref(d), C.byref(xv), C.byref(hva), karr, nh) == 2
    w1p = pack(L, dt, w1, 768, 512 * nh, mode=0)
    d2 = ConvDesc(dt, 1, 1, 0, 512 * nh, 64, 0)
    w2p = torch.zeros(L.dbx_conv_packed_elems(C.byref(d2)) * 2, dtype=torch.uint8, device='cuda')
    for i, (wt, k) in enumerate(zip(w2, ks)):
        check(L.dbx_pack_weight(dt, 0, ptr(wt), k, 512, 1, 1, ptr(w2p), 64, 512 * nh, 0, 512 * i, stream_ptr()))
    sc = torch.empty(L.dbx_heads_forward_fused_scratch_bytes(nh, n * h * w), dtype=torch.uint8, device='cuda')
    res = []
    for rep in range(2):
        fa, ta, hva = framed(torch.zeros(n, 512 * nh, h, w), 0, tdt)
        out_a = torch.full((n, ktot, h, w), 7.0, device='cuda')
        check(L.dbx_heads_forward_fused(C.byref(d), C.byref(xv), ptr(w1p), ptr(b1), C.byref(hva), ptr(w2p), ptr(b2), karr, nh, ptr(out_a), ptr(sc),
                                        stream_ptr()))
        torch.cuda.synchronize()
        res.append((fa, ta, out_a))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][2], res[1][2])
    fa, ta, out_a = res[0]
    outs_h = [torch.full((n, k, h, w), 7.0, device='cuda') for k in ks]
    fc, tc, hvc = framed(torch.zeros(n, 512 * nh, h, w), 0, tdt)
    check(L.dbx_heads_forward_fused_heads(C.byref(d), C.byref(xv), ptr(w1p), ptr(b1), C.byref(hvc), ptr(w2p), ptr(b2), karr, nh,
                                          (C.c_void_p * nh)(*[o.data_ptr() for o in outs_h]), ptr(sc), stream_ptr()))
    # the ws kernel on the same problem (fragment-order weights): the same keep bits, values equal up to the output rounding
    dw = ConvDesc(dt, 1, 1, 0, 768, 512 * nh, _lib.EPI_BIAS | _lib.EPI_DROPHASH | _lib.CONV_WFRAG, seed)
    fb, tb, hvb = framed(torch.zeros(n, 512 * nh, h, w), 0, tdt)
    check(L.dbx_conv_forward(C.byref(dw), C.byref(xv), ptr(pack(L, dt, w1, 768, 512 * nh, mode=4)), ptr(b1), C.byref(hvb), None, None, 0, stream_ptr()))
    # ... and the 8-phase kernel without the second convs (plain dbx_conv_forward on the same descriptor): bitwise the fused call's hidden map
    fd, td, hvd = framed(torch.zeros(n, 512 * nh, h, w), 0, tdt)
    check(L.dbx_conv_forward(C.byref(d), C.byref(xv), ptr(w1p), ptr(b1), C.byref(hvd), None, None, 0, stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(fa, fc) and torch.equal(torch.cat(outs_h, 1), out_a) and torch.equal(fa, fd)
    hid, hid_ws = ta.permute(0, 3, 1, 2).float(), tb.permute(0, 3, 1, 2).float()
    ref = F.conv2d(x.to(tdt).float(), w1.to(tdt).float(), b1)
    tol = (2e-2 if dtn == 'bf16' else 3e-3)
    big = ref.abs() > 0.1
    assert torch.equal((hid != 0)[big], (hid_ws != 0)[big])
    assert torch.allclose(hid, hid_ws, rtol=tol, atol=tol)
    kept = big & (hid != 0)
    assert torch.allclose(hid[kept], 2 * ref[kept], rtol=2 * tol, atol=2 * tol)
    frac = float((hid == 0).float().mean())
    assert 0.35 < frac < 0.85, frac
    out_ref = torch.cat([F.conv2d(hid[:, 512 * i:512 * (i + 1)], w2[i].to(tdt).float()) for i in range(nh)], 1) + b2[:ktot].view(1, -1, 1, 1)
    scale = float(out_ref.abs().max())
    assert float((out_a - out_ref).abs().max()) <= 1e-4 * scale, (float((out_a - out_ref).abs().max()), scale)


@pytest.mark.parametrize('dtn', ['f16', 'bf16'])
@pytest.mark.parametrize('drop', ['hash', 'none'])
@pytest.mark.parametrize('geom', [(3, 60, 60), (2, 23, 37), (5, 12, 30)])
def test_heads1_wgrad_gen_equals_wgrad_of_the_materialised_hidden_gradient(geom, drop, dtn):
    """dbx_heads1_wgrad_gen (d_hid = keep * (d_out W2) generated inside the weight-gradient kernel) against dbx_head2_dgrad into memory +
    dbx_conv_wgrad_slice on it.  W2 is pre-rounded to the compute dtype (the generating MFMA takes it in that dtype), so the two hidden
    gradients differ only where the fp32 sum of <= 8 exact products rounds differently: dW1 / db1 agree to fp32-sum tolerance."""
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    n, h, w = geom
    ks = [1, 4, 4, 8]
    nh = len(ks)
    g = torch.Generator(device='cpu').manual_seed(5 + h)
    dout = torch.zeros(n, 8 * nh, h, w)
    for i, k in enumerate(ks):
        dout[:, 8 * i:8 * i + k] = torch.randn(n, k, h, w, generator=g)
    w2 = [(torch.randn(k, 512, generator=g) * 0.05).to(tdt).float().cuda().contiguous() for k in ks]
    x = torch.randn(n, 256, h, w, generator=g)
    fo, to, dv = framed(dout, 0, tdt)
    fx, tx, xv = framed(x, 1, tdt)
    fd, td, dhv = framed(torch.zeros(n, 512 * nh, h, w), 1, tdt)
    use_hash, seed = (1, 0xBEEF) if drop == 'hash' else (0, 0)
    karr = (C.c_int32 * nh)(*ks)
    wp = (C.c_void_p * nh)(*[t.data_ptr() for t in w2])
    check(L.dbx_head2_dgrad(dt, C.byref(dv), wp, karr, nh, C.byref(dhv), None, 512 * nh, use_hash, seed, stream_ptr()))
    sc = torch.empty(L.dbx_conv_wgrad_scratch_bytes(dt, C.byref(dhv), C.byref(xv), 1, 1), dtype=torch.uint8, device='cuda')
    dw1 = torch.full((512 * nh, 300, 1, 1), 7.0, device='cuda'); db1 = torch.full((512 * nh,), 7.0, device='cuda')
    dw2 = torch.full((512 * nh, 300, 1, 1), 7.0, device='cuda'); db2 = torch.full((512 * nh,), 7.0, device='cuda')
    check(L.dbx_conv_wgrad_slice(dt, C.byref(dhv), C.byref(xv), 1, 1, 0, 512 * nh, 256, ptr(dw1), 300, 44, ptr(db1), ptr(sc), 0, stream_ptr()))
    check(L.dbx_heads1_wgrad_gen(dt, C.byref(dv), C.byref(xv), wp, karr, nh, use_hash, seed, 256, ptr(dw2), 300, 44, ptr(db2), ptr(sc), stream_ptr()))
    torch.cuda.synchronize()
    assert float(dw1[:, 44:300].abs().sum()) > 0 and torch.equal(dw1[:, :44], dw2[:, :44])
    sw, sb = float(dw1[:, 44:300].abs().max()), float(db1.abs().max())
    assert float((dw1 - dw2).abs().max()) <= 2e-4 * sw, (float((dw1 - dw2).abs().max()), sw)
    assert float((db1 - db2).abs().max()) <= 2e-4 * sb, (float((db1 - db2).abs().max()), sb)


def _heads1_dgrad_setup(L, dt, tdt, n, h, w, ks, seed0, drop):
    nh = len(ks)
    g = torch.Generator(device='cpu').manual_seed(seed0)
    dout = torch.zeros(n, 8 * nh, h, w)
    for i, k in enumerate(ks):
        dout[:, 8 * i:8 * i + k] = torch.randn(n, k, h, w, generator=g)
    w2 = [(torch.randn(k, 512, generator=g) * 0.05).to(tdt).float().cuda().contiguous() for k in ks]
    w1 = [(torch.randn(512, 768, 1, 1, generator=g) * 0.03).cuda().contiguous() for _ in ks]      # conv5_1 weights [hidden][768 inputs]
    gate = torch.randn(n, 256, h, w, generator=g)
    fo, to, dv = framed(dout, 0, tdt)
    fg, tg, gv = framed(gate, 1, tdt)
    fd, td, dhv = framed(torch.zeros(n, 512 * nh, h, w), 1, tdt)
    use_hash, seed = (1, 0xF00D) if drop == 'hash' else (0, 0)
    karr = (C.c_int32 * nh)(*ks)
    wp = (C.c_void_p * nh)(*[t.data_ptr() for t in w2])
    check(L.dbx_head2_dgrad(dt, C.byref(dv), wp, karr, nh, C.byref(dhv), None, 512 * nh, use_hash, seed, stream_ptr()))
    # W1^T restricted to input channels 512..767: rows = those 256 channels, K = the hidden channels of all heads, fragment order
    d = ConvDesc(dt, 1, 1, 0, 512 * nh, 256, 0)
    wimg = torch.zeros(L.dbx_conv_packed_elems(C.byref(d)) * _lib.ESIZE[dt], dtype=torch.uint8, device='cuda')
    for i, wt in enumerate(w1):
        check(L.dbx_pack_weight(dt, 5, ptr(wt), 512, 768, 1, 1, ptr(wimg), 256, 512 * nh, -512, 512 * i, stream_ptr()))
    keep = (fo, fg, fd, w2, w1, wimg)
    return keep, dv, gv, dhv, wp, karr, nh, use_hash, seed, wimg


@pytest.mark.parametrize('dtn', ['f16', 'bf16'])
@pytest.mark.parametrize('drop', ['hash', 'none'])
@pytest.mark.parametrize('geom', [(3, 60, 60, [1, 4, 4, 8]), (2, 23, 37, [1, 4, 4, 8]), (5, 12, 30, [2, 4]), (1, 9, 11, [1])])
def test_heads1_dgrad_gen_equals_the_gated_gemm_on_the_materialised_hidden_gradient(geom, drop, dtn):
    """dbx_heads1_dgrad_gen (d_hid generated in registers as the GEMM's B operand) against dbx_head2_dgrad into memory + the ws / band 1x1
    kernel with DBX_EPI_GATE on it.  W2 pre-rounded to the compute dtype: the two hidden gradients agree except for fp32 summation order,
    the outputs to 16-bit rounding of sums in different orders; halo of the output untouched."""
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    n, h, w, ks = geom
    keep, dv, gv, dhv, wp, karr, nh, use_hash, seed, wimg = _heads1_dgrad_setup(L, dt, tdt, n, h, w, ks, 17 + h, drop)
    fy1, ty1, yv1 = framed(torch.zeros(n, 256, h, w), 1, tdt)
    fy2, ty2, yv2 = framed(torch.zeros(n, 256, h, w), 1, tdt)
    d = ConvDesc(dt, 1, 1, 0, 512 * nh, 256, _lib.EPI_GATE, 0)
    plan = _lib.ConvPlan()
    check(L.dbx_conv_plan(C.byref(d), C.byref(dhv), C.byref(yv1), C.byref(plan)))
    if plan.w_frag:
        d1 = ConvDesc(dt, 1, 1, 0, 512 * nh, 256, _lib.EPI_GATE | _lib.CONV_WFRAG, 0)
        check(L.dbx_conv_forward(C.byref(d1), C.byref(dhv), ptr(wimg), None, C.byref(yv1), C.byref(gv), None, 0, stream_ptr()))
    else:       # small problems: the row-major transposed image for the LDS kernels
        w1 = keep[4]
        wrow = torch.zeros(L.dbx_conv_packed_elems(C.byref(d)) * _lib.ESIZE[dt], dtype=torch.uint8, device='cuda')
        for i, wt in enumerate(w1):
            check(L.dbx_pack_weight(dt, 1, ptr(wt), 512, 768, 1, 1, ptr(wrow), 256, 512 * nh, -512, 512 * i, stream_ptr()))
        check(L.dbx_conv_forward(C.byref(d), C.byref(dhv), ptr(wrow), None, C.byref(yv1), C.byref(gv), None, 0, stream_ptr()))
    check(L.dbx_heads1_dgrad_gen(dt, C.byref(dv), wp, karr, nh, use_hash, seed, ptr(wimg), C.byref(yv2), C.byref(gv), stream_ptr()))
    torch.cuda.synchronize()
    a, b = ty1.float(), ty2.float()
    assert float(a.abs().sum()) > 0
    tol = (3e-3 if dtn == 'f16' else 2e-2) * float(a.abs().max())
    assert float((a - b).abs().max()) <= tol, (float((a - b).abs().max()), float(a.abs().max()))
    assert float(ty2[:, 0].float().abs().sum()) == 0 and float(ty2[:, :, 0].float().abs().sum()) == 0      # halo rows / columns untouched
    assert torch.equal((b == 0), (a == 0)) or float(((b == 0) != (a == 0)).float().mean()) < 1e-3           # same gate pattern


@pytest.mark.parametrize('dtn', ['f16', 'bf16'])
@pytest.mark.parametrize('drop', ['hash', 'none'])
def test_heads_gen_16bit_kernels_equal_their_fp32_reference_forms_exactly(drop, dtn):
    """The MFMA generators of the 16-bit step (wgrad_wide2_kernel<T, true>, heads1_dgrad_gen_kernel<T>) against the one-thread-per-output fp32
    instantiations the parity suite runs against the reference (csrc/heads_ref_f32.hip) on operands whose every product and partial sum is
    exactly representable (small integers and halves): dW1 / db1 BITWISE equal, d_x equal to the fp32 result rounded once to the 16-bit type.
    Ties the kernels bench.py times to the ones test_training_step_f32_with_the_16bit_backward_structure_vs_reference pins to the reference."""
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    n, h, w, ks = 3, 60, 60, [1, 4, 4, 8]
    nh = len(ks)
    g = torch.Generator(device='cpu').manual_seed(77)

    def ri(shape, lo, hi, scale=1.0):
        return torch.randint(lo, hi + 1, shape, generator=g).float() * scale
    dout = torch.zeros(n, 8 * nh, h, w)
    for i, k in enumerate(ks):
        dout[:, 8 * i:8 * i + k] = ri((n, k, h, w), -2, 2)
    w2 = [ri((k, 512), -2, 2, 0.5).cuda().contiguous() for k in ks]
    w1 = [ri((512, 768, 1, 1), -2, 2, 0.5).cuda().contiguous() for _ in ks]
    x = ri((n, 256, h, w), -3, 3)
    gate = ri((n, 256, h, w), -1, 1)
    use_hash, seed = (1, 0xACE1) if drop == 'hash' else (0, 0)
    karr = (C.c_int32 * nh)(*ks)
    wp = (C.c_void_p * nh)(*[t.data_ptr() for t in w2])
    res = {}
    for name, d_, td_ in (('lo', dt, tdt), ('f32', _lib.F32, torch.float32)):
        fo, to, dv = framed(dout, 0, td_)
        fx, tx, xv = framed(x, 1, td_)
        fg, tg, gv = framed(gate, 1, td_)
        fy, ty, yv = framed(torch.zeros(n, 256, h, w), 1, td_)
        dz = View(None, n, h, w, 1, 512 * nh, 0, 512 * nh)
        sc = torch.empty(max(1024, L.dbx_conv_wgrad_scratch_bytes(d_, C.byref(dz), C.byref(xv), 1, 1)), dtype=torch.uint8, device='cuda')
        dw = torch.full((512 * nh, 300, 1, 1), 7.0, device='cuda'); db = torch.full((512 * nh,), 7.0, device='cuda')
        check(L.dbx_heads1_wgrad_gen(d_, C.byref(dv), C.byref(xv), wp, karr, nh, use_hash, seed, 256, ptr(dw), 300, 44, ptr(db), ptr(sc), stream_ptr()))
        dd = ConvDesc(d_, 1, 1, 0, 512 * nh, 256, 0)
        wimg = torch.zeros(L.dbx_conv_packed_elems(C.byref(dd)) * _lib.ESIZE[d_], dtype=torch.uint8, device='cuda')
        for i, wt in enumerate(w1):
            check(L.dbx_pack_weight(d_, 5 if name == 'lo' else 1, ptr(wt), 512, 768, 1, 1, ptr(wimg), 256, 512 * nh, -512, 512 * i, stream_ptr()))
        check(L.dbx_heads1_dgrad_gen(d_, C.byref(dv), wp, karr, nh, use_hash, seed, ptr(wimg), C.byref(yv), C.byref(gv), stream_ptr()))
        torch.cuda.synchronize()
        res[name] = (dw.clone(), db.clone(), ty.clone())
    (dwa, dba, ya), (dwb, dbb, yb) = res['lo'], res['f32']
    assert float(dwb[:, 44:300].abs().sum()) > 0 and float(dbb.abs().sum()) > 0 and float(yb.abs().sum()) > 0
    assert torch.equal(dwa, dwb) and torch.equal(dba, dbb)
    assert torch.equal(ya.float(), yb.to(tdt).float())
    if drop == 'hash':          # about half of the hidden gradient is dropped: the two runs must differ from the no-dropout ones
        assert 0.2 < float((yb != 0).float().mean()) < 0.6


@pytest.mark.parametrize('dtn', ['bf16', 'f16'])
@pytest.mark.parametrize('shape', [(3, 40, 72), (2, 24, 64), (5, 62, 90), (2, 240, 240), (2, 30, 70, 128)])
def test_conv_wgrad_with_the_pooling_backward_as_dz_equals_the_two_calls(shape, dtn):
    """dbx_conv_wgrad_pool_dz (conv1_2's weight gradient reading pool1's backward from d_p1 + the arg-max nibbles, wgrad3x3_strip_kernel<T, true>)
    against dbx_maxpool2x2_bwd_idx into memory + dbx_conv_wgrad on that map: dW and db bitwise equal (same kernel, same operand bits) -- on
    activations quantised so that ties and all-zero windows (gate bit clear) occur, widths that leave a ragged last strip, and the real
    conv1_2 geometry."""
    n, h, w = shape[:3]
    c = 64
    cx = shape[3] if len(shape) > 3 else 64                                           # (128 input channels: two ci tiles, the map is written by one of them)
    L = _lib.lib()
    dt, tdt = _lib.DTYPE_ID[dtn], TDT[dtn]
    g = torch.Generator(device='cpu').manual_seed(h * 7 + w)
    act = F.relu(torch.round(torch.randn(n, c, h, w, generator=g) * 2) / 2)          # the pooled layer's output (conv1_2 after its ReLU)
    dy = torch.randn(n, c, h // 2, w // 2, generator=g)
    x = torch.randn(n, cx, h, w, generator=g)                                         # conv1_2's input (conv1_1's output)
    fa, ta, av = framed(act.cuda(), 1, tdt)
    fp, tp, pv = framed(torch.zeros(n, c, h // 2, w // 2), 0, tdt)
    idx = torch.zeros(L.dbx_maxpool_idx_bytes(n, h, w, c) + 16, dtype=torch.uint8, device='cuda')
    check(L.dbx_maxpool2x2_idx(dt, C.byref(av), C.byref(pv), ptr(idx), stream_ptr()))
    fdy, tdy, dyv = framed(dy.cuda(), 0, tdt)
    fx, tx, xv = framed(x.cuda(), 1, tdt)
    fz, tz, zv = framed(torch.zeros(n, c, h, w), 1, tdt)
    assert L.dbx_conv_wgrad_pool_dz_ok(dt, C.byref(zv), C.byref(xv), 3, 3) == 1
    check(L.dbx_maxpool2x2_bwd_idx(dt, ptr(idx), C.byref(dyv), C.byref(zv), 0, 1, stream_ptr()))
    sc = torch.empty(L.dbx_conv_wgrad_scratch_bytes(dt, C.byref(zv), C.byref(xv), 3, 3), dtype=torch.uint8, device='cuda')
    dw1 = torch.full((c, cx, 3, 3), 7.0, device='cuda'); db1 = torch.full((c,), 7.0, device='cuda')
    dw2 = torch.full((c, cx, 3, 3), 7.0, device='cuda'); db2 = torch.full((c,), 7.0, device='cuda')
    check(L.dbx_conv_wgrad(dt, C.byref(zv), C.byref(xv), 3, 3, 1, c, cx, ptr(dw1), ptr(db1), ptr(sc), 0, stream_ptr()))
    zshape = View(None, n, h, w, 1, c, 0, c)                                          # the map is NOT handed over: shape only
    check(L.dbx_conv_wgrad_pool_dz(dt, C.byref(dyv), ptr(idx), c, C.byref(zshape), C.byref(xv), 3, 3, 1, c, cx, ptr(dw2), ptr(db2), ptr(sc), 0, 0, stream_ptr()))
    # write_dz: the same call also leaves the un-pooled gradient map in memory (frame incl. its zero halo; here the destination starts as garbage)
    fz3, tz3, zv3 = framed(torch.full((n, c, h, w), 3.0), 1, tdt)
    tz3[:, 0] = 5.0; tz3[:, -1] = 5.0; tz3[:, :, 0] = 5.0; tz3[:, :, -1] = 5.0
    guard_before = fz3.clone()
    dw3 = torch.full((c, cx, 3, 3), 7.0, device='cuda'); db3 = torch.full((c,), 7.0, device='cuda')
    check(L.dbx_conv_wgrad_pool_dz(dt, C.byref(dyv), ptr(idx), c, C.byref(zv3), C.byref(xv), 3, 3, 1, c, cx, ptr(dw3), ptr(db3), ptr(sc), 0, 1, stream_ptr()))
    torch.cuda.synchronize()
    assert float(dw1.abs().sum()) > 0 and float(db1.abs().sum()) > 0
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2)
    assert torch.equal(dw1, dw3) and torch.equal(db1, db3)
    assert torch.equal(tz3, tz)                                                       # the whole frame, halo zeros included
    lo = (fz3.numel() - tz3.numel()) // 2
    assert torch.equal(fz3[:lo], guard_before[:lo]) and torch.equal(fz3[lo + tz3.numel():], guard_before[lo + tz3.numel():])   # guard bands untouched
    # ... and the pair is the gradient torch computes through ReLU -> MaxPool2d on the same rounded operands
    zr = tz[:, 1:1 + h, 1:1 + w].permute(0, 3, 1, 2).float()
    xr = tx[:, 1:1 + h, 1:1 + w].permute(0, 3, 1, 2).float()
    ref = torch.nn.grad.conv2d_weight(xr, (c, cx, 3, 3), zr, padding=1)
    assert float((dw2 - ref).abs().max()) <= 2e-3 * float(ref.abs().max())
    # odd extents, 3-channel-group mismatches: the query says no
    assert L.dbx_conv_wgrad_pool_dz_ok(dt, C.byref(View(None, n, h + 1, w, 1, c, 0, c)), C.byref(xv), 3, 3) == 0
    assert L.dbx_conv_wgrad_pool_dz_ok(_lib.F32, C.byref(zshape), C.byref(xv), 3, 3) == 0
