"""Every forward-conv kernel conv_forward_t (csrc/conv_igemm.hip) can select in a default process, pinned with exact-integer cases.

Each case (a) asks dbx_conv_plan and asserts kernel id, tile, w_frag and the full NAME against expected_plan() below -- the dispatcher's
rule restated, with the device's CU count where the rule uses it (the 8-phase schedules and their items >= 3 CUs / 4 rule; the shapes are
sized for 256 CUs and a device on which a shape no longer selects its path FAILS with the computed plan in the message) -- plus the
premise the case was sized for (7- and 8-unit tiles mixed, the round-up branch, a ragged last tile, an image seam inside a tile);
(b) packs the weights as the plan says (mode 4 / 5 + DBX_CONV_WFRAG when w_frag, else 0 / 1; the gated cases are data gradients:
transposed, flipped weights); (c) builds x between zero guard bands with a zero halo, y with -5 in its halo and guard bands and 7 at
every pixel a kernel has to write; (d, e) launches and asserts that the WHOLE y buffer, guard bands included, equals the float64
reference of tests/conv_ref.py inside the image and its initial content everywhere else (compared as numbers: two kernels clear the
sign bit of a zero on purpose), and that x and the gate are unchanged; (f) launches again into a fresh buffer: bitwise equal; (g) where
the path takes DBX_EPI_ACCUM, launches onto a y that holds the reference: exactly 2 x reference.  conv_ref's docstring derives the zero
tolerance; its premise is asserted per case and dtype from the reference alone before anything is launched, and so is a sensitivity
check: the reference with one (pixel, tap) term removed at the last pixel / at the first pixel behind a seam (moved to the nearest
pixel within 32 where the removal shows), and with the image transposed, differs from the reference.

Kernel names covered (case names in brackets; shapes are about the smallest that select the path at 256 CUs):
  conv3x3_p8_kernel<T,3>        [p8-3x3-relu-mixed, p8-3x3-gate, p8-3x3-bias-roundup, pool-p8]
  conv3x3_p8_kernel<T,1>        [p8-1x1-none, p8-1x1-gate]
  conv3x3_p8_kernel<T,1,1>      [p8-heads]  (this case also pins dbx_drop_hash32, restated here as drop_keep)
  conv3x3_p8w_kernel<T,3>       [p8w-3x3-relu-mixed, p8w-3x3-bias, p8w-3x3-gate, pool-p8w]  (couts % 128 == 0 and % 256 != 0: 384 here)
  conv3x3_ws_kernel<T,1,3,0>    [ws-3x3-wm1: 256 -> 256 on 29-pixel rows: 180 8-phase tiles < 192, 192 ws tiles over the frame rows]
  conv3x3_ws_kernel<T,2,3,0>    [ws-3x3-wm2: 320 -> 384: the p8w kernel wants cin % 128 == 0]
  conv3x3_ws_kernel<T,1,1,0>    [ws-1x1: 768 -> 512]
  conv3x3_ws_kernel<T,1,1,1>    [ws-1x1-heads: 128 -> 1024 with bias + hash dropout; the 8-phase kernel needs >= 4 K tiles of 64 channels]
  conv3x3_band_kernel<T,256,256> [band-256x256]   <T,144,128> [band-144x128]   <T,144,64> [band-144x64]
  conv3x3_band_kernel<T,192,128> [band-192x128]   <T,192,64> [band-192x64]: reachable with DBX_BAND144 unset -- one image whose 144-pixel
                                tiles number more than 256 / N tiles while the 192-pixel ones do not (36864 < frame positions <= 49152)
  conv3x3_band_kernel<T,288,128> [band-288x128]   <T,512,128> [band-512x128-accum]   <T,512,64> [band-512x64]
  conv3x3_band_kernel<T,256,128> [band-256x128]   <T,128,64> [band-128x64]   <T,256,64> [band-256x64]
  conv3x3_c64p_kernel<T,256,64> [c64p-64, c64p-wide]      conv3x3_c64_kernel<T,256,64> [c64-accum]      conv3x3_c8_kernel<T,256,64> [c8]
  conv_igemm_dma_kernel<T,256,64> [dma-5x5-n64, dma-yc8]  <T,256,256> [dma-1x1-wide, split]  <T,256,128> [dma-5x5-n128]  (f32 too)
  conv_igemm_kernel<T,256,64>   [igemm-1x1-n64, igemm-yc8, igemm-smallc-n64]   <T,128,128> [igemm-1x1-n128, igemm-smallc-n128]  (f32 too)
dbx_conv_plan cannot describe a second destination: the split case's kernel (the 256 x 256 LDS-ring tiles) is read off the dispatcher,
not asserted.  The fused second heads convs (w2f / part) are not launched here; test_hip_kernels.py keeps them.

Content variants on one case per family (p8, p8w, ws, band, c64p, c8, dma, igemm): single impulses in x (corners of the first and last
image, either side of every seam, the last pixel, column W - 1) under dense weights -- the expected y is the bias plus at most k x k
shifted weight columns, so a failure names the pixel and tap; channel-slice views (x read at c_off 64 of a wider frame whose other
channels hold 1000 at every image pixel, y written at c_off 64 between sentinels; the c8 kernel needs ld == 8 for x, so only its y is
a slice); y->c = 8 of 64 packed couts on the LDS-ring and the register-staged kernel (dma-yc8, igemm-yc8); the pooled second destination of both 8-phase kernels with the index
planes starting as 0xFF bytes and compared with a first-maximum arg-max on windows with (asserted) ties.

Cost.  References (float64 on the CPU, computed once per case and shared by its dtypes and variants; tests/conv_ref.py has the
per-case times): 46 s for the whole table on 8 threads.  On an MI355X host with 16 threads the 121 tests of this file took 27 s in
all, references included; the slowest five: band-512x64-bf16 3.96 s, band-512x128-accum-bf16 3.04 s, ws-3x3-wm2-bf16 1.62 s,
p8-3x3-bias-roundup-bf16 1.23 s, p8-3x3-relu-mixed-bf16 1.17 s (each the first dtype of its case: it pays for the reference)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as R                                    # noqa: E402
from heads_ref import drop_keep                         # noqa: E402  (dbx_drop_hash32 restated; shared with the heads backward's reference)

from densebox_amd import _lib                           # noqa: E402
from densebox_amd._lib import View, ConvDesc, check, ptr, stream_ptr   # noqa: E402

pytestmark = pytest.mark.gpu
_FORCING = ('DBX_CONV_VARIANT', 'DBX_P8', 'DBX_P8W', 'DBX_P8_HEADS', 'DBX_BAND144', 'DBX_BAND_ROWSKIP', 'DBX_C64P_WIDE')
if any(k in os.environ for k in _FORCING) or any(k.startswith('DBX_WS') for k in os.environ):
    pytest.skip('this process forces a kernel selection', allow_module_level=True)

TDT = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}
SENTINEL, HALO, FILL = 1000.0, -5.0, 7.0                 # all exact in bf16, f16 and fp32
BIAS, RELU, GATE, ACCUM, DROPHASH, WFRAG = _lib.EPI_BIAS, _lib.EPI_RELU, _lib.EPI_GATE, _lib.EPI_ACCUM, _lib.EPI_DROPHASH, _lib.CONV_WFRAG
EPI = {'none': 0, 'bias': BIAS, 'relu': BIAS | RELU, 'gate': GATE, 'heads': BIAS | DROPHASH}
SEED = 0x1234


def cdiv(a, b):
    return (a + b - 1) // b


class Case:
    """kernel: the name dbx_conv_plan must report (with the dtype filled in).  ci / co: channels the kernel reads / writes (a 'gate' case
    is the data gradient of a co -> ci ... forward layer co_fwd = ci, ci_fwd = co).  pad_ci: (16-bit, f32) cin_pad where it is not ci.
    premise: what the schedule must look like, see assert_plan.  accum: the path takes DBX_EPI_ACCUM (step g)."""

    def __init__(self, name, kernel, n, h, w, ci, co, k=3, cpad=1, epi='relu', q=0.25, xpad=1, ypad=1, yc=None, pad_ci=None, f32=False,
                 accum=False, accum_main=False, variants=False, premise=None):
        self.name, self.kernel, self.n, self.h, self.w, self.ci, self.co, self.k, self.cpad = name, kernel, n, h, w, ci, co, k, cpad
        self.epi, self.q, self.xpad, self.ypad, self.yc, self.pad_ci, self.f32 = epi, q, xpad, ypad, yc or co, pad_ci, f32
        self.accum, self.accum_main, self.variants, self.premise = accum, accum_main, variants, premise
        self.ho, self.wo = h + 2 * cpad - k + 1, w + 2 * cpad - k + 1
        self.cout_pad = cdiv(co, 64) * 64

    def cin_pad(self, dtn):
        return self.ci if self.pad_ci is None else self.pad_ci[1 if dtn == 'f32' else 0]

    def dtypes(self):
        return ('bf16', 'f16', 'f32') if self.f32 else ('bf16', 'f16')

    def __repr__(self):
        return self.name


P8, P8W, WS, BAND = 'conv3x3_p8_kernel<%s,', 'conv3x3_p8w_kernel<%s,3>', 'conv3x3_ws_kernel<%s,', 'conv3x3_band_kernel<%s,'
DMA, IGEMM = 'conv_igemm_dma_kernel<%s,', 'conv_igemm_kernel<%s,'
CASES = [
    # ---- 8-phase kernel, 256 x 256 tiles of 7 / 8 units of 32 pixels; wanted: >= 192 (pixel tile, cout tile) items at 256 CUs
    # 24442 pixels = 764 units (the last of 26 pixels) in 96 tiles of 7 (4) and 8 (92) units x 2 cout tiles = 192 items
    Case('p8-3x3-relu-mixed', P8 + '3>', 2, 101, 121, 128, 512, variants=True, premise='p8-mixed-ragged'),
    Case('p8-3x3-gate', P8 + '3>', 2, 101, 121, 128, 512, epi='gate', premise='p8-mixed-ragged'),
    # 57771 pixels = 1806 units: 226 tiles x 2 = 452 workgroups > 256 -> rounded up to 256 tiles (512 items) of 7 / 8 units
    Case('p8-3x3-bias-roundup', P8 + '3>', 3, 131, 147, 128, 512, epi='bias', premise='p8-roundup'),
    Case('p8-1x1-none', P8 + '1>', 2, 101, 121, 1024, 512, k=1, cpad=0, epi='none', q=0.125, premise='p8-mixed-ragged'),
    Case('p8-1x1-gate', P8 + '1>', 2, 101, 121, 1024, 512, k=1, cpad=0, epi='gate', q=0.125, premise='p8-mixed-ragged'),
    Case('p8-heads', P8 + '1,1>', 2, 101, 121, 256, 512, k=1, cpad=0, epi='heads', ypad=0, premise='p8-mixed-ragged'),
    # ---- 512 x 128 tiles of 14 .. 16 units: 32318 pixels = 1010 units in 64 tiles of 15 (14) and 16 (50) x 3 cout tiles = 192 items
    Case('p8w-3x3-relu-mixed', P8W, 2, 113, 143, 128, 384, variants=True, premise='p8w-mixed-ragged'),
    Case('p8w-3x3-bias', P8W, 2, 113, 143, 128, 384, epi='bias', premise='p8w-mixed-ragged'),
    Case('p8w-3x3-gate', P8W, 2, 113, 143, 128, 384, epi='gate', premise='p8w-mixed-ragged'),
    # ---- register-streamed weights, tiles over the frame rows.  29-pixel rows: 45994 pixels make 180 8-phase tiles (< 192), the
    # 13 x 122 x 31 = 49166 frame positions 192 ws tiles
    Case('ws-3x3-wm1', WS + '1,3,0>', 13, 122, 29, 256, 256, q=0.125, variants=True, premise='p8-too-few'),
    Case('ws-3x3-wm2', WS + '2,3,0>', 2, 133, 122, 320, 384, q=0.125, premise='ws-fill'),
    Case('ws-1x1', WS + '1,1,0>', 2, 101, 121, 768, 512, k=1, cpad=0, epi='none', q=0.125, premise='ws-fill'),
    Case('ws-1x1-heads', WS + '1,1,1>', 2, 61, 99, 128, 1024, k=1, cpad=0, epi='heads', ypad=0, premise='ws-fill'),
    # ---- LDS band kernel over the linearised frame rows (Q positions); 'band': Q no multiple of the tile, and with n > 1 an image
    # seam inside a tile
    Case('band-256x256', BAND + '256,256>', 2, 211, 120, 64, 256, accum=True, premise='band'),                # 202 tiles
    Case('band-144x128', BAND + '144,128>', 1, 161, 177, 64, 128, accum=True, premise='band'),                # Q 28819: 201 / 151 tiles of 144 / 192
    Case('band-144x64', BAND + '144,64>', 1, 161, 177, 128, 64, q=0.125, accum=True, premise='band'),
    Case('band-192x128', BAND + '192,128>', 1, 201, 197, 64, 128, accum=True, premise='band'),                # Q 39999: 278 / 209 tiles
    Case('band-192x64', BAND + '192,64>', 1, 201, 197, 128, 64, q=0.125, accum=True, premise='band'),
    Case('band-288x128', BAND + '288,128>', 1, 251, 270, 64, 128, accum=True, premise='band'),                # Q 68272: 267 tiles of 256 > 256 >= 238 of 288
    # tall tiles: 4 x 363 x 361 = 524172 positions = 1024 tiles of 512; 64 -> 128 without ACCUM belongs to the c64p kernel
    Case('band-512x128-accum', BAND + '512,128>', 4, 363, 359, 64, 128, accum=True, accum_main=True, premise='band'),
    Case('band-512x64', BAND + '512,64>', 4, 363, 359, 128, 64, q=0.125, accum=True, premise='band'),
    Case('band-256x128', BAND + '256,128>', 2, 37, 45, 64, 128, accum=True, variants=True, premise='band'),
    Case('band-128x64', BAND + '128,64>', 2, 37, 45, 128, 64, q=0.125, accum=True, premise='band'),
    Case('band-256x64', BAND + '256,64>', 2, 201, 210, 128, 64, q=0.125, accum=True, premise='band'),         # 333 tiles of 256 > 320
    # ---- halo-tile kernels, 8 x 32 pixel tiles (61 rows: a last tile row of 5; 250 columns: a last tile of 26)
    Case('c64p-64', 'conv3x3_c64p_kernel<%s,256,64>', 4, 61, 250, 64, 64, variants=True, premise='c64-256'),
    Case('c64p-wide', 'conv3x3_c64p_kernel<%s,256,64>', 8, 61, 250, 64, 128, premise='c64-512'),
    Case('c64-accum', 'conv3x3_c64_kernel<%s,256,64>', 4, 61, 250, 64, 64, accum=True, accum_main=True, premise='c64-256'),
    Case('c8', 'conv3x3_c8_kernel<%s,256,64>', 4, 61, 250, 3, 64, q=0.6, pad_ci=(8, 4), variants=True, premise='c64-256'),
    # ---- LDS-DMA ring kernel: 5x5 without padding, a 1x1 layer with 192 input channels (no multiple of 128: neither wide kernel)
    Case('dma-5x5-n64', DMA + '256,64>', 2, 21, 27, 64, 64, k=5, cpad=0, q=0.125, f32=True, accum=True),
    Case('dma-1x1-wide', DMA + '256,256>', 2, 21, 27, 192, 256, k=1, cpad=0, epi='none', f32=True, accum=True, variants=True),
    Case('dma-5x5-n128', DMA + '256,128>', 2, 21, 27, 64, 128, k=5, cpad=0, q=0.125, f32=True, accum=True),
    Case('dma-yc8', DMA + '256,64>', 2, 21, 27, 64, 64, k=5, cpad=0, q=0.125, yc=8, f32=True, accum=True),
    # ---- register-staged kernel: one K step (1x1, 128 bytes of input channels), and one 16-byte chunk per pixel on a map too small
    # for the c8 kernel
    Case('igemm-1x1-n64', IGEMM + '256,64>', 2, 21, 27, 32, 64, k=1, cpad=0, q=0.5, pad_ci=(64, 32), f32=True, accum=True),
    Case('igemm-1x1-n128', IGEMM + '128,128>', 2, 21, 27, 32, 128, k=1, cpad=0, q=0.5, pad_ci=(64, 32), f32=True, accum=True),
    Case('igemm-yc8', IGEMM + '256,64>', 2, 21, 27, 32, 64, k=1, cpad=0, q=0.5, yc=8, pad_ci=(64, 32), f32=True, accum=True),
    Case('igemm-smallc-n64', IGEMM + '256,64>', 2, 21, 27, 3, 64, q=0.6, pad_ci=(8, 4), f32=True, accum=True, variants=True),
    Case('igemm-smallc-n128', IGEMM + '128,128>', 2, 21, 27, 3, 128, q=0.6, pad_ci=(8, 4), f32=True, accum=True),
]
POOL_CASES = [
    Case('pool-p8', P8 + '3>', 2, 102, 122, 128, 512, premise='p8-mixed-ragged'),                                 # 24888 pixels: 98 tiles of 7 / 8
    Case('pool-p8w', P8W, 2, 114, 142, 128, 384, premise='p8w-mixed-ragged'),                                     # 32376 pixels: 64 tiles of 15 / 16
]
BY_NAME = {c.name: c for c in CASES + POOL_CASES}
RUNS = [(c, d) for c in CASES for d in c.dtypes()]
VARIANT_RUNS = [(c, d) for c in CASES if c.variants for d in ('bf16', 'f16')]
_ids = lambda r: '%s-%s' % (r[0].name, r[1])            # noqa: E731


class Problem:
    """What conv_forward_t sees of a call: the descriptor and the two views' geometry."""

    def __init__(self, c, dtn, epi=None, x_off=0, x_ld=None, y_off=0, y_ld=None):
        self.c, self.dtn, self.es = c, dtn, 4 if dtn == 'f32' else 2
        self.epi = EPI[c.epi] | (ACCUM if c.accum_main else 0) if epi is None else epi
        self.cin_pad, self.cout_pad, self.yc = c.cin_pad(dtn), c.cout_pad, c.yc
        self.xc = self.cin_pad
        self.x_off, self.x_ld = x_off, x_ld or self.xc
        self.y_off, self.y_ld = y_off, y_ld or self.yc


def sched8(M, nt, cus, lo, full):
    """p8_schedule / p8w_schedule: tiles of lo .. full units of 32 pixels, their number rounded up to whole rounds of CUs."""
    units = cdiv(M, 32)
    mt = cdiv(units, full)
    rounded = False
    if mt * nt > cus:
        up = cdiv(mt * nt, cus) * cus // nt
        if up > mt and units // up >= lo:
            mt, rounded = up, True
    base, extra = units // mt, units % mt
    ok = extra == 0 if base == full else lo <= base < full
    return dict(ok=ok, mt=mt, base=base, extra=extra, items=mt * nt, rounded=rounded, units=units)


def expected_plan(p, cus):
    """conv_forward_t's selection in a default process, restated: (kernel id, tile_m, tile_n, w_frag, name, notes)."""
    c, es, t = p.c, p.es, p.dtn
    b16 = es == 2
    n, h, w, k, epi = c.n, c.h, c.w, c.k, p.epi
    cin, cout, yc = p.cin_pad, p.cout_pad, p.yc
    x_wp, x_hp = w + 2 * c.xpad, h + 2 * c.xpad
    M = n * c.ho * c.wo
    cpt = cin * es // 16
    smallc = cpt < 8
    ktot_bytes = cdiv(k * k * cin * es, 128) * 128
    taps = k * k
    y16 = (p.y_off * es) % 16 == 0 and (p.y_ld * es) % 16 == 0
    sizes = (M < 1 << 24 and n * x_hp * x_wp * p.x_ld * es < 1 << 32 and 64 * ktot_bytes < 1 << 31 and
             n * (c.ho + 2 * c.ypad) * (c.wo + 2 * c.ypad) * p.y_ld < 1 << 32)
    notes = {}
    k3 = k == 3 and c.cpad == 1 and c.xpad == 1
    k1 = k == 1 and c.cpad == 0
    kk = epi & ~BIAS
    heads = k1 and epi == (BIAS | DROPHASH)
    kinds = kk == 0 or kk == RELU or (kk == GATE and not epi & BIAS)
    p8_ok = (not smallc and b16 and (k3 or k1) and (kinds or heads) and cin % 64 == 0 and (taps * (cin // 64)) % 2 == 0 and
             4 <= taps * (cin // 64) < 7000 and cout % 256 == 0 and yc == cout and y16 and sizes)
    if p8_ok:
        s = notes['p8'] = sched8(M, yc // 256, cus, 7, 8)
        p8_ok = s['ok'] and s['items'] >= cus * 3 // 4
    if p8_ok and ((k3 and cin >= 128) or (k1 and not heads and cin >= 1024) or heads):
        return (_lib.K_P8, 256, 256, 0, 'conv3x3_p8_kernel<%s,%s>' % (t, '1,1' if heads else (3 if k3 else 1)), notes)
    p8w_ok = (not smallc and b16 and k3 and kinds and cin % 128 == 0 and 9 * (cin // 64) < 7000 and cout % 128 == 0 and cout % 256 != 0 and
              yc == cout and y16 and sizes)
    if p8w_ok:
        s = notes['p8w'] = sched8(M, yc // 128, cus, 14, 16)
        p8w_ok = s['ok'] and s['items'] >= cus * 3 // 4
    if p8w_ok:
        return (_lib.K_P8, 512, 128, 0, 'conv3x3_p8w_kernel<%s,3>' % t, notes)
    # register-streamed weights: the plan prefers them on the 1x1 GEMMs, 128-cout-tile layers with >= 256 input channels, and the
    # 512 -> 512 / 256 -> 256 layers
    k1w = k1 and c.xpad <= 1 and cin % 128 == 0 and cout % 256 == 0
    ws_ok = (not smallc and b16 and (k3 or k1w) and not epi & (_lib.EPI_F32_NCHW | _lib.EPI_DROPMASK | ACCUM) and (k1w or not epi & DROPHASH) and
             cin % 64 == 0 and cin >= 128 and yc == cout and cout % 128 == 0 and (p.x_off * es) % 128 == 0 and y16)
    kw_ = epi & (RELU | GATE | DROPHASH)
    ws_ok = ws_ok and (kw_ in (0, RELU, GATE) if k3 else kw_ in (0, DROPHASH, GATE))
    wm = 1 if cout % 256 == 0 else 2
    qtot = n * h * x_wp
    if ws_ok:
        notes['ws_items'] = (qtot // (256 * wm)) * (yc // (256 // wm))
        ws_ok = h * x_wp >= 256 * wm + 8 and qtot < 1 << 30 and notes['ws_items'] >= 192
    ws_pref = k1w or (wm == 2 and cin >= 256) or (wm == 1 and ((cin >= 512 and cout >= 512) or (cin == 256 and cout == 256)))
    if ws_ok and ws_pref:
        if k1w and epi == (BIAS | DROPHASH):
            return (_lib.K_WS, 256, 256, 1, 'conv3x3_ws_kernel<%s,1,1,1>' % t, notes)
        if k1w:
            return (_lib.K_WS, 256, 256, 1, 'conv3x3_ws_kernel<%s,1,1,0>' % t, notes)
        if wm == 1:
            return (_lib.K_WS, 256, 256, 1, 'conv3x3_ws_kernel<%s,1,3,0>' % t, notes)
        return (_lib.K_WS, 512, 128, 1, 'conv3x3_ws_kernel<%s,2,3,0>' % t, notes)
    tiles8x32 = n * cdiv(h, 8) * cdiv(w, 32)
    notes['tiles8x32'] = tiles8x32

    def band(tm, tn):
        notes['band_q'], notes['band_tm'] = Q, tm
        return (_lib.K_BAND, tm, tn, 0, 'conv3x3_band_kernel<%s,%d,%d>' % (t, tm, tn), notes)
    if (not smallc and b16 and k3 and not epi & (_lib.EPI_F32_NCHW | _lib.EPI_DROPMASK | DROPHASH) and (cin * es) % 64 == 0 and yc % 64 == 0):
        Q = n * (h if h * x_wp >= 16 else x_hp) * x_wp            # tiles over the frame without its top / bottom halo rows
        tiles = lambda m: cdiv(Q, m)                               # noqa: E731
        tall = tiles(512) >= 1024
        few256, few128 = tiles(256) * (yc // 256) < 200, tiles(256) * (yc // 128) < 200
        if (cin == 64 and cout == 128 and yc == 128 and ktot_bytes == 1152 and not epi & ACCUM and y16 and tiles8x32 >= 512):
            return (_lib.K_C64, 256, 64, 0, 'conv3x3_c64p_kernel<%s,256,64>' % t, notes)
        if yc % 256 == 0 and cout % 256 == 0 and not few256:
            return band(256, 256)
        if n == 1:
            if yc % 128 == 0 and cout % 128 == 0 and yc <= 256 and tiles(144) * (yc // 128) <= 256 and tiles(192) * (yc // 128) >= 128:
                return band(144, 128)
            if (tiles(144) * (yc // 64) <= 256 and tiles(192) * (yc // 64) >= 128 and
                    not (yc % 128 == 0 and yc <= 256 and tiles(192) * (yc // 128) >= 128)):
                return band(144, 64)
            if yc % 128 == 0 and cout % 128 == 0 and yc <= 256 and 128 <= tiles(192) * (yc // 128) <= 256:
                return band(192, 128)
            if 128 <= tiles(192) * (yc // 64) <= 256:
                return band(192, 64)
            if yc == 128 and cout == 128 and tiles(256) > 256 and tiles(288) <= 256:
                return band(288, 128)
        if yc % 128 == 0 and cout % 128 == 0 and (not few128 or yc == 128):
            return band(512, 128) if tall else band(256, 128)
        if cin == 64 and cout == 64 and yc == 64 and ktot_bytes == 1152 and tiles8x32 >= 256:
            return (_lib.K_C64, 256, 64, 0, ('conv3x3_c64_kernel<%s,256,64>' if epi & ACCUM else 'conv3x3_c64p_kernel<%s,256,64>') % t, notes)
        if tall:
            return band(512, 64)
        if tiles(256) * (yc // 64) <= 320:
            return band(128, 64)
        return band(256, 64)
    if not smallc and ktot_bytes // 128 >= 2:
        if cout % 128 != 0 or yc <= 64:
            return (_lib.K_DMA, 256, 64, 0, 'conv_igemm_dma_kernel<%s,256,64>' % t, notes)
        if cout % 256 == 0 and yc % 256 == 0:
            return (_lib.K_DMA, 256, 256, 0, 'conv_igemm_dma_kernel<%s,256,256>' % t, notes)
        return (_lib.K_DMA, 256, 128, 0, 'conv_igemm_dma_kernel<%s,256,128>' % t, notes)
    if (smallc and b16 and k3 and cout == 64 and yc == 64 and p.x_ld * es == 16 and not epi & ~(BIAS | RELU) and ktot_bytes == 256 and
            tiles8x32 >= 256):
        return (_lib.K_C8, 256, 64, 0, 'conv3x3_c8_kernel<%s,256,64>' % t, notes)
    if cout % 128 != 0 or yc <= 64:
        return (_lib.K_IGEMM, 256, 64, 0, 'conv_igemm_kernel<%s,256,64>' % t, notes)
    return (_lib.K_IGEMM, 128, 128, 0, 'conv_igemm_kernel<%s,128,128>' % t, notes)


def check_premise(c, exp, cus):
    """The schedule property the case was sized for, from the restated rule's own numbers."""
    notes, M = exp[5], c.n * c.ho * c.wo
    if c.premise in ('p8-mixed-ragged', 'p8w-mixed-ragged'):
        s = notes['p8' if c.premise[2] == '-' else 'p8w']
        assert s['extra'] > 0 and not s['rounded'] and M % 32 != 0 and s['items'] >= cus * 3 // 4, (c.name, s)
    elif c.premise == 'p8-roundup':
        assert notes['p8']['rounded'] and notes['p8']['mt'] * (c.yc // 256) % cus == 0, (c.name, notes)
    elif c.premise == 'p8-too-few':
        assert notes['p8']['ok'] and notes['p8']['items'] < cus * 3 // 4 and notes['ws_items'] >= 192, (c.name, notes)
    elif c.premise == 'ws-fill':
        assert notes['ws_items'] >= 192, (c.name, notes)
    elif c.premise == 'band':
        Q, tm = notes['band_q'], notes['band_tm']
        assert Q % tm != 0 and (c.n == 1 or (c.h * (c.w + 2)) % tm != 0), (c.name, Q, tm)
    elif c.premise in ('c64-256', 'c64-512'):
        assert notes['tiles8x32'] >= int(c.premise[4:]) and c.h % 8 != 0 and c.w % 32 != 0, (c.name, notes)
    else:
        assert c.premise is None
    assert (c.w + 2) % 32 != 0 and c.h != c.w and (c.n >= 2 or c.kernel.startswith(BAND))     # n == 1: the single-image band tiles only


def assert_plan(L, c, p, xv, yv, cus=None):
    cus = cus or torch.cuda.get_device_properties(0).multi_processor_count
    exp = expected_plan(p, cus)
    want = c.kernel % p.dtn
    assert exp[4] == want, '%s %s: at %d CUs the dispatcher\'s rule gives %s, the case was sized for %s (%s)' % (c.name, p.dtn, cus, exp[:5], want, exp[5])
    d = ConvDesc(_lib.DTYPE_ID[p.dtn], c.k, c.k, c.cpad, p.cin_pad, p.cout_pad, p.epi, SEED)
    plan = _lib.ConvPlan()
    check(L.dbx_conv_plan(C.byref(d), C.byref(xv), C.byref(yv), C.byref(plan)))
    got = (plan.kernel, plan.tile_m, plan.tile_n, plan.w_frag, plan.name.decode())
    assert got == exp[:5], (c.name, p.dtn, got, exp[:5], cus)
    if p.epi == EPI[c.epi] | (ACCUM if c.accum_main else 0):
        check_premise(c, exp, cus)
    return plan


# ------------------------------------------------------------------------------------------------ operands, reference, sensitivity
_OPS, _REFS = {}, {}


def operands(c):
    """Integer operands per geometry (shared by the cases that differ in the epilogue only), left unchanged.  A 'gate' case convolves with
    the transposed, flipped weight of the forward layer ci_fwd = co -> co_fwd = ci."""
    tr = c.epi == 'gate'
    key = (c.n, c.h, c.w, c.ci, c.co, c.k, c.cpad, c.q, tr)
    if key not in _OPS:
        seed = (c.n * 7 + c.h * 131 + c.w * 17 + c.ci * 3 + c.co + c.k) % 100003
        shape_w = (c.ci, c.co) if tr else (c.co, c.ci)
        _OPS[key] = R.int_operands(seed, c.n, c.ci, shape_w[0], shape_w[1], c.k, c.h, c.w, c.q, c.ho, c.wo, c.co) + ({},)
    return _OPS[key]


def epilogue64(c, pre, gate):
    """The case's epilogue on float64 sums (bias included by conv_ref)."""
    if c.epi == 'relu':
        return pre.clamp(min=0)
    if c.epi == 'gate':
        return pre * (gate > 0)
    if c.epi == 'heads':                                     # Dropout(p = 0.5): kept values doubled
        keep = torch.from_numpy(drop_keep(SEED, c.n * c.ho * c.wo, c.co)).view(c.n, c.ho, c.wo, c.co).permute(0, 3, 1, 2)
        return 2 * pre * keep
    return pre


def sensitivity(c, x, we, ref):
    """Reference-only: a result that misses ONE (pixel, tap) term at the last pixel / at the first pixel behind a seam, or has the
    image transposed, must differ from the reference -- else the exact comparison could not see that fault on this case's operands."""
    tap = (c.k // 2, c.k // 2) if c.cpad else (0, 0)         # a tap whose input pixel exists for every output pixel
    seam = (1, 0, 0) if c.n > 1 else (0, c.ho - 1, 0)        # n == 1: the row seam before the last row
    for what, (img, oy, ox), step in (('last pixel', (c.n - 1, c.ho - 1, c.wo - 1), -1), ('seam', seam, 1)):
        lin, found = oy * c.wo + ox, False
        for j in range(32):                                  # the nearest pixel of the same tile (no tile is below 32 pixels) where it shows
            q = lin + step * j
            if not 0 <= q < c.ho * c.wo:
                break
            qy, qx = divmod(q, c.wo)
            term = we[:, :, tap[0], tap[1]] @ x[img, :, qy + tap[0] - c.cpad, qx + tap[1] - c.cpad]
            damaged = _col_epilogue(c, ref, ref.pre[img, :, qy, qx] - term, img, qy, qx)
            if not torch.equal(damaged[:c.yc], ref.post[img, :c.yc, qy, qx]):
                found = True
                break
        assert found, '%s: no pixel within 32 of the %s where a dropped tap changes the result' % (c.name, what)
    m = min(c.ho, c.wo, 16)
    crop = ref.post[0, :c.yc, :m, :m]
    assert not torch.equal(crop.transpose(1, 2), crop), '%s: the transposed image equals the image' % c.name


def _col_epilogue(c, ref, col, img, qy, qx):
    """The case's epilogue on one pixel's column of sums: the pixel's own mask is whatever turned ref.pre into ref.post there."""
    if c.epi == 'relu':
        return col.clamp(min=0)
    if c.epi in ('gate', 'heads'):
        pre, post = ref.pre[img, :, qy, qx], ref.post[img, :, qy, qx]
        scale = 2.0 if c.epi == 'heads' else 1.0
        passes = (post != 0) | (pre == 0)                    # (a zero sum tells nothing about its mask: take it as passing)
        return scale * col * passes
    return col


def reference(c, dtn):
    """Operands and reference of a case, computed once; premises (a), (b) and the accumulate premise asserted for this dtype, and the
    sensitivity check run, before anything touches the GPU."""
    x, w, bias, gate, convs = operands(c)
    if c.name not in _REFS:
        with_bias = R.BIAS if EPI[c.epi] & BIAS else 0
        if with_bias not in convs:
            convs[with_bias] = R.conv_ref(x, w, bias, c.k, c.cpad, with_bias, transposed=c.epi == 'gate')
        base = convs[with_bias]
        ref = R.Ref(base.pre, epilogue64(c, base.pre, gate), base.absum)
        assert float(ref.post.abs().max()) > 0 and (c.epi in ('none', 'bias') or not torch.equal(ref.post, ref.pre))
        sensitivity(c, x, R.effective_weight(w, c.epi == 'gate'), ref)
        _REFS[c.name] = ref
    ref = _REFS[c.name]
    R.assert_exact_premise(ref, dtn)
    if c.accum:
        R.assert_exact_premise(ref, dtn, times=2)
    return x, w, bias, gate, ref


# ------------------------------------------------------------------------------------------------ buffers
def make_frame(n, h, w, c, pad, tdt, data=None, fill=0.0, c_off=0, ld=None, halo=0.0):
    """Framed NHWC tensor between guard bands (the kernels walk frames linearly and read a tile and some frame rows past either end)
    + its View.  `halo` fills the frame and the guard bands; ld > c: the view is a channel slice and the other channels hold SENTINEL at
    every image pixel.  data: NCHW (any float dtype, CPU) for the view's channels, else `fill`."""
    ld = c if ld is None else ld
    hp, wp = h + 2 * pad, w + 2 * pad
    guard = max(8 * wp, 576 + 4 * wp) * ld
    flat = torch.full((2 * guard + n * hp * wp * ld,), halo, dtype=tdt, device='cuda')
    t = flat[guard:guard + n * hp * wp * ld].view(n, hp, wp, ld)
    inner = t[:, pad:pad + h, pad:pad + w]
    if ld > c:
        inner[...] = SENTINEL
    if data is not None:
        inner[..., c_off:c_off + c] = data.permute(0, 2, 3, 1).to(tdt).cuda()
    else:
        inner[..., c_off:c_off + c] = fill
    return flat, t, View(C.c_void_p(t.data_ptr()), n, h, w, pad, ld, c_off, c)


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def pack(L, dtn, c, w, cin_pad, frag):
    """dbx_pack_weight of the OIHW weight: mode 0 / 4 (forward), 1 / 5 (the gated cases: data gradient) into [cout_pad][taps][cin_pad]."""
    dt = _lib.DTYPE_ID[dtn]
    d = ConvDesc(dt, c.k, c.k, 0, cin_pad, c.cout_pad, 0)
    out = torch.zeros(L.dbx_conv_packed_elems(C.byref(d)) * _lib.ESIZE[dt], dtype=torch.uint8, device='cuda')
    mode = (1 if c.epi == 'gate' else 0) + (4 if frag else 0)
    wf = w.float().cuda().contiguous()
    check(L.dbx_pack_weight(dt, mode, ptr(wf), wf.shape[0], wf.shape[1], c.k, c.k, ptr(out), c.cout_pad, cin_pad, 0, 0, stream_ptr()))
    return out


def assert_frame(got_flat, want_flat, view_t, what):
    if torch.equal(got_flat, want_flat):
        return
    bad = (got_flat != want_flat).nonzero()
    i = int(bad[0])
    off = i - (view_t.data_ptr() - got_flat.data_ptr()) // got_flat.element_size()
    n, hp, wp, ld = view_t.shape
    where = 'guard band, element %d' % i
    if 0 <= off < view_t.numel():
        where = 'frame (image, row, column, channel) = %s' % (tuple(np.unravel_index(off, (n, hp, wp, ld))),)
    raise AssertionError('%s: %d of %d elements differ; first in the %s: got %r, expected %r' %
                         (what, bad.shape[0], got_flat.numel(), where, float(got_flat[i]), float(want_flat[i])))


class Launcher:
    """One case on the device: x, gate, packed weights, bias and the plan; fresh y buffers and launches on request."""

    def __init__(self, c, dtn, x, w, bias, gate, slices=False):
        self.L, self.c, self.dtn, self.tdt = _lib.lib(), c, dtn, TDT[dtn]
        cinp = c.cin_pad(dtn)
        x_off, x_ld, y_off, y_ld = 0, None, 0, None
        if slices:
            y_off, y_ld = 64, 64 + c.yc + 64
            if cinp >= 64:                                   # 128 bytes: what the ws kernel asks of x; the 16-byte-chunk inputs keep ld == c
                x_off, x_ld = 64, 64 + cinp + 64
        self.p = Problem(c, dtn, x_off=x_off, x_ld=x_ld, y_off=y_off, y_ld=y_ld)
        xs = torch.zeros(c.n, cinp, c.h, c.w, dtype=torch.float64)
        xs[:, :c.ci] = x
        self.fx, self.tx, self.xv = make_frame(c.n, c.h, c.w, cinp, c.xpad, self.tdt, data=xs, c_off=x_off, ld=x_ld)
        self.fg = self.gv = None
        if c.epi == 'gate':
            self.fg, self.tg, self.gv = make_frame(c.n, c.ho, c.wo, c.yc, 1, self.tdt, data=gate[:, :c.yc])
        self.bias = bias[:c.co].float().cuda() if EPI[c.epi] & BIAS else None
        self.fx0 = self.fx.clone()
        self.fg0 = self.fg.clone() if self.fg is not None else None
        fy, ty, yv = self.new_y()
        self.plan = assert_plan(self.L, c, self.p, self.xv, yv)
        self.wp = pack(self.L, dtn, c, w, cinp, self.plan.w_frag)

    def new_y(self, data=None, fill=FILL):
        c = self.c
        return make_frame(c.n, c.ho, c.wo, c.yc, c.ypad, self.tdt, data=data, fill=fill, c_off=self.p.y_off, ld=self.p.y_ld, halo=HALO)

    def expected(self, fy, ty, post):
        """The buffer as it must be after a launch: the initial content with the view's channels of every image pixel replaced."""
        c = self.c
        want = fy.clone()
        off = (ty.data_ptr() - fy.data_ptr()) // fy.element_size()
        wt = want[off:off + ty.numel()].view(ty.shape)
        wt[:, c.ypad:c.ypad + c.ho, c.ypad:c.ypad + c.wo, self.p.y_off:self.p.y_off + c.yc] = post.permute(0, 2, 3, 1).to(self.tdt).cuda()
        return want

    def launch(self, yv, epi=None):
        c, p = self.c, self.p
        e = (p.epi if epi is None else epi) | (WFRAG if self.plan.w_frag else 0)
        d = ConvDesc(_lib.DTYPE_ID[self.dtn], c.k, c.k, c.cpad, p.cin_pad, p.cout_pad, e, SEED)
        check(self.L.dbx_conv_forward(C.byref(d), C.byref(self.xv), ptr(self.wp), ptr(self.bias), C.byref(yv),
                                      C.byref(self.gv) if self.gv is not None else None, None, 0, stream_ptr()))

    def assert_inputs_unchanged(self):
        assert torch.equal(bits(self.fx), bits(self.fx0)), '%s %s: the input frame changed' % (self.c.name, self.dtn)
        if self.fg is not None:
            assert torch.equal(bits(self.fg), bits(self.fg0)), '%s %s: the gate frame changed' % (self.c.name, self.dtn)


def run_exact(c, dtn, slices=False):
    x, w, bias, gate, ref = reference(c, dtn)                # premises and sensitivity asserted in here, before any launch
    post = ref.post[:, :c.yc]
    K = Launcher(c, dtn, x, w, bias, gate, slices)
    tag = '%s %s%s' % (c.name, dtn, ' (channel slices)' if slices else '')
    first_fill = 0.0 if c.accum_main else FILL              # an accumulating epilogue adds onto zeros
    fy, ty, yv = K.new_y(fill=first_fill)
    want = K.expected(fy, ty, post)
    K.launch(yv)
    assert_frame(fy, want, ty, tag)
    fy2, ty2, yv2 = K.new_y(fill=first_fill)
    K.launch(yv2)
    assert torch.equal(bits(fy2), bits(fy)), '%s: the second launch differs from the first' % tag
    if c.accum:
        epi = K.p.epi | ACCUM
        fy3, ty3, yv3 = K.new_y(data=post)
        assert_plan(K.L, c, Problem(c, dtn, epi=epi, x_off=K.p.x_off, x_ld=K.p.x_ld, y_off=K.p.y_off, y_ld=K.p.y_ld), K.xv, yv3)   # the same kernel takes it
        want3 = K.expected(fy3, ty3, 2 * post)
        K.launch(yv3, epi=epi)
        assert_frame(fy3, want3, ty3, tag + ', accumulated onto the reference')
    K.assert_inputs_unchanged()


@pytest.mark.parametrize('run', RUNS, ids=_ids)
def test_conv_path_is_exact_on_integer_operands(run):
    run_exact(*run)


@pytest.mark.parametrize('run', VARIANT_RUNS, ids=_ids)
def test_conv_path_is_exact_on_channel_slices_of_wider_frames(run):
    run_exact(run[0], run[1], slices=True)


# ------------------------------------------------------------------------------------------------ impulses
def impulse_places(c):
    """(image, y, x) of the single 1 in x: corners of the first and last image, the last pixel before and the first after every image
    seam, the last pixel of all (the ragged last tile's), and column W - 1 of a middle row."""
    n, h, w = c.n, c.h, c.w
    out = [(img, y, xx) for img in sorted({0, n - 1}) for y in (0, h - 1) for xx in (0, w - 1)]
    for img in range(n - 1):
        out += [(img, h - 1, w - 1), (img + 1, 0, 0)]
    out += [(n - 1, h - 1, w - 1), (n - 1, h // 2, w - 1), (0, h // 2, 0)]
    seen, uniq = set(), []
    for p in out:
        if p not in seen:
            seen.add(p)
            uniq.append(p)
    return uniq


@pytest.mark.parametrize('run', VARIANT_RUNS, ids=_ids)
def test_conv_path_puts_every_impulse_under_each_tap_exactly_once(run):
    c, dtn = run
    assert c.epi in ('relu', 'none')
    x, w, bias, gate, ref = reference(c, dtn)
    K = Launcher(c, dtn, torch.zeros_like(x), w, bias, gate)
    tdt = K.tdt
    wd = w.cuda()                                            # [co][ci][k][k] float64
    bcol = bias[:c.co].cuda() if EPI[c.epi] & BIAS else torch.zeros(c.co, dtype=torch.float64, device='cuda')
    for i, (img, iy, ix) in enumerate(impulse_places(c)):
        ch = (0, c.ci - 1, c.ci // 2)[i % 3]
        K.tx[img, c.xpad + iy, c.xpad + ix, ch] = 1.0
        pre = bcol.view(1, -1, 1, 1).repeat(c.n, 1, c.ho, c.wo)
        hits = 0
        for ky in range(c.k):
            for kx in range(c.k):
                oy, ox = iy - ky + c.cpad, ix - kx + c.cpad
                if 0 <= oy < c.ho and 0 <= ox < c.wo:
                    pre[img, :, oy, ox] += wd[:, ch, ky, kx]
                    hits += 1
        assert hits >= (1 if c.k == 1 else 4)
        post = pre.clamp(min=0) if c.epi == 'relu' else pre
        fy, ty, yv = K.new_y()
        want = K.expected(fy, ty, post[:, :c.yc])
        K.launch(yv)
        K.tx[img, c.xpad + iy, c.xpad + ix, ch] = 0.0
        assert_frame(fy, want, ty, '%s %s, impulse in x at (image %d, row %d, column %d, channel %d)' % (c.name, dtn, img, iy, ix, ch))
    assert float(K.fx.float().abs().sum()) == 0


# ------------------------------------------------------------------------------------------------ pooled second destination
def pool_reference(post):
    """2x2 / stride 2 max of the (post-ReLU) map and its arg-max nibbles: bits 0..1 = window position of the FIRST maximum in
    (0,0), (0,1), (1,0), (1,1) order, bit 2 = maximum > 0; bytes [n][h/2][w/2][c/2], even channel in the low nibble."""
    n, c, h, w = post.shape
    win = post.view(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)
    mx = win.max(-1).values
    pos = torch.full(mx.shape, 3, dtype=torch.int64)
    for j in (2, 1, 0):
        pos = torch.where(win[..., j] == mx, torch.full_like(pos, j), pos)
    ties = int(((win == mx.unsqueeze(-1)).sum(-1) > 1)[mx > 0].sum())
    nib = (pos | ((mx > 0).long() << 2)).permute(0, 2, 3, 1)          # [n][h/2][w/2][c]
    packed = (nib[..., 0::2] | (nib[..., 1::2] << 4)).to(torch.uint8).contiguous()
    return mx, packed, ties


@pytest.mark.parametrize('run', [(c, d) for c in POOL_CASES for d in ('bf16', 'f16')], ids=_ids)
def test_pooled_second_destination_of_the_8phase_kernels_is_exact(run):
    """dbx_conv_forward_pool_idx / dbx_conv_forward_pool on the p8 and p8w kernels: the full map, the pooled map and the nibbles against
    the reference (the max of exact integers is exact); post-ReLU integer maps are full of tied windows, and the count of ties between
    positive maxima is asserted.  The index planes start as 0xFF bytes."""
    c, dtn = run
    x, w, bias, gate, ref = reference(c, dtn)
    mx, nibbles, ties = pool_reference(ref.post)
    assert ties > 1000 and int((mx == 0).sum()) > 1000
    K = Launcher(c, dtn, x, w, bias, gate)
    L, tag = K.L, '%s %s' % (c.name, dtn)
    d = ConvDesc(_lib.DTYPE_ID[dtn], 3, 3, 1, c.ci, c.co, EPI['relu'], SEED)

    def pooled():
        return make_frame(c.n, c.h // 2, c.w // 2, c.co, 1, K.tdt, fill=FILL, halo=HALO)
    nb = L.dbx_maxpool_idx_bytes(c.n, c.h, c.w, c.co)
    assert nb == nibbles.numel()
    fy, ty, yv = K.new_y()
    assert L.dbx_conv_pool_fusable(C.byref(d), C.byref(K.xv), C.byref(yv)) == 1
    want_y = K.expected(fy, ty, ref.post)
    fp, tp, pv = pooled()
    want_p = fp.clone()
    off = (tp.data_ptr() - fp.data_ptr()) // fp.element_size()
    want_p[off:off + tp.numel()].view(tp.shape)[:, 1:-1, 1:-1] = mx.permute(0, 2, 3, 1).to(K.tdt).cuda()
    idx = torch.full((nb + 64,), 255, dtype=torch.uint8, device='cuda')
    check(L.dbx_conv_forward_pool_idx(C.byref(d), C.byref(K.xv), ptr(K.wp), ptr(K.bias), C.byref(yv), C.byref(pv), 1, ptr(idx), stream_ptr()))
    assert_frame(fy, want_y, ty, tag + ', full map')
    assert_frame(fp, want_p, tp, tag + ', pooled map')
    got = idx[:nb].cpu().view(nibbles.shape)
    assert torch.equal(got, nibbles), '%s: %d nibble bytes differ' % (tag, int((got != nibbles).sum()))
    assert bool((idx[nb:] == 255).all())
    # the pooled map alone, without nibbles: the full map stays as it was
    fy2, ty2, yv2 = K.new_y()
    fy2_0 = fy2.clone()
    fp2, tp2, pv2 = pooled()
    check(L.dbx_conv_forward_pool(C.byref(d), C.byref(K.xv), ptr(K.wp), ptr(K.bias), C.byref(yv2), C.byref(pv2), 0, stream_ptr()))
    assert_frame(fp2, want_p, tp2, tag + ', pooled map alone')
    assert torch.equal(bits(fy2), bits(fy2_0))
    K.assert_inputs_unchanged()


# ------------------------------------------------------------------------------------------------ split destination
@pytest.mark.parametrize('dtn', ['bf16', 'f16'])
def test_split_destination_on_the_lds_ring_kernel_is_exact(dtn):
    """dbx_conv_forward_split, 1x1 192 -> 256 + 256: couts [0, 256) plain into an un-framed y, couts [256, 512) ReLU-gated into a framed
    y2.  192 input channels are no multiple of 128, so it is the LDS-ring kernel's 256 x 256 tiles over both destinations."""
    L, tdt, dt = _lib.lib(), TDT[dtn], _lib.DTYPE_ID[dtn]
    n, h, w, ci, c1, c2 = 2, 21, 27, 192, 256, 256
    x, wt, bias, gate = R.int_operands(77, n, ci, c1 + c2, ci, 1, h, w, 0.25, h, w, c2)
    ref = R.conv_ref(x, wt, bias, 1, 0, 0)
    R.assert_exact_premise(ref, dtn)
    y1, y2 = ref.pre[:, :c1], ref.pre[:, c1:] * (gate > 0)
    fx, tx, xv = make_frame(n, h, w, ci, 1, tdt, data=x)
    fg, tg, gv = make_frame(n, h, w, c2, 2, tdt, data=gate)
    fx0, fg0 = fx.clone(), fg.clone()
    d = ConvDesc(dt, 1, 1, 0, ci, c1 + c2, 0)
    wp = torch.zeros(L.dbx_conv_packed_elems(C.byref(d)) * 2, dtype=torch.uint8, device='cuda')
    wf = wt.float().cuda()
    check(L.dbx_pack_weight(dt, 0, ptr(wf), c1 + c2, ci, 1, 1, ptr(wp), c1 + c2, ci, 0, 0, stream_ptr()))
    outs = []
    for _ in range(2):
        fa, ta, av = make_frame(n, h, w, c1, 0, tdt, fill=FILL, halo=HALO)
        fb, tb, bv = make_frame(n, h, w, c2, 1, tdt, fill=FILL, halo=HALO)
        wa, wb = fa.clone(), fb.clone()
        wa[(ta.data_ptr() - fa.data_ptr()) // 2:][:ta.numel()].view(ta.shape)[...] = y1.permute(0, 2, 3, 1).to(tdt).cuda()
        wb[(tb.data_ptr() - fb.data_ptr()) // 2:][:tb.numel()].view(tb.shape)[:, 1:-1, 1:-1] = y2.permute(0, 2, 3, 1).to(tdt).cuda()
        check(L.dbx_conv_forward_split(C.byref(d), C.byref(xv), ptr(wp), None, C.byref(av), None, C.byref(bv), C.byref(gv), c1, GATE, stream_ptr()))
        assert_frame(fa, wa, ta, 'split %s, first destination' % dtn)
        assert_frame(fb, wb, tb, 'split %s, gated second destination' % dtn)
        outs.append((fa, fb))
    assert torch.equal(bits(outs[0][0]), bits(outs[1][0])) and torch.equal(bits(outs[0][1]), bits(outs[1][1]))
    assert torch.equal(bits(fx), bits(fx0)) and torch.equal(bits(fg), bits(fg0))
