"""tests/heads_ref.py (the float64 reference the stage-2 heads backward is pinned with, tests/test_hip_head2_paths.py) checked on the CPU:
against plain loops written from the formulas, against torch's own up-sampling and casts, its premises for every case of the table,
its sensitivity to the errors a kernel can make (a term missing at the last pixel or behind an image seam, the keep bits of the
neighbouring pixel, exchanged interpolation weights, a half-row ownership boundary off by one), the dropout hash against a scalar
restatement at the parameters the p8-heads conv case pins, and the launch plans: the restatement of h2u_plan against the figures of
the case table and against the library's own read-only query dbx_head2_backward_up_plan (host code: no GPU).

Interval-compared outputs (premise (d), up-workload: 3 686 400 d_g44 outputs, printed by test_premise_holds_for_every_case): the
interval [round_T(ref - E), round_T(ref + E)] holds more than one value at 0.21 % (no dropout), 0.09 % (hash) and 0.09 % (mask) of
them in bf16 -- about 7600, 3300 and 3300 outputs -- and at 0.57 %, 0.27 % and 0.27 % in f16 (21 000, 9800, 9800); the no-store forms:
0.09 % and 0.27 %.  Asserted below 1 %; an output sums at most 16 terms (asserted)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads_ref as R                                   # noqa: E402

TDT = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}
UP_CASES = [c for c in R.CASES.values() if c.hs is not None]


# ---------------------------------------------------------------------------------------------------------------- building blocks
@pytest.mark.parametrize('dtn', ['bf16', 'f16', 'f32'])
def test_round_np_is_torchs_cast(dtn):
    rng = np.random.RandomState(1)
    x = np.concatenate([rng.standard_normal(20000) * 10.0 ** rng.randint(-9, 5, 20000), np.arange(-600, 600) / 4.0,
                        [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -9, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -12, 2.0 ** -25, 3 * 2.0 ** -25,
                         2.0 ** -24, 2.0 ** -15 + 2.0 ** -25, 0.0, 65504.0]]).astype(np.float32).astype(np.float64)   # float32 values: torch rounds once
    want = torch.from_numpy(x).float().to(TDT[dtn]).double().numpy()
    assert np.array_equal(R.round_np(x, dtn), want)
    # the two entries the no-store cases plant in W2: 1 + 2**-9 is an f16 number, 1 + 2**-12 is not; bf16 holds neither
    assert R.round_np(R.UNREP['bf16'], 'bf16') == 1.0 and R.round_np(R.UNREP['f16'], 'f16') == 1.0
    assert R.round_np(1 + 2.0 ** -9, 'f16') == 1 + 2.0 ** -9


def _hash32_scalar(seed, m, c32):
    """dbx_drop_hash32 (csrc/common.hpp) one value at a time on Python integers."""
    M = 0xFFFFFFFF
    x = (seed ^ ((m * 0x9E3779B1) & M) ^ ((c32 * 0x85EBCA77) & M)) & M
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M
    x ^= x >> 15
    x = (x * 0x846CA68B) & M
    x ^= x >> 16
    return x


def test_drop_keep_is_the_hash_the_p8_heads_conv_case_pins():
    """tests/test_hip_conv_paths.py compares the forward epilogue (DBX_EPI_DROPHASH) with drop_keep(0x1234, 2 x 101 x 121, 512): the very
    function the reference here takes its keep bits from.  A scalar restatement agrees with it at those parameters and at this
    file's seed; dbx_drop_bits4 (what the separate kernels read: four bits per call) selects the same bits."""
    for seed, M, co in ((0x1234, 2 * 101 * 121, 512), (R.SEED, 2 * 17 * 33, 2048)):
        keep = R.drop_keep(seed, M, co)
        assert keep.shape == (M, co) and 0.49 < keep.mean() < 0.51
        for m in (0, 1, 2, 31, 32, M // 2, M - 2, M - 1):
            for ch in (0, 1, 31, 32, 33, 255, 256, co - 33, co - 1):
                x = _hash32_scalar(seed, m, ch // 32)
                assert bool(keep[m, ch]) == bool(x >> (ch % 32) & 1)
                c4 = ch // 4
                bits4 = (_hash32_scalar(seed, m, c4 >> 3) >> ((c4 & 7) * 4)) & 15
                assert bool(keep[m, ch]) == bool(bits4 >> (ch % 4) & 1)


@pytest.mark.parametrize('sizes', [(9, 5), (17, 9), (33, 17), (65, 33), (60, 30), (3, 2), (5, 3), (171, 86)])
def test_coefficients_are_atens(sizes):
    """up_matrix is the matrix of F.interpolate(bilinear, align_corners=True) (float64 there, float32 coefficients here), its rows sum
    to one, and the float32 arithmetic is the documented one: on dyadic sizes every coefficient is exactly 0, 1/2 or 1."""
    out, inn = sizes
    U = R.up_matrix(out, inn)
    eye = torch.eye(inn, dtype=torch.float64).view(inn, 1, inn, 1)              # one image per source row, a 1-wide column
    want = F.interpolate(eye, size=(out, 1), mode='bilinear', align_corners=True).view(inn, out).t().numpy()
    tol = inn * 2.0 ** -22                                  # scale and src are rounded to float32: two half-ulps of a number below `inn`
    assert np.abs(U - want).max() < tol and np.abs(U.sum(axis=1) - 1).max() < 1e-6
    i0, i1, l0, l1 = R.bilin_coef(out, inn)
    assert l0.dtype == np.float32 and l1.dtype == np.float32 and (l1 >= 0).all() and (l0 >= 0).all() and i1.max() == inn - 1
    if (inn - 1) * 2 == out - 1:
        assert set(np.unique(U).tolist()) <= {0.0, 0.5, 1.0}
        assert np.array_equal(i0, np.minimum(np.arange(out) // 2, inn - 1))


def test_up_transposed_is_the_gradient_of_the_up_sampling():
    rng = np.random.RandomState(2)
    n, h, w, hs, ws, C = 2, 9, 17, 5, 9, 3
    d = rng.randint(-64, 65, size=(n, h, w, C)).astype(np.float64)
    g, ga = R.up_transposed(d, hs, ws)
    x = torch.zeros(n, C, hs, ws, dtype=torch.float64, requires_grad=True)
    F.interpolate(x, size=(h, w), mode='bilinear', align_corners=True).backward(torch.from_numpy(d).permute(0, 3, 1, 2))
    assert np.abs(g - x.grad.permute(0, 2, 3, 1).numpy()).max() < 1e-9 and g.shape == (n, hs, ws, C)
    # ... and the loop over destination pixels, term by term
    Uy, Ux = R.up_matrix(h, hs), R.up_matrix(w, ws)
    loop, loop_abs = np.zeros_like(g), np.zeros_like(g)
    for oy in range(h):
        for ox in range(w):
            for iy in np.nonzero(Uy[oy])[0]:
                for ix in np.nonzero(Ux[ox])[0]:
                    loop[:, iy, ix] += Uy[oy, iy] * Ux[ox, ix] * d[:, oy, ox]
                    loop_abs[:, iy, ix] += Uy[oy, iy] * Ux[ox, ix] * np.abs(d[:, oy, ox])
    assert np.array_equal(loop, g) and np.array_equal(loop_abs, ga)               # dyadic: exact in any order


@pytest.mark.parametrize('drop', ['none', 'hash', 'mask'])
def test_head2_ref_equals_the_loop(drop):
    ks, P = (1, 3, 8), 23
    d_out, hid, w2, mask = R.int_operands(5, P, ks)
    keep = {'none': None, 'mask': mask, 'hash': R.drop_keep(9, P, 512 * len(ks))}[drop]
    scale = 1 if drop == 'none' else 2
    ref = R.head2_ref(d_out, hid, w2, keep, scale)
    assert set(np.unique(d_out).tolist()) == {-2, -1, 0, 1, 2} and set(np.unique(hid).tolist()) == set(range(-4, 5)) and 0.4 < (hid == 0).mean() < 0.6
    for hd, k in enumerate(ks):
        assert set(np.unique(w2[hd]).tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0} and not d_out[:, hd, k:].any()
        dw, db, dh = np.zeros((k, 512)), np.zeros(k), np.zeros((P, 512))
        for p in range(P):
            for j in range(k):
                db[j] += d_out[p, hd, j]
                dw[j] += float(d_out[p, hd, j]) * hid[p, 512 * hd:512 * (hd + 1)]
                dh[p] += float(d_out[p, hd, j]) * w2[hd][j]
            dh[p] *= scale
            if keep is not None:
                dh[p] *= keep[p, 512 * hd:512 * (hd + 1)] != 0
        assert np.array_equal(ref.dw[hd], dw) and np.array_equal(ref.db[hd], db) and np.array_equal(ref.d_hid[:, hd], dh)
        assert (ref.absw[hd] >= np.abs(dw)).all() and float(np.abs(dw).max()) > 0
    R.assert_premise(ref)


def test_premises_fire():
    d_out, hid, w2, mask = R.int_operands(5, 16, (2,))
    with pytest.raises(AssertionError, match=r'premise \(a\)'):
        R.assert_premise(R.head2_ref(d_out, hid, [w2[0] * 0.5], None, 1))
    with pytest.raises(AssertionError, match=r'premise \(a\)'):
        R.assert_premise(R.head2_ref(d_out, hid, [w2[0] * 32], None, 2))
    with pytest.raises(AssertionError, match=r'premise \(b\)'):
        R.assert_premise(R.head2_ref(d_out, hid.astype(np.float64) * 2.0 ** 20, w2, None, 2))
    with pytest.raises(AssertionError, match='contract'):
        R.head2_ref(np.ones((16, 1, 8)), hid, w2, None, 1)
    ref = R.head2_ref(d_out, hid, w2, None, 2)
    g, ga = R.up_transposed(ref.d_hid.reshape(1, 4, 4, 512), 3, 3)              # 3 -> 4: coefficients in thirds
    with pytest.raises(AssertionError, match=r'premise \(c\)'):
        R.assert_premise(ref, g, ga, True, (1, 4, 4, 3, 3))


# ---------------------------------------------------------------------------------------------------------------- the case table
@pytest.mark.parametrize('drop', ['none', 'hash', 'mask'])
@pytest.mark.parametrize('case', list(R.CASES.values()), ids=lambda c: c.name)
def test_premise_holds_for_every_case(case, drop):
    m = R.make(case, drop)
    geom = (case.n, case.h, case.w, case.hs, case.ws)
    R.assert_premise(m['ref'], m.get('g44'), m.get('g44_abs'), case.dyadic, geom)
    assert float(np.abs(m['ref'].d_hid).max()) >= 16 and all(float(np.abs(a).max()) > 0 for a in m['ref'].dw + m['ref'].db)
    if case.hs is not None:
        assert R.max_terms(case) <= 16
        assert (case.dyadic is True) == ((case.hs - 1) * 2 == case.h - 1 and (case.ws - 1) * 2 == case.w - 1)
    if case.dyadic is False:
        for dtn in ('bf16', 'f16'):
            lo, hi, share = R.interval(m['g44'], m['g44_abs'], dtn)
            print('%s %s %s: %.4f %% of %d d_g44 outputs have an interval wider than one value' % (case.name, drop, dtn, 100 * share, lo.size))
            assert share < 0.01 and (lo <= hi).all() and (R.round_np(m['g44'], dtn) >= lo).all() and (R.round_np(m['g44'], dtn) <= hi).all()


@pytest.mark.parametrize('dtn', ['bf16', 'f16'])
@pytest.mark.parametrize('name', ['up-two-halves-ring', 'up-workload'])
def test_nostore_cases_pin_the_rounding_of_w2(name, dtn):
    """d_hid->ptr == NULL rounds W2 to T: the references with the rounded and with the fp32 W2 differ, in d_hid and in d_g44; the
    rounded one keeps the integer premise (the planted entries round to 1)."""
    case = R.CASES[name]
    m = R.make(case, 'hash', w2_dtn=dtn)
    assert any((a != b).any() for a, b in zip(m['w2'], m['w2_raw'])) and all(np.array_equal(a, np.rint(a)) for a in m['w2'])
    differ = R.round_np(m['ref'].d_hid, dtn) != R.round_np(m['ref_raw'].d_hid, dtn)
    assert differ.mean() > 0.001
    graw, _ = R.up_transposed(R.round_np(m['ref_raw'].d_hid, dtn).reshape(case.n, case.h, case.w, -1), case.hs, case.ws)
    assert (R.round_np(graw, dtn) != R.round_np(m['g44'], dtn)).mean() > 0.001
    if not case.dyadic:
        share = R.interval(m['g44'], m['g44_abs'], dtn)[2]
        print('%s no-store %s: %.4f %% wide intervals' % (name, dtn, 100 * share))
        assert share < 0.01
    R.assert_premise(m['ref'], m['g44'], m['g44_abs'], case.dyadic, (case.n, case.h, case.w, case.hs, case.ws))


# ---------------------------------------------------------------------------------------------------------------- sensitivity
def _outputs(case, ref, swap=False):
    g, _ = R.up_transposed(ref.d_hid.reshape(case.n, case.h, case.w, -1), case.hs, case.ws, swap)
    return ref, g


@pytest.mark.parametrize('drop', ['none', 'hash'])
@pytest.mark.parametrize('name', ['up-two-halves-ring', 'up-stride-2h'])
def test_reference_notices_what_a_kernel_can_get_wrong(name, drop):
    case = R.CASES[name]
    m = R.make(case, drop)
    n, h, w, nh = case.n, case.h, case.w, len(case.ks)
    ref, g = _outputs(case, m['ref'])
    # one (pixel, j) term missing: the last pixel of the last image / the first pixel of the second image (behind the first seam)
    for p in (n * h * w - 1, h * w):
        for hd, k in enumerate(case.ks):
            d2 = m['d_out'].copy()
            assert d2[p, hd, k - 1] != 0
            d2[p, hd, k - 1] = 0
            r2, g2 = _outputs(case, R.head2_ref(d2, m['hid'], m['w2'], m['keep'], m['scale']))
            assert (r2.d_hid[p, hd] != ref.d_hid[p, hd]).any() and (r2.dw[hd][k - 1] != ref.dw[hd][k - 1]).any()
            assert r2.db[hd][k - 1] != ref.db[hd][k - 1] and (g2[..., 512 * hd:512 * (hd + 1)] != g[..., 512 * hd:512 * (hd + 1)]).any()
    # the keep bits of pixel p + 1
    if m['keep'] is not None:
        r2, g2 = _outputs(case, R.head2_ref(m['d_out'], m['hid'], m['w2'], np.roll(m['keep'], -1, axis=0), m['scale']))
        assert (r2.d_hid != ref.d_hid).mean() > 0.1 and (g2 != g).mean() > 0.1
    # l0 and l1 exchanged
    _, g2 = _outputs(case, ref, swap=True)
    assert (g2 != g).mean() > 0.1
    # the ownership boundary one column to the right for the left half only: column P enters the weight-gradient sums twice;
    # for the right half only: it enters them never
    plan = R.plan_ref(case, 'bf16')
    assert plan.halves == 2
    col = np.tile(np.arange(w), n * h)
    for times in (2, 0):
        own = np.where(col == plan.half[0].own_hi, times, 1)
        r2 = R.head2_ref(m['d_out'], m['hid'], m['w2'], m['keep'], m['scale'], own_w=own)
        for hd in range(nh):
            assert (r2.dw[hd] != ref.dw[hd]).any() and (r2.db[hd] != ref.db[hd]).any()
        assert np.array_equal(r2.d_hid, ref.d_hid)


# ---------------------------------------------------------------------------------------------------------------- plans
def test_restated_plans_have_the_figures_of_the_case_table():
    P = {name: R.plan_ref(c, 'bf16') for name, c in R.CASES.items()}
    H, L = R.Half, R.Launch
    p = P['up-one-half']
    assert (p.fused, p.halves) == (1, 1) and p.half[0] == p.half[1] == H(0, 17, 0, 17, 0, 9)
    assert p.launches == [L(0, 1, 1, 2, 2), L(1, 1, 2, 2, 2), L(2, 1, 4, 2, 2), L(3, 1, 8, 2, 2)]
    p = P['up-two-halves-ring']                                 # walked columns [0, 16) and [14, 33), boundary 15; 9 source rows > the ring's 8
    assert (p.fused, p.halves) == (1, 2) and p.half == [H(0, 16, 0, 15, 0, 8), H(14, 19, 15, 33, 8, 9)] and R.CASES['up-two-halves-ring'].hs == 9
    assert p.launches == [L(0, 1, 1, 2, 4), L(1, 2, 4, 2, 4), L(3, 1, 8, 2, 4)]
    p = P['up-stride-2h']                                       # the k = 4 launch: 16 groups < 17 images; nblk 34 / 32 / 34 in one reduce
    assert p.halves == 2 and p.launches == [L(0, 1, 1, 17, 34), L(1, 2, 4, 16, 32), L(3, 1, 8, 17, 34)]
    c = R.CASES['up-stride-2h']
    assert [((c.n - g + 16 - 1) // 16) * c.h for g in range(16)] == [10] + [5] * 15      # rows per workgroup: odd against the pipeline depth 2
    p = P['up-stride-1h']
    assert (p.fused, p.halves) == (1, 1) and p.launches == [L(0, 4, 4, 16, 16)] and R.CASES['up-stride-1h'].n == 17
    p = P['up-reduce-unrolled']                                 # 64 partial blocks > 48: the reduce kernel's four-way loop runs
    assert p.halves == 2 and p.launches == [L(0, 1, 1, 32, 64), L(1, 1, 8, 32, 64)] and R.CASES['up-reduce-unrolled'].n == 33
    p = P['up-workload']                                        # 31 + 31 columns, boundary 30
    assert p.halves == 2 and p.half == [H(0, 31, 0, 30, 0, 15), H(29, 31, 30, 60, 15, 15)]
    assert p.launches == [L(0, 1, 1, 2, 4), L(1, 2, 4, 2, 4), L(3, 1, 8, 2, 4)]
    assert P['up-fallback'].fused == 0 and R.plan_ref(R.CASES['up-one-half'], 'f32').fused == 0
    for name in ('wgrad-cap-3h', 'wgrad-cap-1h'):               # 513 rows -> 512 workgroups of 6 pixels (rows are 5), 84 of them empty
        assert R.wgrad_blocks(R.CASES[name]) == (512, 6, 84) and P[name].fused == 0
    # at batch 64 the workload's k = 4 launch walks four images per workgroup
    big = R.plan_ref(R.Case('b64', 64, 60, 60, 30, 30, (1, 4, 4, 8), False), 'bf16')
    assert [l.groups for l in big.launches] == [32, 16, 32]
    # every launch of every case fits the scratch the caller sizes by rows (partial blocks + 32 bias sums each)
    for name, c in R.CASES.items():
        nh = len(c.ks)
        used = sum(l.blocks * (l.heads * 4096 + 32) for l in P[name].launches)
        assert used <= min(c.n * c.h, 512) * (nh * 4096 + 32)


def _query(case, dtn, ks=None):
    from densebox_amd import _lib
    L = _lib.lib()
    ks = list(ks or case.ks)
    nh = len(ks)
    hv = _lib.View(None, case.n, case.h, case.w, 0, 512 * nh, 0, 512 * nh)
    gv = _lib.View(None, case.n, case.hs or case.h, case.ws or case.w, 1, 512 * nh, 0, 512 * nh)
    out = _lib.Head2UpPlan()
    rc = L.dbx_head2_backward_up_plan(_lib.DTYPE_ID[dtn], C.byref(hv), C.byref(gv), (C.c_int32 * nh)(*ks), nh, C.byref(out))
    return rc, out


def plan_of(out):
    half = [R.Half(*[getattr(out.half[i], f) for f in R.Half._fields]) for i in range(2)]
    return R.Plan(out.fused, out.halves, half, [R.Launch(*[getattr(out.launch[i], f) for f in R.Launch._fields]) for i in range(out.launches)])


@pytest.mark.skipif('DBX_HEAD2_UP' in os.environ or 'DBX_HEAD2_UP_SPLIT' in os.environ, reason='this process forces a kernel selection')
@pytest.mark.parametrize('dtn', ['bf16', 'f16', 'f32'])
def test_library_plan_query_equals_the_restatement(dtn):
    from densebox_amd import _build
    _build.build(verbose=False)
    extra = [R.Case('b64', 64, 60, 60, 30, 30, (1, 4, 4, 8), False), R.Case('w64', 2, 10, 64, 9, 32, (2, 4), None),
             R.Case('w64-33', 2, 10, 64, 9, 33, (2, 4), None), R.Case('odd', 3, 23, 37, 12, 19, (8, 1, 8, 2), None),
             R.Case('down', 2, 9, 17, 9, 17, (1,), None), R.Case('one-row', 2, 1, 17, 1, 9, (1,), None)]
    for case in list(R.CASES.values()) + extra:
        rc, out = _query(case, dtn)
        assert rc == 0 and plan_of(out) == R.plan_ref(case, dtn), (case.name, plan_of(out), R.plan_ref(case, dtn))
        if case.hs is not None:
            from densebox_amd import _lib
            nh = len(case.ks)
            hv = _lib.View(None, case.n, case.h, case.w, 0, 512 * nh, 0, 512 * nh)
            gv = _lib.View(None, case.n, case.hs, case.ws, 1, 512 * nh, 0, 512 * nh)
            assert _lib.lib().dbx_head2_backward_up_fused(_lib.DTYPE_ID[dtn], C.byref(hv), C.byref(gv)) == out.fused
