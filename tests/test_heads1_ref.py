"""tests/heads1_ref.py checked on the CPU: the reference against torch float64 autograd through the literal module structure, the premise
helpers against cases built to violate each clause, the sensitivity of the reference to the faults the GPU file is there to catch, the
plan restatements at 256 and 304 CUs for every case of the tables, the impulse pixel lists, and the domain on which the float32 row
recovery of genhid_pixel (csrc/common.hpp: a helper no kernel calls) is exact."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads_ref as H                                   # noqa: E402
import heads1_ref as R                                  # noqa: E402


def test_keep_bits_is_drop_keep():
    for seed, M, co in ((R.SEED, 777, 2048), (0x1234, 100, 512), (0xFFFFFFFF, 33, 1024)):
        assert np.array_equal(R.keep_bits(seed, M, co), H.drop_keep(seed, M, co))


# ---------------------------------------------------------------------------------------------------------------- autograd
def small_problem(seed=3, n=2, h=3, w=5, ks=(1, 4, 3)):
    rng = np.random.RandomState(seed)
    P, nh = n * h * w, len(ks)
    z = rng.randint(-2, 3, size=(P, 768)).astype(np.float64)
    w1 = rng.randint(-2, 3, size=(nh, 512, 768)).astype(np.float64)
    b1 = rng.randint(-3, 4, size=512 * nh).astype(np.float64)
    w2 = [rng.randint(-2, 3, size=(k, 512)).astype(np.float64) for k in ks]
    b2 = rng.randint(-3, 4, size=sum(ks)).astype(np.float64)
    d_out = np.zeros((P, nh, 8))
    for hd, k in enumerate(ks):
        d_out[:, hd, :k] = rng.randint(-2, 3, size=(P, k))
    return dict(n=n, h=h, w=w, ks=ks, P=P, nh=nh, z=z, w1=w1, b1=b1, w2=w2, b2=b2, d_out=d_out, keep=H.drop_keep(77, P, 512 * nh))


def test_reference_equals_autograd_through_the_module_structure():
    """Conv1x1(768 -> 512) -> mask * 2 -> Conv1x1(512 -> k) per head -> concat, behind the ReLU whose output is the fusion map: the forward
    outputs, dW1 / db1 and the ReLU-gated d_x of the channels [512, 768), all exact on integers in float64."""
    p = small_problem()
    n, h, w, ks, P, nh = p['n'], p['h'], p['w'], p['ks'], p['P'], p['nh']

    def nchw(a):
        return torch.from_numpy(np.ascontiguousarray(a.reshape(n, h, w, -1).transpose(0, 3, 1, 2)))
    z = nchw(p['z']).requires_grad_(True)
    fusion = torch.relu(z)
    outs, conv1 = [], []
    for hd, k in enumerate(ks):
        c1 = torch.nn.Conv2d(768, 512, 1).double()
        c2 = torch.nn.Conv2d(512, k, 1).double()
        with torch.no_grad():
            c1.weight.copy_(torch.from_numpy(p['w1'][hd]).view(512, 768, 1, 1))
            c1.bias.copy_(torch.from_numpy(p['b1'][512 * hd:512 * (hd + 1)]))
            c2.weight.copy_(torch.from_numpy(p['w2'][hd]).view(k, 512, 1, 1))
            c2.bias.copy_(torch.from_numpy(p['b2'][sum(ks[:hd]):sum(ks[:hd + 1])]))
        mask = nchw(p['keep'][:, 512 * hd:512 * (hd + 1)].astype(np.float64))
        outs.append(c2(c1(fusion) * mask * 2))
        conv1.append(c1)
    out = torch.cat(outs, 1)
    g = torch.cat([nchw(p['d_out'][:, hd, :k]) for hd, k in enumerate(ks)], 1)
    (out * g).sum().backward()
    x = np.maximum(p['z'], 0)
    # forward
    pre, absum = R.fwd_pre(x, p['w1'].reshape(512 * nh, 768), p['b1'])
    assert absum >= float((np.abs(x) @ np.abs(p['w1'].reshape(512 * nh, 768)).T + np.abs(p['b1'])).max())       # the row-sum bound IS a bound
    hid, exact, ref_out, _ = R.fwd_ref(pre, p['keep'], p['w2'], p['b2'], ks, 'f32')
    assert np.array_equal(hid, exact)
    want = out.detach().numpy().transpose(0, 2, 3, 1).reshape(P, -1)
    assert np.array_equal(np.concatenate(ref_out, axis=1), want) and np.abs(want).max() > 0
    # backward: the slice [512, 768) of the fusion map, as the engine calls the two generators
    wg = R.wgrad_ref(p['d_out'], p['w2'], p['keep'], 2, x[:, 512:], 'f32')
    for hd in range(nh):
        assert np.array_equal(wg.dw[512 * hd:512 * (hd + 1)], conv1[hd].weight.grad.numpy()[:, 512:, 0, 0])
        assert np.array_equal(wg.db[512 * hd:512 * (hd + 1)], conv1[hd].bias.grad.numpy())
    w1t = np.ascontiguousarray(p['w1'][:, :, 512:].reshape(512 * nh, 256))
    dg = R.dgrad_ref(p['d_out'], p['w2'], p['keep'], 2, w1t, x[:, 512:], 'f32', chunk=7)
    zg = z.grad.numpy().transpose(0, 2, 3, 1).reshape(P, 768)[:, 512:]
    assert np.array_equal(dg.d_x, zg) and np.abs(zg).max() > 0 and (zg == 0).mean() > 0.3
    assert dg.absum >= float((np.abs(wg.d_hid) @ np.abs(w1t)).max())


def test_reference_without_dropout_has_scale_one():
    p = small_problem(seed=4, ks=(2,))
    a = R.dhid_exact(p['d_out'], p['w2'], None, 1)
    assert np.array_equal(a, p['d_out'][:, 0, :2] @ p['w2'][0])


# ---------------------------------------------------------------------------------------------------------------- premise helpers
def test_premise_helpers_reject_what_violates_them():
    R.assert_integers(np.array([1.0, -3.0]))
    with pytest.raises(AssertionError, match='premise \\(a\\)'):
        R.assert_integers(np.array([1.0, 0.5]))
    R.assert_sum_premise(2 ** 24 - 1, 'x')
    with pytest.raises(AssertionError, match='premise \\(a\\)'):
        R.assert_sum_premise(2 ** 24, 'x')
    R.assert_representable(np.array([256.0, 258.0, -0.5]), 'bf16', 'x')
    with pytest.raises(AssertionError, match='premise \\(b\\)'):
        R.assert_representable(np.array([256.0, 257.0]), 'bf16', 'x')
    R.assert_representable(np.array([2047.0, 2050.0]), 'f16', 'x')
    with pytest.raises(AssertionError, match='premise \\(b\\)'):
        R.assert_representable(np.array([2049.0]), 'f16', 'x')
    ties = np.arange(257.0, 257.0 + 64, 2)                 # odd integers above 256: exact ties in bf16
    assert R.rounding_stats(ties, 'bf16') == (1.0, 32)
    R.assert_rounding_premise(ties, 'bf16', 'x')
    with pytest.raises(AssertionError, match='premise \\(c\\)'):
        R.assert_rounding_premise(np.concatenate([ties[:4], np.zeros(100)]), 'bf16', 'x')          # 4 % need rounding
    with pytest.raises(AssertionError, match='premise \\(c\\)'):
        R.assert_rounding_premise(np.arange(256.25, 300, 2), 'bf16', 'x')                         # all need rounding, none is a tie
    # a tie rounds to even, once
    assert H.round_np(np.array([257.0, 259.0]), 'bf16').tolist() == [256.0, 260.0]


def test_rounding_contents_meet_their_premise_on_the_reference_alone():
    f = R.FWD['f-nh4']
    m = R.make_fwd(f, 'rounding')
    R.assert_sum_premise(m['absum'], 'hid')
    for dtn in R.DTN16:
        hid, exact, out, absum = R.fwd_ref(m['pre'], m['keep'], m['w2'], m['b2'], f.ks, dtn)
        R.assert_rounding_premise(exact, dtn, 'hid')
        R.assert_sum_premise(absum, 'out')
    for drop in ('none', 'hash'):
        mw = R.make_wg(R.WG['b-min'], drop, 'rounding')
        md = R.make_dg(R.dg_cases(256)['c-256'], drop, 'rounding')
        for dtn in R.DTN16:
            r = R.wg_reference(mw, dtn)
            R.assert_rounding_premise(r.exact, dtn, 'd_hid')
            R.assert_sum_premise(max(r.absw, r.absb), 'dW1')
            d = R.dg_reference(md, dtn)
            R.assert_rounding_premise(d.exact, dtn, 'd_x')
            R.assert_sum_premise(d.absum, 'd_x')


# ---------------------------------------------------------------------------------------------------------------- sensitivity
def test_reference_is_sensitive_to_the_faults_the_gpu_tests_are_there_for():
    p = small_problem(seed=5)
    P, nh, ks = p['P'], p['nh'], p['ks']
    x = np.maximum(p['z'], 0)
    w1t = np.ascontiguousarray(p['w1'][:, :, 512:].reshape(512 * nh, 256))
    gate = np.ones((P, 256))

    def both(d_out, keep):
        wg = R.wgrad_ref(d_out, p['w2'], keep, 2, x[:, 512:], 'f32')
        return wg, R.dgrad_ref(d_out, p['w2'], keep, 2, w1t, gate, 'f32')
    wg0, dg0 = both(p['d_out'], p['keep'])
    # one removed (pixel, hidden channel) term
    pix, ch = np.argwhere((wg0.d_hid != 0) & (np.abs(x[:, 512:]).sum(axis=1) > 0)[:, None])[0]
    keep = p['keep'].copy()
    keep[pix, ch] = False
    wg1, dg1 = both(p['d_out'], keep)
    assert (wg1.dw[ch] != wg0.dw[ch]).any() and wg1.db[ch] != wg0.db[ch] and (dg1.d_x[pix] != dg0.d_x[pix]).any()
    assert np.array_equal(np.delete(wg1.dw, ch, axis=0), np.delete(wg0.dw, ch, axis=0)) and np.array_equal(np.delete(dg1.d_x, pix, axis=0), np.delete(dg0.d_x, pix, axis=0))
    pre, _ = R.fwd_pre(x, p['w1'].reshape(512 * nh, 768), p['b1'])
    o0 = R.fwd_ref(pre, p['keep'], p['w2'], p['b2'], ks, 'f32')[2]
    o1 = R.fwd_ref(pre, keep, p['w2'], p['b2'], ks, 'f32')[2]
    assert any((a[pix] != b[pix]).any() for a, b in zip(o0, o1))
    # a d_out slot taken from the neighbouring head, at one pixel
    d_out = p['d_out'].copy()
    d_out[pix, 1, :] = 0
    d_out[pix, 1, :ks[1]] = p['d_out'][pix, 2, :ks[1]] + 1
    wg2, dg2 = both(d_out, p['keep'])
    assert (wg2.d_hid[pix] != wg0.d_hid[pix]).any() and (wg2.dw != wg0.dw).any() and (dg2.d_x[pix] != dg0.d_x[pix]).any()
    # keep bits taken from the neighbouring pixel
    wg3, dg3 = both(p['d_out'], np.roll(p['keep'], 1, axis=0))
    assert (wg3.dw != wg0.dw).any() and (wg3.db != wg0.db).any() and (dg3.d_x != dg0.d_x).any()
    # scale 1 under hash, a W2 that is not rounded to T
    assert (R.dhid_exact(p['d_out'], p['w2'], p['keep'], 1) != wg0.exact).any()
    raw = [np.where(a == 1, H.UNREP['bf16'], a) for a in p['w2']]
    assert (H.round_np(R.dhid_exact(p['d_out'], raw, p['keep'], 2), 'bf16') != wg0.exact).any()


# ---------------------------------------------------------------------------------------------------------------- plans
def test_forward_plan_restated_at_256_and_304_cus():
    for name, case in R.FWD.items():
        p = R.fwd_plan(case, 256)
        s = p['p8']
        assert (s['mt'], s['base'], s['extra'], s['rounded'], s['items'], s['last'], p['ws_items']) == R.FWD_AT_256[name], (name, p)
        assert p['kinds'] == [2, 1] and p['fusable'] == 2 and p['shape_ok'], (name, p)       # each shape qualifies for both kernels at 256 CUs
        q = R.fwd_plan(case, 304)
        # 192 .. 198 items are fewer than three quarters of 304 CUs: only the ws kernel takes the first four; the round-up case keeps both
        assert q['kinds'] == ([2, 1] if name == 'f-roundup' else [1]) and q['ws_items'] == p['ws_items'], (name, q)
    assert R.fwd_plan(R.FWD['f-roundup'], 304)['p8']['items'] == 452 and not R.fwd_plan(R.FWD['f-roundup'], 304)['p8']['rounded']
    assert not R.fwd_plan(R.FWD['f-nh4']._replace(ks=(1, 9)), 256)['shape_ok'] and R.fwd_plan(R.FWD['f-nh4']._replace(h=3), 256)['kinds'] == []


def test_wgrad_plan_restated_at_256_and_304_cus():
    for cus in (256, 304):
        for name, case in R.WG.items():
            p = R.wgrad_plan_ref(case, cus)
            assert (p['spi'], p['steps_total'], p['splits'], p['steps_per_split']) == R.WG_AT_256[name], (cus, name, p)   # (too few steps for the CU count to matter)
            assert p['ok'] and p['grid'] == 2 * len(case.ks) * p['splits']
    p = R.wgrad_plan_ref(R.WG['b-empty-split'], 256)
    assert p['empty'] == 1 and p['short'] == 4 and 14 * 9 < 130 <= 15 * 9
    p = R.wgrad_plan_ref(R.WG['b-ragged-seam'], 256)
    assert p['short'] == 9 and (11 * 37) % 32 != 0 and [s * 10 // 13 for s in range(4)] == [0, 0, 1, 2]      # splits 1 and 2 start inside images 0 and 1 ...
    assert [(min(s * 10 + 10, 39) - 1) // 13 for s in range(4)] == [0, 1, 2, 2]                                # ... and end in the next one
    assert not R.wgrad_plan_ref(R.WG['b-min']._replace(w=29), 256)['ok']
    # a problem large enough for the CU count to set the splits: 64 images -> 832 steps, 8 tiles
    big = R.WG['b-ragged-seam']._replace(n=64)
    assert R.wgrad_plan_ref(big, 256)['splits'] == 32 and R.wgrad_plan_ref(big, 304)['splits'] == 32 and R.wgrad_plan_ref(big._replace(ks=(8,)), 304)['splits'] == 104


def test_dgrad_plan_restated_at_256_and_304_cus():
    for cus in (256, 304):
        cases = R.dg_cases(cus)
        two, three = cases['c-two-tiles'], cases['c-three-tiles']
        p2 = R.dgrad_plan_ref(two.n * two.h * two.w, cus)
        p3 = R.dgrad_plan_ref(three.n * three.h * three.w, cus)
        assert cus < p2['ntiles'] < 2 * cus and (p2['most'], p2['least'], p2['grid']) == (2, 1, cus) and (two.n * two.h * two.w) % 256
        assert 2 * cus < p3['ntiles'] < 3 * cus and (p3['most'], p3['least'], p3['grid']) == (3, 2, cus) and (three.n * three.h * three.w) % 256
        assert p2['with_most'] == p2['ntiles'] - cus and p3['with_most'] == p3['ntiles'] - 2 * cus
        for name in R.DG_SMALL:
            c = cases[name]
            p = R.dgrad_plan_ref(c.n * c.h * c.w, cus)
            assert p['most'] == 1 and p['grid'] == p['ntiles']
    c = R.dg_cases(256)
    assert (c['c-two-tiles'].n, R.dgrad_plan_ref(7 * 97 * 113, 256)['ntiles'], R.dgrad_plan_ref(7 * 97 * 113, 256)['with_most']) == (7, 300, 44)
    assert c['c-three-tiles'].n == 14 and len(c['c-three-tiles'].ks) == 1
    assert (c['c-partial'].n * c['c-partial'].h * c['c-partial'].w, c['c-256'].h * c['c-256'].w, (c['c-513'].h * c['c-513'].w) % 256) == (99, 256, 1)


def test_impulse_pixel_lists_hold_the_places_the_issue_names():
    for cus in (256, 304):
        for case in R.FWD.values():
            n, h, w = case.n, case.h, case.w
            px, hw, wp = set(R.fwd_impulse_pixels(case, cus)), h * w, w + 2
            assert {0, w - 1, hw - w, hw - 1, (n - 1) * hw, n * hw - 1} <= px and all({i * hw - 1, i * hw} <= px for i in range(1, n))
            assert {(h // 2) * w + w - 1, (h // 2 + 1) * w} <= px
            row, col = 128 // wp, 128 % wp                  # the first ws tile boundary: frame position 128 of image 0
            assert 1 <= col <= w and {row * w + col - 2, row * w + col - 1} <= px
            s = R.sched8(n * hw, 2 * len(case.ks), cus)
            assert {32 * (s['base'] + 1) - 1, 32 * (s['base'] + 1), 32 * s['base'] - 1, 32 * s['base']} <= px
        for case in R.WG.values():
            n, h, w, pad = case.n, case.h, case.w, case.pad
            px, hw, wp = set(R.wg_impulse_pixels(case, cus)), h * w, w + 2 * pad
            assert {0, hw - 1, (n - 1) * hw, n * hw - 1} <= px and all({i * hw - 1, i * hw} <= px for i in range(1, n))
            pl = R.wgrad_plan_ref(case, cus)
            q = 32                                          # the first step boundary, counted over the valid rows from their first halo column
            near = R.frame_neighbours(n, h, w, pad, [(0, q)])
            assert len(near) == 2 and set(near) <= px
            for sp in range(1, pl['splits']):
                g = sp * pl['steps_per_split']
                if g < pl['steps_total'] and g % pl['spi']:
                    assert set(R.frame_neighbours(n, h, w, pad, [(g // pl['spi'], 32 * (g % pl['spi']))])) <= px
        for case in R.dg_cases(cus).values():
            P = case.n * case.h * case.w
            px = set(R.dg_impulse_pixels(case, cus))
            assert {0, P - 1} <= px and (P <= 256 or {255, 256} <= px)
            if P > 256 * cus:
                assert {256 * cus - 1, 256 * cus} <= px
    assert R.frame_neighbours(1, 3, 4, 1, [(0, 6)]) == [3, 4] and R.frame_neighbours(1, 3, 4, 1, [(0, 8)]) == [4, 5]


def test_fragment_order_index_follows_the_header():
    """include/densebox_hip.h, dbx_pack_weight modes 4 / 5, 1x1: [row / BN][k / 128][(k % 128) / 16][(row % BN) / 32][32 ((k % 16) / 8) + row % 32][k % 8]."""
    assert int(R.frag_index_1x1(33, 9, 128, 256)) == ((0 * 8 + 0) * 8 + 1) * 512 + (32 + 1) * 8 + 1 == 777
    assert int(R.frag_index_1x1(300, 150, 256, 512)) == ((((1 * 2 + 1) * 8 + 1) * 8 + 1) * 64 + 12) * 8 + 6
    m = np.arange(256 * 1024, dtype=np.float64).reshape(256, 1024)
    img = R.frag_image_1x1(m)
    assert img[int(R.frag_index_1x1(7, 1000, 1024, 256))] == m[7, 1000] and sorted(img.tolist()) == m.ravel().tolist()


# ---------------------------------------------------------------------------------------------------------------- row recovery
def test_float_row_recovery_of_the_unused_helper_is_exact_below_2_to_22_positions():
    """genhid_pixel's fy = (int)((q + 0.5f) * inv_wp), inv_wp = 1.f / wp, emulated in NumPy float32, for every frame width 32 .. 4100 and
    every position q below 2**22.  NO kernel calls genhid_pixel (the weight-gradient generator divides in integers once per workgroup
    and walks incrementally), so no DBX_REQUIRE follows from this: the sweep documents the helper's domain, which its comment in
    csrc/common.hpp quotes.  The per-image frame sizes dbx_heads1_wgrad_gen admits reach 2**24 positions and more (fewer than 2**24
    pixels plus the halo): the helper is NOT exact on all of them -- the first wrong position is 4 201 469 (wp 4095), asserted below.
    Every float operation of the expression is monotone in q, so fy is a non-decreasing step function of q: it equals q / wp everywhere
    iff it is r at q = r wp and at most r - 1 at r wp - 1 for every row r -- two evaluations per row cover every q."""
    for wp in range(32, 4101):
        r = np.arange(0, 2 ** 22 // wp + 2, dtype=np.int64)
        assert np.array_equal(R.row_recovery_f32(r * wp, wp), r), wp
        assert np.array_equal(R.row_recovery_f32(r[1:] * wp - 1, wp), r[1:] - 1), wp
    # dense over a few widths, as a check of the monotonicity argument itself
    for wp in (32, 33, 61, 62, 4095, 4100):
        q = np.arange(0, 2 ** 20, dtype=np.int64)
        assert np.array_equal(R.row_recovery_f32(q, wp), q // wp), wp
    assert 4201469 > 2 ** 22 and int(R.row_recovery_f32(np.array([4201469]), 4095)[0]) != 4201469 // 4095
