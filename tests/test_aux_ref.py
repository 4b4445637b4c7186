"""tests/aux_ref.py checked from the reference alone (CPU): (a) it agrees with torch's own CPU operators; (b) the premise of every exact
case holds; (c) on every interval case few outputs admit more than one value; (d) every case is sensitive to the defects it is
there for; (e) the kernels' fixed-size tables cannot overflow inside the ranges the dispatcher gives them; (f) plan_ref equals the
library's own query on the case table and on the workload's shapes (host code: no GPU)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aux_ref as A                                     # noqa: E402

from densebox_amd import _lib                           # noqa: E402

DTNS = ('bf16', 'f16', 'f32')
CAP = {'bf16': 0.025, 'f16': 0.10}
INTERVAL_BWD = [c.name for c in A.BWD.values() if not c.exact]
INTERVAL_FWD = [c.name for c in A.FWD.values() if not c.exact]


# ---------------------------------------------------------------------------------------------------------------- (a) against torch
@pytest.mark.parametrize('hi,wi,ho,wo', [(15, 15, 30, 30), (5, 5, 12, 12), (11, 17, 23, 33), (4, 7, 9, 17), (9, 9, 5, 5), (1, 1, 4, 6), (5, 7, 1, 1)])
def test_up_sampling_matches_interpolate_and_its_autograd(hi, wi, ho, wo):
    """float32 torch on the CPU, each against the float64 reference within K 2**-24 sum |terms| + half an ulp of the result: K_FWD
    forward; backward max_terms + 3 (ATen scatters ly lx g term by term: two products and the adds into the source pixel)."""
    rng = np.random.RandomState(hi * 100 + ho)
    x = rng.standard_normal((2, hi, wi, 5))
    g = rng.standard_normal((2, ho, wo, 5))
    xt = torch.from_numpy(x.astype(np.float32)).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    yt = F.interpolate(xt, size=(ho, wo), mode='bilinear', align_corners=True)
    yt.backward(torch.from_numpy(g.astype(np.float32)).permute(0, 3, 1, 2).contiguous())
    ref, ab = A.up_forward(x.astype(np.float32).astype(np.float64), ho, wo)
    lo, hi_, _ = A.bounds(ref, ab, 'f32', A.K_FWD)
    got = yt.detach().permute(0, 2, 3, 1).double().numpy()
    assert ((got >= lo) & (got <= hi_)).all(), float(np.abs(got - ref).max())
    ref, ab = A.up_backward(g.astype(np.float32).astype(np.float64), hi, wi)
    lo, hi_, _ = A.bounds(ref, ab, 'f32', A.max_terms(ho, wo, hi, wi) + 3)
    got = xt.grad.permute(0, 2, 3, 1).double().numpy()
    assert ((got >= lo) & (got <= hi_)).all(), float(np.abs(got - ref).max())


@pytest.mark.parametrize('planes,hi,wi,ho,wo', [(2, 14, 20, 40, 52), (3, 15, 15, 31, 31), (2, 1, 1, 3, 4), (2, 5, 7, 1, 1)])
def test_the_float32_restatement_is_the_float64_value_rounded_a_few_times(planes, hi, wi, ho, wo):
    x = np.random.RandomState(planes + ho).standard_normal((planes, hi, wi)).astype(np.float32)
    got = A.up_nchw_f32(x, ho, wo).astype(np.float64)
    ref, ab = A.up_forward(x.astype(np.float64).transpose(1, 2, 0)[None], ho, wo)
    lo, hi_, _ = A.bounds(ref[0].transpose(2, 0, 1), ab[0].transpose(2, 0, 1), 'f32', 4)      # (its chain of 4 roundings: aux_ref's docstring)
    assert ((got >= lo) & (got <= hi_)).all()


@pytest.mark.parametrize('h,w', [(12, 20), (15, 9), (6, 7), (1, 1)])
def test_pooling_matches_max_pool2d_and_its_backward_with_ties_everywhere(h, w):
    x = A.halves(h * 31 + w, (2, h, w, 6))
    y, nib = A.pool_forward(x)
    ph, pw = h // 2, w // 2
    assert y.shape == (2, ph, pw, 6) and ((nib & 3) != 0).any() == (ph > 0) and int(nib.max(initial=0)) < 8
    dy = np.random.RandomState(5).randint(-2, 3, size=y.shape).astype(np.float64)
    if ph and pw:
        xt = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        yt = F.max_pool2d(xt, 2, 2)
        yt.backward(torch.from_numpy(dy).permute(0, 3, 1, 2).contiguous())
        assert np.array_equal(yt.detach().permute(0, 2, 3, 1).numpy(), y)
        assert np.array_equal(xt.grad.permute(0, 2, 3, 1).numpy(), A.pool_backward(nib, dy, h, w))
        win = x[:, :2 * ph, :2 * pw].reshape(2, ph, 2, pw, 2, 6)
        assert ((win == win.max(axis=(2, 4), keepdims=True)).sum(axis=(2, 4)) > 1).mean() > 0.2, 'ties are not everywhere'
        assert ((nib & 4) == 0).any() and ((nib & 4) != 0).any()
    gated = A.pool_backward(nib, dy, h, w, relu_gate=True)
    old = np.full((2, h, w, 6), 3.0)
    assert np.array_equal(A.pool_backward(nib, dy, h, w, old=old, relu_gate=True), gated + 3)
    assert not gated[:, 2 * ph:].any() and not gated[:, :, 2 * pw:].any()
    by = A.pool_idx_bytes(nib).reshape(2, ph, pw, 3)
    assert np.array_equal(by & 15, nib[..., 0::2]) and np.array_equal(by >> 4, nib[..., 1::2])


def test_layout_restatements():
    img = np.arange(256, dtype=np.uint8)[None, :, None, None].repeat(3, axis=3).reshape(1, 16, 16, 3)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    f64 = (img / 255.0 - np.array(mean)) / np.array(std)
    for dtn, rel in (('f32', 2.0 ** -22), ('f16', 2.0 ** -10), ('bf16', 2.0 ** -7)):
        got = A.u8hwc(img, mean, std, dtn)
        assert np.array_equal(got, A.round_np(got, dtn)) and np.abs(got - f64).max() <= rel * np.abs(f64).max()
    x = np.arange(2 * 3 * 4 * 5, dtype=np.float32).reshape(2, 3, 4, 5)
    fr = A.nchw_to_framed(x, 8, 'f32')
    assert fr.shape == (2, 4, 5, 8) and fr[1, 2, 3, 1] == x[1, 1, 2, 3] and not fr[..., 3:].any()
    assert np.array_equal(A.framed_to_nchw(fr)[:, :3], x)
    sc = A.nchw_to_framed_ch(np.full((2, 4, 5, 8), 9.0), x[:, :1], 4, 'bf16')
    assert np.array_equal(sc[..., 4], A.round_np(x[:, 0], 'bf16')) and (np.delete(sc, 4, axis=3) == 9).all()
    ad = A.framed_add_ch(fr, fr, 0, 2, 1, 'f32')
    assert np.array_equal(ad[..., 1], fr[..., 1] + fr[..., 0]) and np.array_equal(ad[..., 2], fr[..., 2] + fr[..., 1])
    assert np.array_equal(ad[..., 0], fr[..., 0]) and np.array_equal(ad[..., 3:], fr[..., 3:])


# ---------------------------------------------------------------------------------------------------------------- (b) the exact premise
@pytest.mark.parametrize('name,content', [(c.name, 'dense') for c in A.BWD.values() if c.exact] + [(n, 'impulse') for n in A.VARIANTS])
def test_premise_of_the_exact_backward_cases(name, content):
    case = A.BWD[name]
    assert case.exact
    m = A.make_bwd(case, content)
    assert set(np.unique(m['dy'])) <= {-2, -1, 0, 1, 2} and set(np.unique(m['gate'])) == {-1, 0, 1}
    A.assert_exact_premise(case.h, case.w, case.hs, case.ws, m['ref'], m['ref_abs'])


@pytest.mark.parametrize('name', [c.name for c in A.FWD.values() if c.exact])
def test_premise_of_the_exact_forward_cases(name):
    case = A.FWD[name]
    m = A.make_fwd(case)
    A.assert_exact_premise(case.ho, case.wo, case.hi, case.wi, m['ref'], m['ref_abs'])


def test_the_interval_geometries_are_not_exact():
    for c in list(A.BWD.values()) + list(A.FWD.values()):
        o, i = (c.h, c.hs) if hasattr(c, 'hs') else (c.ho, c.hi)
        co = np.concatenate(A.bilin_coef(o, i)[2:]).astype(np.float64) * 8
        assert np.array_equal(co, np.rint(co)) == c.exact, c.name


# ---------------------------------------------------------------------------------------------------------------- (c) the cap
@pytest.mark.parametrize('name', INTERVAL_BWD)
@pytest.mark.parametrize('dtn', ['bf16', 'f16'])
def test_few_backward_outputs_admit_more_than_one_value(name, dtn):
    case = A.BWD[name]
    m = A.make_bwd(case)
    K = A.k_bwd(case.path, case.h, case.w, case.hs, case.ws)
    for gated in (False, True):
        lo, hi, share = A.bwd_bounds(case, m, dtn, gated)
        print('%s %s K %d gate %d: %.2f %% of the outputs admit more than one value' % (name, dtn, K, gated, 100 * share))
        assert share <= CAP[dtn], (name, dtn, K, share)
        assert (lo <= hi).all() and np.array_equal(lo, A.round_np(lo, dtn))


@pytest.mark.parametrize('name', INTERVAL_FWD)
@pytest.mark.parametrize('dtn', ['bf16', 'f16'])
def test_few_forward_outputs_admit_more_than_one_value(name, dtn):
    case = A.FWD[name]
    lo, hi, share = A.fwd_bounds(case, A.make_fwd(case), dtn)
    print('%s %s K %d: %.2f %% of the outputs admit more than one value' % (name, dtn, A.K_FWD, 100 * share))
    assert share <= CAP[dtn], (name, dtn, share)


def test_the_derived_K_of_every_interval_case():
    got = {n: A.k_bwd(A.BWD[n].path, A.BWD[n].h, A.BWD[n].w, A.BWD[n].hs, A.BWD[n].ws) for n in INTERVAL_BWD}
    # walk-7rows: 7 rows in a pair + 3 columns + 3; walk-workload: 6 + 4 + 3; rows-widest: 6 x 6 terms + 3; rows-2x-small-c: 4 x 4 + 3;
    # flat-third: 5 x 5 + 3
    assert got == {'walk-7rows': 13, 'walk-workload': 13, 'rows-widest': 39, 'rows-2x-small-c': 19, 'flat-third': 28}, got
    assert max(A.walk_rows(23, 11)) == 7 and int(A.nonzero_counts(33, 17).max()) == 3
    assert max(A.walk_rows(60, 30)) == 6 and int(A.nonzero_counts(60, 30).max()) == 4
    assert A.max_terms(12, 12, 5, 5) == 36 and A.max_terms(30, 30, 15, 15) == 16 and A.max_terms(10, 10, 4, 4) == 25


# ---------------------------------------------------------------------------------------------------------------- (d) sensitivity
def _caught(alt, lo, hi, dtn):
    """A kernel that computed `alt` would be caught: its stored value leaves [lo, hi] somewhere."""
    r = alt if dtn == 'f32' else A.round_np(alt, dtn)
    return bool(((r < lo) | (r > hi)).any())


def _probe_columns(case):
    """(seam columns, last column): the first source column of every segment but the first (the middle column where there is no seam)."""
    cols = [c_lo for c_lo, _ in A.seams(case.ws, max(case.nseg, 1))[1:]] or [case.ws // 2]
    return cols, case.ws - 1


@pytest.mark.parametrize('name', list(A.BWD))
@pytest.mark.parametrize('dtn', DTNS)
def test_every_backward_case_is_sensitive(name, dtn):
    case = A.BWD[name]
    m = A.make_bwd(case)
    Cn = case.cg * A.VEC[dtn]
    lo, hi, _ = A.bwd_bounds(case, m, dtn, gated=False)
    assert not _caught(m['ref'][..., :Cn], lo, hi, dtn)
    Uy, Ux = A.up_matrix(case.h, case.hs), A.up_matrix(case.w, case.ws)
    # swapped weights (a no-op where both source extents are 1: the two weights then land on the same pixel)
    swapped = A.up_backward(m['dy'], case.hs, case.ws, swap=True)[0][..., :Cn]
    if case.hs == 1 and case.ws == 1:
        assert np.array_equal(A.up_matrix(case.h, 1, True), Uy) and np.array_equal(A.up_matrix(case.w, 1, True), Ux)
    else:
        assert _caught(swapped, lo, hi, dtn), 'swapped weights pass'
    # one (destination row, destination column) term lost: at every seam column, in the last column, in the last source row (the
    # single-row last pair of the walk when hs is odd) -- the heaviest contributor, on the channels where dy is not zero there
    seam_cols, last = _probe_columns(case)
    probes = [(case.hs // 2, ix, 'seam column %d' % ix) for ix in seam_cols] + [(case.hs // 2, last, 'last column'), (case.hs - 1, case.ws // 2, 'last row')]
    if case.path == A.WALK and case.nseg > 1:
        assert all(0 < c < case.ws for c in seam_cols) and len(seam_cols) == case.nseg - 1
    for iy, ix, what in probes:
        oy, ox = int(np.argmax(Uy[:, iy])), int(np.argmax(Ux[:, ix]))
        wgt = Uy[oy, iy] * Ux[ox, ix]
        alt = m['ref'][..., :Cn].copy()
        if wgt == 0:                                        # a source that receives no term (out == 1): one that does not belong
            assert case.h == 1 and case.w == 1 and not alt[:, iy, ix].any()
            wgt = -1.0
        alt[:, iy, ix] -= wgt * m['dy'][:, oy, ox, :Cn]
        assert m['dy'][:, oy, ox, :Cn].any() and _caught(alt, lo, hi, dtn), 'a lost term at the %s passes' % what


@pytest.mark.parametrize('name', list(A.FWD))
@pytest.mark.parametrize('dtn', DTNS)
def test_every_forward_case_is_sensitive(name, dtn):
    case = A.FWD[name]
    m = A.make_fwd(case)
    Cn = case.cg * A.VEC[dtn]
    lo, hi, _ = A.fwd_bounds(case, m, dtn)
    assert not _caught(m['ref'][..., :Cn], lo, hi, dtn)
    Uy, Ux = A.up_matrix(case.ho, case.hi, True), A.up_matrix(case.wo, case.wi, True)
    swapped = np.einsum('ai,bj,nijc->nabc', Uy, Ux, m['x'][..., :Cn])
    if case.hi == 1 and case.wi == 1:
        assert np.array_equal(swapped, m['ref'][..., :Cn])
    else:
        assert _caught(swapped, lo, hi, dtn), 'swapped weights pass'
    alt = m['ref'][..., :Cn].copy()                          # the last pixel computed from the last source pixel alone
    alt[:, -1, -1] = m['x'][:, -1, -1, :Cn] * 0.5
    assert _caught(alt, lo, hi, dtn)


def test_impulse_pixels_cover_corners_seams_last_row_and_column():
    for name in A.VARIANTS:
        case = A.BWD[name]
        px = set(A.impulse_pixels(case))
        n, h, w = case.n, case.h, case.w
        assert {(i, y, x) for i in (0, n - 1) for y in (0, h - 1) for x in (0, w - 1)} <= px
        assert any(x == w - 1 and 0 < y < h - 1 for _, y, x in px) and any(y == h - 1 and 0 < x < w - 1 for _, y, x in px)
        x0 = A.bilin_coef(w, case.ws)[0]
        for c_lo, _ in A.seams(case.ws, max(case.nseg, 1))[1:]:
            sides = {int(x0[x]) >= c_lo for _, y, x in px if abs(int(x0[x]) - c_lo) <= 1 and y == 1}
            assert sides == {False, True}, (name, c_lo)
        m = A.make_bwd(case, 'impulse')
        assert m['dy'].sum() == len(px) and set(np.unique(m['dy'])) == {0, 1}
        assert m['dy'][..., :4 * case.cg].sum() == len(px)     # every impulse lies in the channels f32 sees
    assert A.seams(25, 3) == [(0, 8), (8, 16), (16, 25)]


# ---------------------------------------------------------------------------------------------------------------- (e) the tables
def _kernel_range(in_size, out_size, pair):
    """The kernels' own [lo, hi] of destination indices per source index (or per source pair), restated in float32."""
    s = A.ac_scale(in_size, out_size)
    i = np.arange(0, in_size, 2 if pair else 1)
    i1 = np.minimum(i + 1, in_size - 1) if pair else i
    if not s > 0:
        return np.zeros_like(i), np.full_like(i, out_size - 1)
    lo = np.floor((i - 1).astype(np.float32) / s).astype(np.int64)
    hi = np.ceil((i1 + 1).astype(np.float32) / s).astype(np.int64)
    return np.maximum(lo, 0), np.minimum(hi, out_size - 1)


def test_tables_cannot_overflow_inside_the_dispatch_ranges():
    """Sizes 2 .. 259 on either side.  walk (scale in (0.45, 1)): at most MAXR = 8 destination rows per source-row pair (7 reached), x0
    non-decreasing in steps of 0 or 1 (the two rolling accumulators), both weights on x0 and x0 + 1.  rows (scale > 0.34): a window of
    at most WIN = 8 destination columns per source column (6 reached) and at most MAXR = 16 rows.  In both, the [lo, hi] range the
    kernel scans -- floor((i - 1) / s), ceil((i + 1) / s) in float -- holds every destination index with weight."""
    walk_max, win_max, cnt_max = 0, 0, 0
    walk_at, win_at = None, None
    for out_size in range(2, 260):
        d = np.arange(out_size)
        for in_size in range(2, 260):
            s = A.ac_scale(in_size, out_size)
            if not s > np.float32(0.34):
                continue
            i0, i1, l0, l1 = A.bilin_coef(out_size, in_size)
            nz0, nz1 = l0 != 0, (l1 != 0)
            first = np.full(in_size, out_size)
            last = np.full(in_size, -1)
            for idx, nz in ((i0, nz0), (i1, nz1)):
                np.minimum.at(first, idx[nz], d[nz])
                np.maximum.at(last, idx[nz], d[nz])
            # destinations with weight per source index (a destination whose two indices coincide counts once)
            cnt = np.bincount(np.concatenate([i0[nz0], i1[nz1 & ((i1 != i0) | ~nz0)]]), minlength=in_size)
            lo, hi = _kernel_range(in_size, out_size, pair=False)
            got = last >= 0
            assert (lo[got] <= first[got]).all() and (hi[got] >= last[got]).all(), ('rows range', in_size, out_size)
            span = int((last - first + 1)[got].max())
            assert span <= 8 and int(cnt.max()) <= 16, ('WIN / MAXR of the rows kernel', in_size, out_size, span, int(cnt.max()))
            if span > win_max:
                win_max, win_at = span, (in_size, out_size)
            cnt_max = max(cnt_max, int(cnt.max()))
            if np.float32(0.45) < s < 1:
                assert ((np.diff(i0) == 0) | (np.diff(i0) == 1)).all() and (i1 <= i0 + 1).all(), ('x0 steps', in_size, out_size)
                plo, phi = _kernel_range(in_size, out_size, pair=True)
                pf = np.minimum(first[0::2], first[np.minimum(np.arange(0, in_size, 2) + 1, in_size - 1)])
                pl = np.maximum(last[0::2], last[np.minimum(np.arange(0, in_size, 2) + 1, in_size - 1)])
                assert (plo <= pf).all() and (phi >= pl).all(), ('walk range', in_size, out_size)
                rows = int((pl - pf + 1).max())                # (contiguous: every destination between the first and last carries weight)
                assert rows <= 8, ('MAXR', in_size, out_size, rows)
                if rows > walk_max:
                    walk_max, walk_at = rows, (in_size, out_size)
    assert (walk_max, walk_at) == (7, (11, 23)), (walk_max, walk_at)
    assert (win_max, win_at) == (6, (5, 12)), (win_max, win_at)
    assert cnt_max <= 6
    assert max(A.walk_rows(23, 11)) == 7 and int(A.nonzero_counts(12, 5).max()) == 6


# ---------------------------------------------------------------------------------------------------------------- (f) the plan
def query(dtn, dy, dx):
    out = _lib.UpsampleBwdPlan()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    v = [_lib.View(None, g.n, g.h, g.w, g.pad, g.ld, 0, g.c) for g in (dy, dx)]
    _lib.check(_lib.lib().dbx_upsample_bilinear_bwd_plan(_lib.DTYPE_ID[dtn], C.byref(v[0]), C.byref(v[1]), C.byref(out)))
    return A.Plan(out.kernel, out.nseg, out.workgroups, out.lds_bytes)


@pytest.mark.parametrize('name', list(A.BWD))
@pytest.mark.parametrize('dtn', DTNS)
def test_plan_of_every_case(name, dtn):
    case = A.BWD[name]
    dy, dx = A.geos(case, dtn)
    plan = query(dtn, dy, dx)
    assert plan == A.plan_ref(dtn, dy, dx) and (plan.kernel, plan.nseg) == (case.path, case.nseg), (name, dtn, plan)
    wide = (dy._replace(ld=dy.ld + 96, pad=0), dx._replace(ld=dx.ld + 48, pad=1))              # the view variant's frames
    assert query(dtn, *wide) == plan


def test_plan_of_the_named_cases():
    p = {n: query('bf16', *A.geos(A.BWD[n], 'bf16')) for n in A.BWD}
    assert p['walk-dyadic-1seg'] == A.Plan(A.WALK, 1, 10, 17 * 12) and p['walk-dyadic-1seg'].workgroups % 8 != 0
    assert p['walk-dyadic-segs'] == A.Plan(A.WALK, 3, 9, 49 * 12) and p['walk-rounds2'] == A.Plan(A.WALK, 2, 4, 33 * 12)
    assert A.BWD['walk-rounds2'].cg == 256 + 64 and A.BWD['rows-below-walk'].cg == 63 and 9 * 63 > 256
    assert p['rows-below-walk'] == A.Plan(A.ROWS, 0, 18, 9 * 36) and p['flat-quarter'] == A.Plan(A.FLAT, 0, 1, 0)
    assert A.ac_scale(11, 23) == np.float32(10) / np.float32(22) > np.float32(0.45)
    assert np.float32(0.34) < A.ac_scale(5, 12) and A.ac_scale(4, 10) < np.float32(0.34)


def test_plan_on_the_workload_shapes_and_the_dispatch_edges():
    """Host only.  The 2**32 guard cannot be exercised on the GPU within a few seconds (a framed dy of more than 8 GB): it is asserted
    here, through the library's query, and nowhere else."""
    def both(dtn, dy, dx):
        plan = query(dtn, dy, dx)
        assert plan == A.plan_ref(dtn, dy, dx), (dtn, dy, dx, plan)
        return plan
    G = A.Geo
    # the training step: batch 64, the 2048-channel hidden gradient 60 x 60 -> 30 x 30, and the 512- / 256-channel maps
    assert both('bf16', G(64, 60, 60, 0, 2048, 2048), G(64, 30, 30, 1, 2048, 2048)) == A.Plan(A.WALK, 3, 64 * 15 * 3, 720)
    assert both('f16', G(64, 60, 60, 1, 768, 512), G(64, 30, 30, 1, 512, 512)) == A.Plan(A.WALK, 3, 2880, 720)
    assert both('f32', G(64, 60, 60, 1, 768, 256), G(64, 30, 30, 1, 256, 256)) == A.Plan(A.WALK, 3, 2880, 720)
    assert both('bf16', G(1, 60, 60, 0, 2048, 2048), G(1, 30, 30, 1, 2048, 2048)).nseg == 3       # capped at one segment per 8 columns
    assert both('bf16', G(64, 60, 130, 0, 2048, 2048), G(64, 30, 65, 1, 2048, 2048)).nseg == 4     # 12288 / 3840 + 1
    assert both('bf16', G(1, 60, 60, 0, 4096, 4096), G(1, 30, 30, 1, 4096, 4096)).kernel == A.WALK  # two channel-group rounds
    # dy.w: 4096 walks, 4097 does not (its 12-byte column table); dx.w 2049 is past the rows kernel's 1536 too
    assert both('bf16', G(1, 5, 4096, 0, 512, 512), G(1, 3, 2048, 1, 512, 512)).kernel == A.WALK
    assert both('bf16', G(1, 5, 4097, 0, 512, 512), G(1, 3, 2049, 1, 512, 512)) == A.Plan(A.FLAT, 0, min(-(-3 * 2049 * 64 // 256), 8192), 0)
    # dx.w: 1536 is tabulated, 1537 is flat (below the walk's channel threshold); with 64 groups the walk takes it
    assert both('bf16', G(1, 5, 3071, 0, 64, 64), G(1, 3, 1536, 1, 64, 64)) == A.Plan(A.ROWS, 0, 3, 1536 * 36)
    assert both('bf16', G(1, 5, 3073, 0, 64, 64), G(1, 3, 1537, 1, 64, 64)).kernel == A.FLAT
    assert both('bf16', G(1, 5, 3073, 0, 512, 512), G(1, 3, 1537, 1, 512, 512)).kernel == A.WALK
    # the walk keeps dy's row offsets in 32 bits: a framed dy of 2**32 elements or more takes the rows kernel
    assert 582 * 3600 * 2048 < 2 ** 32 <= 583 * 3600 * 2048
    assert both('bf16', G(582, 60, 60, 0, 2048, 2048), G(582, 30, 30, 1, 2048, 2048)).kernel == A.WALK
    assert both('bf16', G(583, 60, 60, 0, 2048, 2048), G(583, 30, 30, 1, 2048, 2048)) == A.Plan(A.ROWS, 0, 583 * 30, 30 * 36)
    assert both('bf16', G(64, 60, 60, 0, 18641, 2048), G(64, 30, 30, 1, 2048, 2048)).kernel == A.WALK
    assert both('bf16', G(64, 60, 60, 0, 18648, 2048), G(64, 30, 30, 1, 2048, 2048)).kernel == A.ROWS   # the span counts ld, not c
    assert both('bf16', G(520, 60, 60, 1, 2048, 2048), G(520, 30, 30, 1, 2048, 2048)).kernel == A.WALK   # ... and the frame: 62 x 62
    assert both('bf16', G(546, 60, 60, 1, 2048, 2048), G(546, 30, 30, 1, 2048, 2048)).kernel == A.ROWS
    assert 64 * 62 * 62 * 2048 == 503840768 < 2 ** 32 // 8                                      # the batch-64 map: 5.0e8 elements
    # scale thresholds: exactly 1 and down-sampling are the rows kernel's, scale 0 the flat one's
    assert both('bf16', G(1, 9, 9, 0, 512, 512), G(1, 9, 9, 1, 512, 512)).kernel == A.ROWS
    assert both('bf16', G(1, 5, 5, 0, 512, 512), G(1, 9, 9, 1, 512, 512)).kernel == A.ROWS
    assert both('bf16', G(1, 1, 1, 0, 512, 512), G(1, 9, 9, 1, 512, 512)).kernel == A.FLAT
    assert both('bf16', G(1, 9, 9, 0, 512, 512), G(1, 1, 1, 1, 512, 512)).kernel == A.FLAT
