"""The threshold pyramid on the GPU.  dbx_thresh_rows_batch writes, bit for bit, the rows, indices and counts dbx_detect_thresh_batch
writes, in slot layout and nothing else; dbx_merge_nms_thresh_batch writes the packed rows of tests/pyramid_thresh_ref and the keep
lists of that restatement and of dbx_nms_large on every frame's union, and nothing outside them; detect_pyramid(score_thresh=...) equals
the composition of detect_batch_resized(score_thresh=...) per size + a host concatenate + decode.NMS per frame, with one resize launch
per call, len(sizes) rows launches and one merge launch per chunk."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyramid_thresh_ref as PT                         # noqa: E402
import thresh_ref                                       # noqa: E402

import densebox_amd as D                                # noqa: E402
from densebox_amd import _lib, decode as DC, resize, synth      # noqa: E402
from densebox_amd._lib import check, ptr, stream_ptr    # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 512                    # sentinel bytes in front of and behind every buffer
MODES = ('box', 'hm', 'll')    # det_cols 5; 13 from heat maps; 13 from offsets
KINDS = ['DenseBox', 'DenseBoxLM', 'DenseBoxLMLOC']


def _guarded(nbytes):
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    return buf, buf[GUARD:GUARD + nbytes]


def _guards_intact(named):
    for name, g in named.items():
        a = g.cpu().numpy()
        assert (a[:GUARD] == 0xA5).all() and (a[-GUARD:] == 0xA5).all(), name + ': written outside the buffer'


# ------------------------------------------------------------------------------------------------------------ the rows kernel
def _maps_of(maps, mode):
    return (maps['score'], maps['loc'], maps['lm_heat'] if mode != 'box' else None, maps['lm_loc'] if mode == 'll' else None,
            5 if mode == 'box' else 13)


def _rows_abi(maps, mode, t, cap):
    """dbx_thresh_rows_batch with sentinels: per image (rows [n_b, dc], indices [n_b], (n_b, pixels above t))"""
    s, l, hm, ll, dc = _maps_of(maps, mode)
    B, _, rows, cols = s.shape
    L = _lib.lib()
    g_d, dets = _guarded(B * cap * dc * 8)
    g_t, topk = _guarded(B * cap * 8)
    g_c, counts = _guarded(B * 2 * 4)
    g_s, scratch = _guarded(L.dbx_thresh_rows_batch_scratch_bytes(B, rows, cols, cap))
    check(L.dbx_thresh_rows_batch(ptr(s), ptr(l), ptr(hm), ptr(ll), B, rows, cols, t, cap, ptr(dets), dc, ptr(topk), ptr(counts),
                                  ptr(scratch), stream_ptr()))
    torch.cuda.synchronize()
    _guards_intact(dict(dets=g_d, topk=g_t, counts=g_c, scratch=g_s))
    pairs = counts.cpu().numpy().view(np.int32).reshape(B, 2)
    d, tk = dets.cpu().numpy().reshape(B, cap * dc * 8), topk.cpu().numpy().reshape(B, cap * 8)
    out = []
    for b in range(B):
        n = int(pairs[b, 0])
        assert 0 <= n <= cap
        assert (d[b, n * dc * 8:] == 0xA5).all() and (tk[b, n * 8:] == 0xA5).all(), 'slot %d: written beyond row n_b' % b
        out.append((d[b, :n * dc * 8].view(np.float64).reshape(n, dc).copy(), tk[b, :n * 8].view(np.int64).copy(),
                    (n, int(pairs[b, 1]))))
    return out


def _detect_thresh_abi(maps, mode, t, cap):
    """dbx_detect_thresh_batch, the existing entry point, on the same maps: per image (rows, indices, (n_b, pixels above t))"""
    s, l, hm, ll, dc = _maps_of(maps, mode)
    B, _, rows, cols = s.shape
    L = _lib.lib()
    dets = torch.zeros(B * cap * dc, dtype=torch.float64, device='cuda')
    keep = torch.zeros(B * (cap + 1), dtype=torch.int32, device='cuda')
    topk = torch.zeros(B * cap, dtype=torch.int64, device='cuda')
    counts = torch.zeros(3 * B + 1, dtype=torch.int32, device='cuda')
    scratch = torch.empty(L.dbx_detect_thresh_batch_scratch_bytes(B, rows, cols, cap), dtype=torch.uint8, device='cuda')
    check(L.dbx_detect_thresh_batch(ptr(s), ptr(l), ptr(hm), ptr(ll), B, rows, cols, t, cap, 0.4, ptr(dets), dc, ptr(topk), ptr(keep),
                                    ptr(counts), ptr(scratch), stream_ptr()))
    c, d, tk = counts.cpu().numpy(), dets.cpu().numpy().reshape(-1, dc), topk.cpu().numpy()
    out = []
    for b in range(B):
        p, n = int(c[2 * B + b]), int(c[2 * b])
        out.append((d[p:p + n].copy(), tk[p:p + n].copy(), (n, int(c[2 * b + 1]))))
    return out


def _stack(images):
    return {k: torch.from_numpy(np.ascontiguousarray(np.concatenate([m[k] for m in images]))).cuda() for k in images[0]}


def _rows_images(batch):
    """crafted maps with 0 candidates, a few, many (cut by the smaller caps); the last image of a batch carries ties, NaN and +-inf"""
    counts = {1: (1500,), 3: (700, 0, 63), 5: (2, 0, 1025, 4096, 1500)}[batch]
    images = [thresh_ref.craft_maps(50 * batch + i, 128, 128, n, 9) for i, n in enumerate(counts)]
    rs = np.random.RandomState(batch)
    s = images[-1]['score']
    s[:] = (np.round(s * 16.0) / 16.0).astype(np.float32)
    flat = s.reshape(-1)
    flat[rs.choice(flat.size, 300, replace=False)] = np.nan
    flat[rs.choice(flat.size, 20, replace=False)] = np.inf
    flat[rs.choice(flat.size, 20, replace=False)] = -np.inf
    return images


@pytest.mark.parametrize('batch', [1, 3, 5])
def test_rows_kernel_is_bitwise_the_threshold_decode(batch):
    images = _rows_images(batch)
    maps = _stack(images)
    seen = set()
    for mode in MODES:
        for t, cap in ((0.5, 4096), (0.5, 1000), (0.5, 64), (0.25, 700), (2.0, 100), (float('inf'), 100)):     # 2.0 leaves the +inf pixels, +inf nothing
            got, want = _rows_abi(maps, mode, t, cap), _detect_thresh_abi(maps, mode, t, cap)
            for b, ((gd, gt, gc), (wd, wt, wc)) in enumerate(zip(got, want)):
                print('batch %d %s t %g cap %d image %d: n %d of %d above' % (batch, mode, t, cap, b, gc[0], gc[1]))
                assert gc == wc, (mode, t, cap, b, gc, wc)
                with np.errstate(invalid='ignore'):
                    assert gc[1] == int((images[b]['score'] > np.float32(t)).sum()) and gc[0] == min(gc[1], cap)
                assert gd.shape == wd.shape and gd.tobytes() == wd.tobytes(), (mode, t, cap, b, 'rows')
                assert np.array_equal(gt, wt), (mode, t, cap, b, 'indices')
                seen.add('empty' if gc[1] == 0 else ('below' if gc[1] < cap else ('cut' if gc[1] > cap else 'at')))
    assert seen >= {'empty', 'below', 'cut'}, seen


# ------------------------------------------------------------------------------------------------------------ the merge kernels
def _keep_list(k):
    return [int(v) for v in k[1:1 + int(k[0])]]


def _merge_abi(frames, counts, xforms, cap, thresh=0.4, behind=False, ws=None, raw_counts=None):
    """dbx_merge_nms_thresh_batch on frames[b][l] = [cap, dc] rows, counts[b][l], xforms[b][l], with sentinels around every output and
    in their unwritten parts.  raw_counts: what the device count words hold, where that is not counts.  Returns (per frame (rows,
    keep list), pairs [batch][levels][2], the workspace)."""
    batch, levels, dc = len(frames), len(frames[0]), frames[0][0].shape[1]
    raw = counts if raw_counts is None else raw_counts
    dev = [torch.from_numpy(np.ascontiguousarray(np.stack([frames[b][l] for b in range(batch)]))).cuda() for l in range(levels)]
    cnt_np = [np.array([[raw[b][l], raw[b][l] + 3 * l + b] for b in range(batch)], np.int32) for l in range(levels)]
    cnt = [torch.from_numpy(c).cuda() for c in cnt_np]
    nrow = batch * levels * cap
    g_d, od = _guarded(nrow * dc * 8 + ((nrow + batch) * 4 if behind else 0))
    g_k, ok = _guarded((nrow + batch) * 4)
    g_c, oc = _guarded((2 * batch * levels + batch + 1) * 4)
    L = _lib.lib()
    nws = L.dbx_merge_nms_thresh_batch_workspace_bytes(levels, batch, cap)
    if ws is None:
        ws = _guarded(nws)
    assert ws[1].numel() == nws and ws[1].data_ptr() % 256 == 0
    dp = (C.c_void_p * levels)(*[t.data_ptr() for t in dev])
    cp = (C.c_void_p * levels)(*[t.data_ptr() for t in cnt])
    xf = (_lib.MergeXform * (levels * batch))()
    for l in range(levels):
        for b in range(batch):
            xf[l * batch + b].scale, xf[l * batch + b].off_x, xf[l * batch + b].off_y = xforms[b][l]
    check(L.dbx_merge_nms_thresh_batch(dp, cp, xf, levels, batch, cap, dc, thresh, ptr(od), ptr(od if behind else ok), ptr(oc),
                                       ptr(ws[1]), stream_ptr()))
    for l in range(levels):                                  # the caller's host arrays may be reused on return
        dp[l] = None
        cp[l] = None
    C.memset(xf, 0xFF, C.sizeof(xf))
    torch.cuda.synchronize()
    _guards_intact(dict(out_dets=g_d, out_keep=g_k, out_counts=g_c, workspace=ws[0]))
    for t, l in zip(dev, range(levels)):
        assert t.cpu().numpy().tobytes() == np.stack([frames[b][l] for b in range(batch)]).tobytes(), 'an input level was written'
    for t, a in zip(cnt, cnt_np):
        assert np.array_equal(t.cpu().numpy(), a), 'an input count was written'
    c = oc.cpu().numpy().view(np.int32)
    pairs, prefix = c[:2 * batch * levels].reshape(batch, levels, 2), c[2 * batch * levels:]
    m = [sum(PT.clamp(n, cap) for n in counts[b]) for b in range(batch)]
    assert prefix.tolist() == [0] + np.cumsum(m).tolist(), (prefix, m)
    for b in range(batch):
        for l in range(levels):
            assert pairs[b, l].tolist() == [PT.clamp(raw[b][l], cap), raw[b][l] + 3 * l + b], (b, l, pairs[b, l])
    total = int(prefix[batch])
    d = od.cpu().numpy()
    kb = d[total * dc * 8:] if behind else ok.cpu().numpy()
    # packed: exactly `total` rows and total + batch list words are written; everything behind them is untouched
    assert (kb[(total + batch) * 4:] == 0xA5).all(), 'out_keep: written behind the lists'
    if behind:
        assert (ok.cpu().numpy() == 0xA5).all()
    else:
        assert (d[total * dc * 8:] == 0xA5).all(), 'out_dets: written behind the packed rows'
    rows = d[:total * dc * 8].view(np.float64).reshape(total, dc)
    lists = kb[:(total + batch) * 4].view(np.int32)
    out = []
    for b in range(batch):
        p = int(prefix[b])
        k = lists[p + b:p + b + m[b] + 1]
        assert 0 <= k[0] <= m[b] and (k[0] > 0 or m[b] == 0)
        out.append((rows[p:p + m[b]].copy(), _keep_list(k)))
    return out, pairs, ws


def _nms_large(d, th):
    n, dc = d.shape
    L = _lib.lib()
    t = torch.from_numpy(np.ascontiguousarray(d)).cuda()
    keep = torch.zeros(n + 1, dtype=torch.int32, device='cuda')
    scr = torch.empty(L.dbx_nms_large_scratch_bytes(n), dtype=torch.uint8, device='cuda')
    check(L.dbx_nms_large(ptr(t), n, dc, th, ptr(keep), ptr(scr), stream_ptr()))
    return _keep_list(keep.cpu().numpy())


def _check_case(frames, counts, xforms, cap, thresh, what, **kw):
    """the kernel against the restatement and dbx_nms_large, and the case's own non-triviality on the kernel's output"""
    got, _, ws = _merge_abi(frames, counts, xforms, cap, thresh, **kw)
    levels = len(frames[0])
    two = nms = False
    for b, (gd, gk) in enumerate(got):
        union, keep = PT.merge_nms(frames[b], counts[b], xforms[b], cap, thresh)
        print('%s frame %d: counts %s, %d rows, %d kept' % (what, b, [PT.clamp(n, cap) for n in counts[b]], len(gd), len(gk)))
        assert gd.shape == union.shape and gd.tobytes() == union.tobytes(), (what, b, 'rows')
        assert gk == keep, (what, b, 'restatement')
        if len(gd):
            assert gk == _nms_large(gd, thresh), (what, b, 'dbx_nms_large')
            assert all(0 <= k < len(gd) for k in gk) and len(set(gk)) == len(gk)
        else:
            assert gk == []
        two = two or sum(PT.clamp(n, cap) > 0 for n in counts[b]) >= 2
        nms = nms or 1 < len(gk) < len(gd)
    assert nms and (two or levels == 1), (what, 'the case proves nothing: two levels %s, suppression %s' % (two, nms))
    return got, ws


@pytest.mark.parametrize('dc', [5, 13])
@pytest.mark.parametrize('batch', [1, 3, 5])
def test_merge_kernels_are_bitwise_the_restatement_and_the_single_nms(batch, dc):
    """1 to 4 levels; per (level, frame) 0 everywhere, 0 at some levels, 1, 63, 64, 65 and max_dets rows; continuous and quantised
    scores (ties across levels), NaN scores and boxes, identical boxes at several levels"""
    for levels in (1, 2, 3, 4):
        frames, counts, xforms = PT.grid_case(levels, batch, dc)
        _check_case(frames, counts, xforms, 100, 0.4, 'levels %d batch %d dc %d' % (levels, batch, dc), behind=(levels % 2 == 0))


@pytest.mark.parametrize('which', [0, 1])
def test_a_union_of_exactly_4096_rows(which):
    frames, counts, xforms, cap = PT.full_case(which)
    got, _ = _check_case(frames, counts, xforms, cap, 0.4, 'full %d' % which, behind=bool(which))
    assert len(got[0][0]) == 4096


def test_counts_above_max_dets_are_clamped_on_the_device():
    frames, counts, xforms = PT.grid_case(3, 3, 13)
    raw = [[c + 1000 if c == 100 else (-5 if c == 0 else c) for c in fr] for fr in counts]
    assert any(c > 100 for fr in raw for c in fr) and any(c < 0 for fr in raw for c in fr)
    got, pairs, _ = _merge_abi(frames, counts, xforms, 100, raw_counts=raw)
    for b, (gd, gk) in enumerate(got):
        union, keep = PT.merge_nms(frames[b], raw[b], xforms[b], 100)
        assert gd.tobytes() == union.tobytes() and gk == keep, b


def test_other_nms_thresholds_and_a_second_call_in_the_same_workspace():
    frames, counts, xforms = PT.grid_case(3, 5, 13)
    kept = {}
    ws = None
    for th in (0.0, 0.4, 0.7):
        got, ws = _check_case(frames, counts, xforms, 100, th, 'nms_thresh %g' % th, ws=ws)
        kept[th] = [len(k) for _, k in got]
    assert kept[0.0] != kept[0.4] != kept[0.7]
    # other (smaller) counts over what the calls above left in the workspace
    small = [[max(0, c - 37) for c in fr] for fr in counts]
    _check_case(frames, small, xforms, 100, 0.4, 'reused workspace', ws=ws)
    again, _ = _check_case(frames, counts, xforms, 100, 0.7, 'reused workspace, first counts', ws=ws)
    assert [len(k) for _, k in again] == kept[0.7]


@pytest.mark.parametrize('dc', [5, 13])
def test_equal_counts_give_the_fixed_k_merge(dc):
    """all counts equal to K: rows and keep lists are dbx_merge_nms_batch's"""
    L = _lib.lib()
    for levels, batch, K in ((2, 3, 10), (3, 5, 100), (4, 1, 300)):
        rs = np.random.RandomState(levels * K + dc)
        kinds = [(b + levels) % 4 for b in range(batch)]
        frames = [PT.frame_levels(rs, k, levels, K, dc) for k in kinds]
        xforms = [PT.frame_xforms(k, b, levels) for b, k in enumerate(kinds)]
        got, _ = _check_case(frames, [[K] * levels] * batch, xforms, K, 0.4, 'equal counts %d x %d' % (levels, K))
        n = levels * K
        dev = [torch.from_numpy(np.ascontiguousarray(np.stack([frames[b][l] for b in range(batch)]))).cuda() for l in range(levels)]
        od = torch.zeros((batch, n, dc), dtype=torch.float64, device='cuda')
        ok = torch.zeros((batch, n + 1), dtype=torch.int32, device='cuda')
        ptrs = (C.c_void_p * levels)(*[t.data_ptr() for t in dev])
        xf = (_lib.MergeXform * (levels * batch))()
        for l in range(levels):
            for b in range(batch):
                xf[l * batch + b].scale, xf[l * batch + b].off_x, xf[l * batch + b].off_y = xforms[b][l]
        ws = torch.empty(L.dbx_merge_nms_batch_workspace_bytes(levels, batch, K), dtype=torch.uint8, device='cuda')
        check(L.dbx_merge_nms_batch(ptrs, xf, levels, batch, K, dc, 0.4, ptr(od), ptr(ok), ptr(ws), stream_ptr()))
        od, ok = od.cpu().numpy(), ok.cpu().numpy()
        for b, (gd, gk) in enumerate(got):
            assert gd.tobytes() == od[b].tobytes() and gk == _keep_list(ok[b]), (levels, K, b)


# ------------------------------------------------------------------------------------------------------------ the pipeline
def _img(rs, h, w):
    img = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    img[::7] = 0
    img[:, ::11] = 255
    return img


def _net(kind, dtype='f32'):
    net = getattr(D, kind)(synth.vgg19_standin(seed=0))
    synth.fill_params_(net, 11)
    net = net.cuda().eval()
    net.compute_dtype = dtype
    return net


MIXED = ((120, 200), (200, 120), (160, 160), (97, 240), (240, 97))
SIZES = (160, 240, 320)


def _threshold_leaving(net, frames, size, count):
    """the score of frame 0 at the `size` level that leaves about `count` of its pixels above it (the tree has no trained weights)"""
    x = resize.pad_resize_batch(frames[:1], size)
    with torch.no_grad():
        s = DC._maps(net.KIND, net(x))[0][0]
    return float(torch.sort(s.reshape(-1).float(), descending=True).values[count])


def _composition(net, frames, sizes, t, cap, th=0.4, max_batch=32):
    """What a user composes from the single-size call: detect_batch_resized(score_thresh=...) per size, a host concatenate, decode.NMS
    per frame.  Per frame (rows, keep list, rows per level)."""
    per = [net.detect_batch_resized(frames, size=s, nms_thresh=th, max_batch=max_batch, score_thresh=t, max_dets=cap) for s in sizes]
    out = []
    for i in range(len(per[0])):
        d = np.concatenate([per[l][i][0] for l in range(len(sizes))], axis=0)
        out.append((d, DC.NMS(d, th) if len(d) else [], [len(per[l][i][0]) for l in range(len(sizes))]))
    return out


def _assert_results(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[0].dtype == np.float64 and g[0].shape == w[0].shape, (what, i, g[0].shape, w[0].shape)
        assert g[0].tobytes() == w[0].tobytes(), (what, i, 'rows')
        assert g[1] == w[1], (what, i, 'keep')
        if len(g) > 2:
            assert np.asarray(g[2]).tolist() == list(w[2]), (what, i, 'rows per level')


@pytest.mark.parametrize('dtype', ['f32', 'f16'])
@pytest.mark.parametrize('kind', KINDS)
def test_detect_pyramid_with_a_threshold_is_the_composition_bit_for_bit(kind, dtype):
    net = _net(kind, dtype)
    dc = 5 if kind == 'DenseBox' else 13
    rs = np.random.RandomState(41)
    frames = [_img(rs, h, w) for h, w in MIXED]
    batch = np.stack([_img(rs, 120, 200) for _ in range(3)])
    for count, cap in ((150, 1024), (1500, 1000)):        # a few hundred rows per frame; a level above max_dets
        t = _threshold_leaving(net, frames, SIZES[1], count)
        want = _composition(net, frames, SIZES, t, cap)
        per_level = [w[2] for w in want]
        print(kind, dtype, 'threshold %r cap %d: rows per level and frame %s' % (t, cap, per_level))
        if count < cap:
            assert 100 <= len(want[0][0]) <= 2000, 'the pick was to leave a few hundred rows'
        else:
            assert want[0][2][1] == cap, 'the 240 level of frame 0 was to exceed max_dets'
        # untrained weights: the boxes are whatever the random heads give, so how many rows the NMS removes is printed, not asserted
        # (the kernel tests above assert suppression on plate-like boxes); the levels do meet in one union here
        print('    kept per frame', [len(w[1]) for w in want])
        assert any(sum(n > 0 for n in p) >= 2 for p in per_level) and all(1 <= len(w[1]) <= len(w[0]) for w in want if len(w[0]))
        got = net.detect_pyramid(frames, sizes=SIZES, score_thresh=t, max_dets=cap, with_levels=True)
        _assert_results(got, want, 'numpy list')
        assert all(g[2].shape == (3,) and g[2].dtype.kind == 'i' for g in got)
        two = net.detect_pyramid(frames, sizes=SIZES, score_thresh=t, max_dets=cap)
        assert all(len(g) == 2 for g in two)
        _assert_results(two, want, 'replay')
        _assert_results(net.detect_pyramid([torch.from_numpy(f).cuda() for f in frames], sizes=SIZES, score_thresh=t, max_dets=cap),
                        want, 'device-resident frames')
        want_b = _composition(net, torch.from_numpy(batch), SIZES, t, cap)
        _assert_results(net.detect_pyramid(torch.from_numpy(batch), sizes=SIZES, score_thresh=t, max_dets=cap, with_levels=True),
                        want_b, 'uint8 batch tensor')
        _assert_results(net.detect_pyramid(torch.from_numpy(batch).cuda(), sizes=SIZES, score_thresh=t, max_dets=cap), want_b,
                        'uint8 batch tensor on the device')
    for d, keep, lv in net.detect_pyramid(frames, sizes=SIZES, score_thresh=1e30, with_levels=True):
        assert d.shape == (0, dc) and d.dtype == np.float64 and keep == [] and lv.tolist() == [0, 0, 0]


def _graphs(net):
    return {k: id(v[1]) for k, v in net.__dict__.get('_detect_graphs', {}).items()}


def test_eager_capture_replay_and_other_frames_through_the_cached_graphs(monkeypatch):
    rs = np.random.RandomState(42)
    frames = [_img(rs, *MIXED[i % 5]) for i in range(5)]
    other = [_img(rs, *MIXED[i % 5]) for i in range(5)]
    for kind in KINDS:
        net = _net(kind, 'f16')
        t = _threshold_leaving(net, frames, SIZES[1], 200)
        with monkeypatch.context() as m:
            m.setenv('DBX_GRAPH', '0')
            eager = net.detect_pyramid(frames, sizes=SIZES, score_thresh=t, max_batch=5, with_levels=True)
            eager_other = net.detect_pyramid(other, sizes=SIZES, score_thresh=t, max_batch=5, with_levels=True)
            assert not [k for k in net.__dict__.get('_detect_graphs', {}) if k[0] == 'level_thresh']
        _assert_results(net.detect_pyramid(frames, sizes=SIZES, score_thresh=t, max_batch=5, with_levels=True), eager, kind + ' capture')
        snap = _graphs(net)
        keys = [k for k in snap if k[0] == 'level_thresh']
        assert {k[1] for k in keys} == {(5, s, s, 3) for s in SIZES} and all(k[3] == (1024, t) for k in keys), list(snap)
        _assert_results(net.detect_pyramid(frames, sizes=SIZES, score_thresh=t, max_batch=5, with_levels=True), eager, kind + ' replay')
        _assert_results(net.detect_pyramid(other, sizes=SIZES, score_thresh=t, max_batch=5, with_levels=True), eager_other,
                        kind + ' other frames')
        assert _graphs(net) == snap, 'a call through the cached graphs captured a new one'
        assert [g[2].tolist() for g in eager] != [g[2].tolist() for g in eager_other]
        assert len(net.__dict__['_detect_graphs']) <= DC._MAX_GRAPHS
    # train mode runs the same launches eagerly (its forward draws dropout masks, so only the structure is checked)
    net = _net('DenseBoxLMLOC', 'f16')
    net.train()
    res = net.detect_pyramid(frames, sizes=SIZES, score_thresh=t, with_levels=True)
    assert not net.__dict__.get('_detect_graphs')
    for d, keep, lv in res:
        assert d.shape == (int(lv.sum()), 13) and keep == (DC.NMS(d, 0.4) if len(d) else [])


def test_chunking_in_f32():
    """max_batch 2 over 5 frames.  f32: the chunk size changes the batch of every forward, and only the fp32 forward is bit for bit
    independent of its batch."""
    net = _net('DenseBoxLMLOC', 'f32')
    rs = np.random.RandomState(43)
    frames = [_img(rs, *MIXED[i % 5]) for i in range(5)]
    t = _threshold_leaving(net, frames, SIZES[1], 300)
    whole = net.detect_pyramid(frames, sizes=SIZES, score_thresh=t, with_levels=True)
    _assert_results(whole, _composition(net, frames, SIZES, t, 1024), 'one chunk')
    chunked = net.detect_pyramid(frames, sizes=SIZES, score_thresh=t, max_batch=2, with_levels=True)        # chunks of 2, 2, 1
    _assert_results(chunked, [tuple(w) for w in whole], 'max_batch 2 against 32')
    _assert_results(chunked, _composition(net, frames, SIZES, t, 1024, max_batch=2), 'max_batch 2 against the composition')
    _assert_results(net.detect_pyramid(frames, sizes=SIZES, score_thresh=t, max_batch=2, with_levels=True), chunked, 'replay')
    assert len(net.__dict__['_detect_graphs']) <= DC._MAX_GRAPHS


def test_one_resize_launch_per_call_rows_and_merge_launches_per_chunk(monkeypatch):
    net = _net('DenseBoxLM', 'f16')
    rs = np.random.RandomState(44)
    frames = [_img(rs, *MIXED[i % 5]) for i in range(7)]
    t = _threshold_leaving(net, frames, SIZES[1], 200)
    L = _lib.lib()
    names = ['dbx_resize_cubic_batch_u8', 'dbx_thresh_rows_batch', 'dbx_merge_nms_thresh_batch', 'dbx_detect_thresh_batch',
             'dbx_nms_large', 'dbx_nms', 'dbx_merge_nms_batch', 'dbx_detect_batch']
    calls = {n: [] for n in names + ['decode.NMS']}

    def wrap(name):
        real = getattr(L, name)

        def f(*a):
            calls[name].append(a)
            return real(*a)
        monkeypatch.setattr(L, name, f)
    for name in names:
        wrap(name)
    real_nms = DC.NMS
    monkeypatch.setattr(DC, 'NMS', lambda *a, **k: calls['decode.NMS'].append(a) or real_nms(*a, **k))
    unused = ('dbx_detect_thresh_batch', 'dbx_nms_large', 'dbx_nms', 'dbx_merge_nms_batch', 'dbx_detect_batch', 'decode.NMS')
    for max_batch, chunks in ((32, 1), (3, 3), (4, 2)):
        for rep in range(2):                                 # the capturing call warms up through the binding; the replay is bare
            for v in calls.values():
                del v[:]
            res = net.detect_pyramid(frames, sizes=SIZES, score_thresh=t, max_batch=max_batch)
            assert len(res) == 7
            assert len(calls['dbx_resize_cubic_batch_u8']) == 1, (max_batch, rep)
            assert calls['dbx_resize_cubic_batch_u8'][0][1] == 7 * len(SIZES)          # B * L jobs
            assert len(calls['dbx_merge_nms_thresh_batch']) == chunks, (max_batch, rep)
            assert [c[4] for c in calls['dbx_merge_nms_thresh_batch']] == [min(max_batch, 7 - i) for i in range(0, 7, max_batch)]
            assert all(c[3] == len(SIZES) and c[5] == 1024 for c in calls['dbx_merge_nms_thresh_batch'])
            assert all(len(calls[n]) == 0 for n in unused), {n: len(calls[n]) for n in unused}
        assert len(calls['dbx_thresh_rows_batch']) == 0, 'a replay launches the rows kernel from the graph, not through the binding'
    with monkeypatch.context() as m:
        m.setenv('DBX_GRAPH', '0')
        for v in calls.values():
            del v[:]
        net.detect_pyramid(frames, sizes=SIZES, score_thresh=t, max_batch=3)
        assert (len(calls['dbx_resize_cubic_batch_u8']), len(calls['dbx_merge_nms_thresh_batch'])) == (1, 3)
        assert len(calls['dbx_thresh_rows_batch']) == 3 * len(SIZES)                     # one per level per chunk
        assert all(len(calls[n]) == 0 for n in unused)
