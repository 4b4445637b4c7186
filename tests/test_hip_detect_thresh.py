"""Score-threshold decode on the GPU: dbx_detect_thresh_batch == the NumPy restatement (oracle parse_det(K = n_b) + nms) == the fixture
captured from the reference == the existing top-K kernel at K = n_b, bit for bit (rows as bytes, index lists as integers), for candidate
counts on both sides of every size class of the NMS; the cap; dbx_nms_large == dbx_nms; nothing outside an image's own blocks is
written; detect_batch_thresh / detect_batch_resized / detect_plates compose it as they say."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import densebox_amd as D
from densebox_amd import _lib, decode as DC, rectify, resize, synth
from densebox_amd._lib import check, ptr, stream_ptr
from oracle import densebox_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thresh_ref  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 512                    # sentinel bytes in front of and behind every buffer
MODES = ('box', 'hm', 'll')    # det_cols 5; 13 from heat maps; 13 from offsets


def _guarded(nbytes):
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    return buf, buf[GUARD:GUARD + nbytes]


def _run_abi(maps, mode, t, cap, nms=0.4, behind=False):
    """dbx_detect_thresh_batch on a stack of maps with sentinels around (and in the unwritten parts of) every buffer.  Returns per image
    (rows, topk, keep list, pixels above t) after the containment checks."""
    s, l = maps['score'], maps['loc']
    hm = maps['lm_heat'] if mode != 'box' else None
    ll = maps['lm_loc'] if mode == 'll' else None
    dc = 5 if mode == 'box' else 13
    B, _, rows, cols = s.shape
    L = _lib.lib()
    nd, nk = B * cap * dc * 8, B * (cap + 1) * 4
    g_d, dets = _guarded(nd + (nk if behind else 0))
    g_k, keep = _guarded(nk)
    g_t, topk = _guarded(B * cap * 8)
    g_c, counts = _guarded((3 * B + 1) * 4)
    nscr = L.dbx_detect_thresh_batch_scratch_bytes(B, rows, cols, cap)
    g_s, scratch = _guarded(nscr)
    assert scratch.data_ptr() % 256 == 0
    check(L.dbx_detect_thresh_batch(ptr(s), ptr(l), ptr(hm), ptr(ll), B, rows, cols, t, cap, nms, ptr(dets), dc, ptr(topk),
                                    ptr(dets if behind else keep), ptr(counts), ptr(scratch), stream_ptr()))
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in dict(d=g_d, k=g_k, t=g_t, c=g_c, s=g_s).items()}
    for name, a in h.items():                                   # the guards of every buffer, scratch included, survive
        assert (a[:GUARD] == 0xA5).all() and (a[-GUARD:] == 0xA5).all(), name
    cnt = h['c'][GUARD:-GUARD].view(np.int32)
    pairs, prefix = cnt[:2 * B].reshape(B, 2), cnt[2 * B:]
    assert prefix[0] == 0 and np.array_equal(prefix[1:], np.cumsum(pairs[:, 0])), (pairs, prefix)     # exclusive prefix + total
    total = int(prefix[B])
    d = h['d'][GUARD:-GUARD]
    kb = (d[total * dc * 8:] if behind else h['k'][GUARD:-GUARD])
    # packed: exactly `total` rows, `total` indices and total + B list words are written; everything behind them is untouched
    assert (kb[(total + B) * 4:] == 0xA5).all()
    if behind:
        assert (h['k'][GUARD:-GUARD] == 0xA5).all()
    else:
        assert (d[total * dc * 8:] == 0xA5).all()
    assert (h['t'][GUARD:-GUARD][total * 8:] == 0xA5).all()
    rows_all = d[:total * dc * 8].view(np.float64).reshape(total, dc)
    tk = h['t'][GUARD:-GUARD][:total * 8].view(np.int64)
    lists = kb[:(total + B) * 4].view(np.int32)
    out = []
    for b in range(B):
        p, n = int(prefix[b]), int(pairs[b, 0])
        k = lists[p + b:p + b + n + 1]
        assert 0 <= k[0] <= n
        out.append((rows_all[p:p + n].copy(), tk[p:p + n].copy(), [int(v) for v in k[1:1 + int(k[0])]], int(pairs[b, 1])))
    return out


def _stack(images):
    return {k: torch.from_numpy(np.ascontiguousarray(np.concatenate([m[k] for m in images]))).cuda() for k in images[0]}


def _ref(m, mode, t, cap, nms=0.4):
    rows, cols = m['score'].shape[2:]
    return thresh_ref.thresh_detect(m['score'], m['loc'], m['lm_heat'] if mode != 'box' else None, m['lm_loc'] if mode == 'll' else None,
                                    rows * 4, cols * 4, t, cap, nms)


def _old_kernel(maps, b, mode, K, nms=0.4):
    """the existing top-K kernel on image b's maps, NaN scores included: rows, indices, keep list.  Every path of its selection, the
    arg-max rounds of K > 1024 too, ranks NaN below every number (tests/test_hip_topk_paths.py), as the threshold kernel does by never
    admitting NaN."""
    sl = lambda k: maps[k][b:b + 1]          # noqa: E731
    score = sl('score')
    d, tk, kp = DC._run_batch(score, sl('loc'), K, lm_heat=sl('lm_heat') if mode != 'box' else None,
                              lm_loc=sl('lm_loc') if mode == 'll' else None, nms_thresh=nms)
    kp = kp.cpu().numpy()[0]
    return d.cpu().numpy()[0], tk.cpu().numpy()[0], [int(v) for v in kp[1:1 + int(kp[0])]]


STACKS = [        # (rows, cols, plates, candidate counts of the B = 4 images): every size class of sort and NMS, 0 between two others
    (60, 60, 4, (2, 0, 63, 1)),
    (128, 128, 9, (64, 65, 1023, 1024)),
    (128, 128, 9, (1025, 4095, 0, 4096)),
    (270, 480, 12, (65, 1025, 0, 2)),
    (25, 33, 2, (1, 0, 63, 2)),
]


@pytest.mark.parametrize('case', range(len(STACKS)))
def test_kernel_is_the_numpy_restatement(case):
    rows, cols, plates, counts = STACKS[case]
    images = [thresh_ref.craft_maps(100 * case + i, rows, cols, n, plates) for i, n in enumerate(counts)]
    maps = _stack(images)
    for mode in MODES:
        for behind in ((False, True) if mode == 'll' else (False,)):
            got = _run_abi(maps, mode, 0.5, 4096, behind=behind)
            for b, (m, n) in enumerate(zip(images, counts)):
                d, keep, total = _ref(m, mode, 0.5, 4096)
                gd, gt, gk, gtot = got[b]
                assert gtot == total == n and gd.shape == d.shape, (mode, b, gtot, total, gd.shape)
                assert gd.tobytes() == d.tobytes(), (mode, b, 'rows')
                assert gk == keep, (mode, b, 'keep')
                s = m['score'].reshape(-1)
                assert np.array_equal(s[gt].astype(np.float64), gd[:, 4]) and len(set(gt.tolist())) == n, (mode, b, 'indices')
                if 1 <= n <= 1025 and (rows, cols) != (270, 480) or n == 65:
                    od, ot, ok = _old_kernel(maps, b, mode, n)
                    assert gd.tobytes() == od.tobytes() and np.array_equal(gt, ot) and gk == ok, (mode, b, 'top-K kernel')
            assert len(got[1][2]) == 0 or counts[1] > 0


def test_kernel_is_the_reference_on_the_captured_fixture(golden):
    g = golden('decode_thresh')
    maps = {k: torch.from_numpy(g[k]).cuda() for k in ('score', 'loc', 'lm_heat', 'lm_loc')}
    [(d, tk, keep, total)] = _run_abi(maps, 'll', float(g['t']), 4096, float(g['nms_thresh']))
    assert total == g['rows'].shape[0] > 1024
    assert d.tobytes() == g['rows'].tobytes()
    assert keep == [int(v) for v in g['keep']]
    [(d, tk, keep, total)] = _run_abi(maps, 'll', float(g['t']), 1000, float(g['nms_thresh']))
    assert total == g['rows'].shape[0] and d.tobytes() == g['rows'][:1000].tobytes()


def _tie_stack():
    """B = 4 at 60 x 60 for the HIP-against-HIP cases: quantised scores (ties inside the candidate set and across the cap); NaN and
    +-inf scores; signed zeros; a plain crafted image whose scores include the threshold itself."""
    base = [thresh_ref.craft_maps(900 + i, 60, 60, 1500, 4) for i in range(4)]
    rs = np.random.RandomState(77)
    base[0]['score'] = (np.round(base[0]['score'] * 16.0) / 16.0).astype(np.float32)
    s1 = base[1]['score'].reshape(-1)
    s1[rs.choice(3600, 300, replace=False)] = np.nan
    s1[rs.choice(3600, 40, replace=False)] = np.inf
    s1[rs.choice(3600, 40, replace=False)] = -np.inf
    s2 = base[2]['score'].reshape(-1)
    s2[rs.choice(3600, 500, replace=False)] = 0.0
    s2[rs.choice(3600, 500, replace=False)] = -0.0
    s2[rs.choice(3600, 300, replace=False)] = -0.25
    return base


@pytest.mark.parametrize('t,cap', [(0.5, 4096), (0.5, 1000), (0.5625, 4096), (0.0, 4096), (-0.0, 700), (float('-inf'), 1000),
                                   (float('-inf'), 10), (0.25, 1025), (float('inf'), 100)])
def test_ties_nan_and_the_cap_against_the_top_k_kernel(t, cap):
    """rows / indices / keep equal dbx_detect_batch with K = n_b on the same maps; the counts equal NumPy's strict fp32 comparison"""
    images = _tie_stack()
    maps = _stack(images)
    for mode in (('box', 'll') if cap >= 1000 else MODES):
        got = _run_abi(maps, mode, t, cap)
        for b, m in enumerate(images):
            gd, gt, gk, gtot = got[b]
            with np.errstate(invalid='ignore'):
                total = int((m['score'] > np.float32(t)).sum())
            assert gtot == total and gd.shape[0] == min(total, cap), (t, cap, mode, b, gtot, total)
            if gd.shape[0] == 0:
                assert gk == []
                continue
            if gd.shape[0] > 1024 and b >= 2:
                continue                              # the top-K kernel's slow path (K > 1024): two images per case
            od, ot, ok = _old_kernel(maps, b, mode, gd.shape[0])
            assert gd.tobytes() == od.tobytes(), (t, cap, mode, b, 'rows')
            assert np.array_equal(gt, ot), (t, cap, mode, b, 'indices')
            assert gk == ok, (t, cap, mode, b, 'keep')
    if t == 0.5625:                                   # a threshold that IS a score of image 3: that pixel is out
        assert (images[3]['score'] == np.float32(t)).sum() == 1


@pytest.mark.parametrize('cap', [1, 10, 1000, 4096])
def test_more_candidates_than_max_dets_is_top_max_dets(cap):
    rs = np.random.RandomState(3)
    B = 2
    maps = dict(score=torch.from_numpy(rs.rand(B, 1, 128, 128).astype(np.float32)).cuda(),
                loc=torch.from_numpy((rs.randn(B, 4, 128, 128) * 8).astype(np.float32)).cuda(),
                lm_heat=torch.from_numpy(rs.rand(B, 4, 128, 128).astype(np.float32)).cuda(),
                lm_loc=torch.from_numpy(rs.randn(B, 8, 128, 128).astype(np.float32)).cuda())
    maps['score'][1] = torch.round(maps['score'][1] * 64) / 64            # ties across the cap
    for mode in ('box', 'hm') if cap < 4096 else ('ll',):
        got = _run_abi(maps, mode, 0.1, cap)
        for b in range(B):
            gd, gt, gk, gtot = got[b]
            assert gtot == int((maps['score'][b] > 0.1).sum()) > cap and gd.shape[0] == cap
            od, ot, ok = _old_kernel(maps, b, mode, cap)
            assert gd.tobytes() == od.tobytes() and np.array_equal(gt, ot) and gk == ok, (cap, mode, b)


def _nms_pair(d, th):
    L = _lib.lib()
    n, dc = d.shape
    t = torch.from_numpy(d).cuda()
    res = []
    for large in (False, True):
        g_k, keep = _guarded((n + 1) * 4)
        nscr = L.dbx_nms_large_scratch_bytes(n) if large else 5 * n + 16
        g_s, scr = _guarded((nscr + 255) // 256 * 256)
        fn = L.dbx_nms_large if large else L.dbx_nms
        check(fn(ptr(t), n, dc, th, ptr(keep), ptr(scr), stream_ptr()))
        torch.cuda.synchronize()
        for a in (g_k.cpu().numpy(), g_s.cpu().numpy()):
            assert (a[:GUARD] == 0xA5).all() and (a[-GUARD:] == 0xA5).all()
        k = keep.cpu().numpy().view(np.int32)
        res.append([int(v) for v in k[1:1 + int(k[0])]])
    return res


@pytest.mark.parametrize('n', [1, 64, 65, 1024, 1025, 2500, 4096])
def test_nms_large_is_nms(n):
    rs = np.random.RandomState(n)
    for th in (0.0, 0.4, 0.7):
        for dc in (5, 13):
            d = rs.rand(n, dc) * 400.0
            d[:, 2:4] = d[:, 0:2] + rs.rand(n, 2) * 120.0
            d[:, 4] = rs.rand(n)
            old, new = _nms_pair(d, th)                       # distinct scores: NumPy's order is defined too
            assert new == old, (n, th, dc, 'distinct')
            if len(np.unique(d[:, 4])) == n:
                assert new == O.nms(d, th), (n, th, dc, 'oracle')
            # duplicates, equal scores, zero-area and inverted boxes, NaN scores and NaN coordinates, signed zeros, infinities
            e = d.copy()
            e[:, 4] = np.round(e[:, 4] * 8.0) / 8.0
            m = max(1, n // 10)
            e[rs.choice(n, m), :] = e[rs.choice(n, m), :]
            e[rs.choice(n, m), 2:4] = e[rs.choice(n, m), 0:2] - 1.0
            e[rs.choice(n, m), 4] = np.nan
            e[rs.choice(n, m), rs.randint(0, 4)] = np.nan
            e[rs.choice(n, m), 4] = -0.0
            e[rs.choice(n, m), 4] = 0.0
            e[rs.choice(n, max(1, m // 4)), 4] = np.inf
            e[rs.choice(n, max(1, m // 4)), 4] = -np.inf
            e[rs.choice(n, m), 4] = -e[rs.choice(n, m), 4]
            old, new = _nms_pair(e, th)
            assert new == old, (n, th, dc, 'ties and NaN')


# ---------------------------------------------------------------------------------------------- pipeline
def _net(kind, dtype, seed=11):
    net = getattr(D, kind)(synth.vgg19_standin(seed=0))
    synth.fill_params_(net, seed)
    net = net.cuda().eval()
    net.compute_dtype = dtype
    return net


def _threshold_leaving(net, x, count):
    """the score of image 0 of the batch x that leaves about `count` of its pixels above it (the tree has no trained weights)"""
    with torch.no_grad():
        s = DC._maps(net.KIND, net(x))[0][0]
    return float(torch.sort(s.reshape(-1), descending=True).values[count])


def _composition(net, x, t, cap, nms=0.4):
    """forward of the chunk eagerly, dbx_detect_thresh_batch on its maps through the ABI runner with sentinels"""
    with torch.no_grad():
        outs = net(x)
    s, l, hm, ll = DC._maps(net.KIND, outs)
    maps = dict(score=s.contiguous(), loc=l.contiguous(), lm_heat=hm, lm_loc=ll)
    mode = 'box' if net.KIND == 'DenseBox' else ('hm' if net.KIND == 'DenseBoxLM' else 'll')
    return [(d, k, tot) for d, _, k, tot in _run_abi(maps, mode, t, cap, nms)]


def _assert_results(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[0].dtype == np.float64 and g[0].shape == w[0].shape, (what, i, g[0].shape, w[0].shape)
        assert g[0].tobytes() == w[0].tobytes() and g[1] == w[1], (what, i)
        if len(g) > 2:
            assert g[2] == w[2], (what, i)


@pytest.mark.parametrize('kind', ['DenseBox', 'DenseBoxLM', 'DenseBoxLMLOC'])
def test_detect_batch_thresh_is_forward_plus_the_kernel(kind, monkeypatch):
    net = _net(kind, 'f16')
    x = synth.synth_images(4, 512, 512, seed=21).cuda()
    y = synth.synth_images(4, 512, 512, seed=22).cuda()
    for count, cap in ((300, 1024), (2000, 4096)):
        t = _threshold_leaving(net, x, count)
        want_x, want_y = _composition(net, x, t, cap), _composition(net, y, t, cap)
        assert want_x[0][0].shape[0] <= count and max(w[0].shape[0] for w in want_x + want_y) > (1024 if count > 1024 else 64)
        with monkeypatch.context() as m:
            m.setenv('DBX_GRAPH', '0')
            _assert_results(net.detect_batch_thresh(x, t, max_dets=cap, with_totals=True), want_x, 'eager')
        _assert_results(net.detect_batch_thresh(x, t, max_dets=cap, with_totals=True), want_x, 'graph (capture)')
        _assert_results(net.detect_batch_thresh(x, t, max_dets=cap, with_totals=True), want_x, 'graph (replay)')
        # other frames through the cached graph: other counts, their own results
        n_graphs = len(net._detect_graphs)
        _assert_results(net.detect_batch_thresh(y, t, max_dets=cap, with_totals=True), want_y, 'graph (other frames)')
        assert len(net._detect_graphs) == n_graphs
        assert [w[0].shape[0] for w in want_x] != [w[0].shape[0] for w in want_y]
        assert len(net.detect_batch_thresh(x, t, max_dets=cap)[0]) == 2
    # nothing above the threshold: empty rows of the right width, an empty keep list
    for d, k, tot in net.detect_batch_thresh(x, 1e30, with_totals=True):
        assert d.shape == (0, 5 if kind == 'DenseBox' else 13) and d.dtype == np.float64 and k == [] and tot == 0


def test_uint8_list_and_chunking(monkeypatch):
    net = _net('DenseBoxLMLOC', 'f32')
    rs = np.random.RandomState(4)
    u8 = torch.from_numpy(rs.randint(0, 256, size=(3, 240, 240, 3)).astype(np.uint8))
    t = _threshold_leaving(net, u8.cuda(), 300)
    a = net.detect_batch_thresh(u8.cuda(), t)
    _assert_results(a, [w[:2] for w in _composition(net, u8.cuda(), t, 1024)], 'uint8 batch')
    xf = O.normalize_u8(u8)
    _assert_results(net.detect_batch_thresh(xf, t), [w[:2] for w in _composition(net, xf.cuda(), t, 1024)], 'float batch from the host')
    # f32: one chunk == chunks of 2 and 1 (the f16 forward is not batch-invariant)
    _assert_results(net.detect_batch_thresh(u8, t, max_batch=2), a, 'max_batch = 2')
    # a list of mixed sizes: grouped by shape, results in input order
    big = synth.synth_images(2, 320, 256, seed=31)
    small = synth.synth_images(2, 240, 240, seed=32)
    images = [big[0], small[0:1], big[1], small[1]]
    got = net.detect_batch_thresh(images, t, max_dets=2048, with_totals=True)
    wb, ws = _composition(net, big.cuda(), t, 2048), _composition(net, small.cuda(), t, 2048)
    _assert_results(got, [wb[0], ws[0], wb[1], ws[1]], 'mixed list')


def _map_rows(d, h, w, size):
    side, pad_x, pad_y = resize.pad_geometry(h, w)
    s = side / size
    d = d.copy()
    xs = [0, 2] + list(range(5, d.shape[1], 2))
    ys = [1, 3] + list(range(6, d.shape[1], 2))
    d[:, xs] = d[:, xs] * s - pad_x
    d[:, ys] = d[:, ys] * s - pad_y
    return d


def test_resized_and_plates_with_a_threshold_and_without():
    net = _net('DenseBoxLMLOC', 'f16')
    rs = np.random.RandomState(8)
    frames = [torch.from_numpy(rs.randint(0, 256, size=s).astype(np.uint8)) for s in ((200, 300, 3), (240, 240, 3), (310, 170, 3))]
    x = resize.pad_resize_batch(frames, 240)
    t = _threshold_leaving(net, x, 400)
    base = net.detect_batch_thresh(x, t, max_dets=2048)
    got = net.detect_batch_resized(frames, size=240, score_thresh=t, max_dets=2048)
    _assert_results(got, [(_map_rows(d, f.size(0), f.size(1), 240), k) for f, (d, k) in zip(frames, base)], 'resized + threshold')
    assert sum(d.shape[0] for d, _ in got) > 0
    # without a threshold: the top-K composition, as before
    top = net.detect_batch(x, K=10)
    _assert_results(net.detect_batch_resized(frames, size=240), [(_map_rows(d, f.size(0), f.size(1), 240), k) for f, (d, k) in zip(frames, top)],
                    'resized, top-K')
    # plates: the batched warp on the kept rows of the threshold decode
    same = [torch.from_numpy(rs.randint(0, 256, size=(240, 240, 3)).astype(np.uint8)) for _ in range(2)]
    t = _threshold_leaving(net, torch.stack(same).cuda(), 200)
    for thr, ref in ((t, net.detect_batch_thresh(torch.stack(same), t, max_dets=512)), (None, net.detect_batch(torch.stack(same), K=10))):
        res = net.detect_plates(same, region='plate', score_thresh=thr, max_dets=512)
        _assert_results([r[:2] for r in res], ref, 'plates rows')
        quads = [[[d[k, 5:7], d[k, 7:9], d[k, 9:11], d[k, 11:13]] for k in keep] for d, keep in ref]
        want = rectify.perspective_transform_batch(same, quads, region='plate')
        for (_, keep, plates), w in zip(res, want):
            assert len(plates) == len(keep) == len(w)
            for p, q in zip(plates, w):
                assert (p is None) == (q is None)
                assert p is None or np.array_equal(np.asarray(p.cpu() if torch.is_tensor(p) else p), np.asarray(q.cpu() if torch.is_tensor(q) else q))
