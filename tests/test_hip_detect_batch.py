"""Batched inference on the GPU: dbx_detect_batch is image by image the single-image decode bit for bit; detect_batch's forward,
graph replay, uint8 input, list grouping and graph cache (one graph per batch shape) give the per-image results they should."""
import numpy as np
import pytest
import torch

import densebox_amd as D
from densebox_amd import decode as DC
from densebox_amd import synth
from oracle import densebox_oracle as O

pytestmark = pytest.mark.gpu

KINDS = ['DenseBox', 'DenseBoxLM', 'DenseBoxLMLOC']
TOL = {'f32': 1e-4, 'f16': 3.8e-3}          # flat forward bars of tests/test_hip_forward.py


def _net(kind, dtype, seed=11):
    net = getattr(D, kind)(synth.vgg19_standin(seed=0))
    synth.fill_params_(net, seed)
    net = net.cuda().eval()
    net.compute_dtype = dtype
    return net


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(-1)


def _same(a, b):
    """bit-for-bit equality of two arrays (NaN rows included)"""
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _keep_list(k):
    return [int(v) for v in k[1:1 + int(k[0])]]


def _stack_from_fixture(g):
    """B = 4 map stacks from the fixture's 60 x 60 maps: as they are; a fixed pixel permutation; quantised scores (ties across
    the K-th place); some NaN scores."""
    s, l, hm, ll = g['a_s'], g['a_l'], g['a_hm'], g['a_ll']
    n = s.shape[2] * s.shape[3]
    perm = np.random.RandomState(17).permutation(n)

    def permuted(m):
        return m.reshape(m.shape[0], m.shape[1], n)[:, :, perm].reshape(m.shape)
    s2 = (np.round(s * 8.0) / 8.0).astype(np.float32)
    s3 = s.copy()
    s3.reshape(-1)[np.random.RandomState(18).choice(n, 200, replace=False)] = np.nan
    ss = np.concatenate([s, permuted(s), s2, s3])
    ls = np.concatenate([l, permuted(l), l, l])
    hms = np.concatenate([hm, permuted(hm), hm[:, ::-1], hm])
    lls = np.concatenate([ll, permuted(ll), ll, -ll])
    return [torch.from_numpy(np.ascontiguousarray(m)).cuda() for m in (ss, ls, hms, lls)]


def _check_against_single(s, l, hm, ll, K, th=0.4):
    """dbx_detect_batch over the stack == dbx_detect on every image's own maps, bit for bit (rows, top-K indices, keep lists)"""
    B, _, rows, cols = s.shape
    dets, topk, keep = DC._run_batch(s, l, K, lm_heat=hm, lm_loc=ll, nms_thresh=th)
    dets, topk, keep = dets.cpu().numpy(), topk.cpu().numpy(), keep.cpu().numpy()
    assert dets.shape == (B, K, 5 if hm is None and ll is None else 13)
    for b in range(B):
        sl = lambda t: None if t is None else t[b:b + 1]          # noqa: E731
        d1, t1, k1 = DC._run(sl(s), sl(l), rows * 4, cols * 4, K, lm_heat=sl(hm), lm_loc=sl(ll), nms_thresh=th)
        k1 = k1.cpu().numpy()
        assert _same(dets[b], d1.cpu().numpy()), (K, b, 'rows')
        assert np.array_equal(topk[b], t1.cpu().numpy()), (K, b, 'top-K')
        assert _keep_list(keep[b]) == _keep_list(k1), (K, b, 'keep')
    return dets, keep


def test_batched_decode_is_bitwise_the_single_image_decode(golden):
    g = golden('decode')
    s, l, hm, ll = _stack_from_fixture(g)
    fixture = {(5, 10): 'a_parse_output', (5, 50): 'a_parse_out_MN_K50', ('hm', 10): 'a_parse_DetLM', ('ll', 10): 'a_parse_DetLMLOC'}
    for K in (7, 10, 50, 1000):                          # tourney (K <= 48) and radix select (49..1024) on a 60 x 60 map
        for mode, h, lo in ((5, None, None), ('hm', hm, None), ('ll', hm, ll)):
            dets, keep = _check_against_single(s, l, h, lo, K)
            name = fixture.get((mode, K))
            if name is not None:                         # image 0 = the fixture's maps: the reference's rows and keep list
                assert _same(dets[0], g[name]), name
                assert _keep_list(keep[0]) == list(g[name + '_keep']), name
            assert np.isnan(dets[3][:, 4]).sum() == 0 or K > 3600 - 200   # NaN ranks below every number
    # the 1080p input's 270 x 480 map: K = 10 takes the rounds path through GLOBAL scratch (per-image slices), K = 1000 select
    rs = np.random.RandomState(5)
    s = torch.from_numpy(rs.rand(3, 1, 270, 480).astype(np.float32)).cuda()
    s[1] = torch.round(s[1] * 16) / 16                   # ties
    l = torch.from_numpy((rs.randn(3, 4, 270, 480) * 8).astype(np.float32)).cuda()
    for K in (10, 1000):
        _check_against_single(s, l, None, None, K)


def test_batched_forward_per_image_matches_single_image_forward():
    x = synth.synth_images(4, 512, 512, seed=21).cuda()
    for kind in KINDS:
        net = _net(kind, 'f32')
        with torch.no_grad():
            ref = [[o.cpu().numpy() for o in net(x[b:b + 1])] for b in range(4)]
            got32 = [o.cpu().numpy() for o in net(x)]
        net.compute_dtype = 'f16'
        with torch.no_grad():
            outs16 = net(x)
            got16 = [o.cpu().numpy() for o in outs16]
        for dtype, got in (('f32', got32), ('f16', got16)):
            for i, o in enumerate(got):
                for b in range(4):
                    r = ref[b][i][0]
                    err = float(np.abs(o[b] - r).max())
                    assert err <= TOL[dtype] * max(1.0, float(np.abs(r).max())), (kind, dtype, i, b, err)
        # graph-mode detect_batch == dbx_detect_batch on the eager batched maps, per image, bit for bit
        s, l, hm, ll = DC._maps(kind, outs16)
        dets, _, keep = DC._run_batch(s, l, 10, lm_heat=hm, lm_loc=ll, nms_thresh=0.4)
        dets, keep = dets.cpu().numpy(), keep.cpu().numpy()
        res = net.detect_batch(x, K=10, nms_thresh=0.4)
        res2 = net.detect_batch(x, K=10, nms_thresh=0.4)          # replay
        assert len(res) == 4
        for b in range(4):
            for d, k in (res[b], res2[b]):
                assert _same(d, dets[b]) and k == _keep_list(keep[b]), (kind, b)


def test_detect_batch_fixture_1080p(golden):
    g = golden('net_DenseBox_1080p')
    net = _net('DenseBox', 'f32')
    res = net.detect_batch(synth.synth_images(2, 1080, 1920, seed=5), K=10, nms_thresh=0.4)     # (CPU input)
    dets, keep = res[0]
    assert dets.shape == (10, 5) and dets.dtype == np.float64
    assert np.allclose(dets, g['dets'], rtol=1e-4, atol=2e-3)
    assert keep == list(g['keep'])
    assert len(res) == 2 and res[1][0].shape == (10, 5)


def test_batch_of_one_is_detect():
    x = synth.synth_images(2, 512, 512, seed=9).cuda()
    for kind in KINDS:
        net = _net(kind, 'f16')
        d1, k1 = net.detect(x[0:1], K=10, nms_thresh=0.4)
        [(d2, k2)] = net.detect_batch(x[0:1], K=10, nms_thresh=0.4)
        assert _same(d1, d2) and k1 == k2, kind


def test_uint8_batch_equals_normalised_float_batch():
    rs = np.random.RandomState(4)
    u8 = torch.from_numpy(rs.randint(0, 256, size=(3, 512, 512, 3)).astype(np.uint8))
    xf = O.normalize_u8(u8)
    net = _net('DenseBoxLM', 'f16')
    a = net.detect_batch(u8.cuda(), K=10)
    b = net.detect_batch(xf.cuda(), K=10)
    c = net.detect_batch([u8[i] for i in range(3)], K=10)       # list of [H,W,3] uint8 images, from the host
    assert len(a) == len(b) == len(c) == 3
    for (da, ka), (db, kb), (dc, kc) in zip(a, b, c):
        assert _same(da, db) and ka == kb
        assert _same(da, dc) and ka == kc


def _eager(monkeypatch, fn):
    with monkeypatch.context() as m:
        m.setenv('DBX_GRAPH', '0')
        return fn()


def _assert_same_results(got, want, what):
    assert len(got) == len(want), what
    for i, ((dg, kg), (dw, kw)) in enumerate(zip(got, want)):
        assert _same(dg, dw) and kg == kw, (what, i)


def test_list_input_order_graph_cache_and_training_step(monkeypatch):
    from densebox_amd.optim import SGD
    net = _net('DenseBoxLMLOC', 'f16')
    big = synth.synth_images(3, 512, 512, seed=31)
    small = synth.synth_images(2, 240, 240, seed=32)
    images = [big[0], small[0:1], big[1], small[1], big[2:3]]      # [3,H,W] and [1,3,H,W] mixed
    # groups: 512^2 -> images 0, 2 | 4 (max_batch 2), 240^2 -> images 1, 3; expected results from those chunks run eagerly
    def expected():
        e = {}
        for idx, t in (([0, 2], big[0:2]), ([4], big[2:3]), ([1, 3], small)):
            for i, r in zip(idx, DC.detect_batch(net, t, K=10)):
                e[i] = r
        return [e[i] for i in range(5)]
    want = _eager(monkeypatch, expected)
    want_list = _eager(monkeypatch, lambda: net.detect_batch(images, K=10, max_batch=2))
    _assert_same_results(want_list, want, 'eager list')
    got = net.detect_batch(images, K=10, max_batch=2)              # captures
    _assert_same_results(got, want, 'graph list (capture)')
    got = net.detect_batch(images, K=10, max_batch=2)              # replays
    _assert_same_results(got, want, 'graph list (replay)')
    assert not _same(got[0][0], got[2][0]) and not _same(got[1][0], got[3][0])
    # a training step: new weights -> the cached graphs must re-capture
    net.train()
    net.compute_dtype = 'f16'
    opt = SGD(net.parameters(), lr=2e-9, momentum=0.9, weight_decay=5e-8)
    x, bbox, vert, lab = synth.synth_batch(2, seed=7, neg_frac=0.0)
    outs = net(x.cuda())
    loss = net.loss(outs, bbox, vert, lab)
    loss.backward()
    opt.step()
    net.eval()
    got2 = net.detect_batch(images, K=10, max_batch=2)
    assert not _same(got2[0][0], got[0][0]), 'detections did not change after a weight update (stale graph)'
    _assert_same_results(got2, _eager(monkeypatch, expected), 'graph list after a training step')
    # B = 4 and B = 2 graphs of one image shape, alternated: each replays its own buffers
    x4 = synth.synth_images(4, 240, 240, seed=41).cuda()
    x2 = synth.synth_images(2, 240, 240, seed=42).cuda()
    w4 = _eager(monkeypatch, lambda: net.detect_batch(x4, K=10))
    w2 = _eager(monkeypatch, lambda: net.detect_batch(x2, K=10))
    for _ in range(2):
        _assert_same_results(net.detect_batch(x4, K=10), w4, 'B = 4')
        _assert_same_results(net.detect_batch(x2, K=10), w2, 'B = 2')
    with pytest.raises(RuntimeError, match='K='):
        net.detect_batch(x2, K=60 * 60 + 1)
