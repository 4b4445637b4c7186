"""Pyramid detection on the GPU: dbx_merge_nms_batch writes, bit for bit, the rows of tests/pyramid_ref.merge and the keep lists of
dbx_nms / pyramid_ref.nms_stable on them, on all three paths of the NMS, and nothing outside its arrays; detect_pyramid equals the
composition of detect_batch_resized per size + a host concatenate + decode.NMS per frame, with one resize launch per call and one
merge launch per chunk; chunking, the shared graph cache and the eager path."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyramid_ref as P                                 # noqa: E402

import densebox_amd as D                                # noqa: E402
from densebox_amd import _lib, decode as DC, synth      # noqa: E402
from densebox_amd._lib import check, stream_ptr         # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64                       # sentinel elements in front of and behind each output array
SENT_D = -7.25e300               # a float64 no input produces
SENT_K = -0x5A5A5A5B
KINDS = ['DenseBox', 'DenseBoxLM', 'DenseBoxLMLOC']
# (scale, off_x, off_y) per level: 1080 x 1920 at 480 / 720 / 1080, and a portrait frame with an odd difference at 320
XFORMS = [(1920 / 480, 0.0, 420.0), (1920 / 720, 0.0, 420.0), (1920 / 1080, 0.0, 420.0), (517 / 320, 108.0, 0.0)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _keep_list(k):
    return [int(v) for v in k[1:1 + int(k[0])]]


def _merge_abi(level_np, xforms, thresh=0.4):
    """dbx_merge_nms_batch through ctypes on level_np[l] = [batch, K, dc] arrays and xforms[l][b]: (out_dets, out_keep) as NumPy arrays,
    after checking that the sentinel bands around both outputs are untouched."""
    levels, (batch, K, dc) = len(level_np), level_np[0].shape
    n = levels * K
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in level_np]
    od = torch.full((GUARD + batch * n * dc + GUARD,), SENT_D, dtype=torch.float64, device='cuda')
    ok = torch.full((GUARD + batch * (n + 1) + GUARD,), SENT_K, dtype=torch.int32, device='cuda')
    ptrs = (C.c_void_p * levels)(*[t.data_ptr() for t in dev])
    xf = (_lib.MergeXform * (levels * batch))()
    for l in range(levels):
        for b in range(batch):
            xf[l * batch + b].scale, xf[l * batch + b].off_x, xf[l * batch + b].off_y = xforms[l][b]
    L = _lib.lib()
    ws = torch.empty(L.dbx_merge_nms_batch_workspace_bytes(levels, batch, K), dtype=torch.uint8, device='cuda')
    check(L.dbx_merge_nms_batch(ptrs, xf, levels, batch, K, dc, thresh, C.c_void_p(od.data_ptr() + 8 * GUARD),
                                C.c_void_p(ok.data_ptr() + 4 * GUARD), C.c_void_p(ws.data_ptr()), stream_ptr()))
    for l in range(levels):                                  # the caller's host arrays may be reused on return
        ptrs[l] = None
    C.memset(xf, 0xFF, C.sizeof(xf))
    od, ok = od.cpu().numpy(), ok.cpu().numpy()
    for t, a in zip(dev, level_np):
        assert _same(t.cpu().numpy(), np.ascontiguousarray(a)), 'an input level was written'
    assert (od[:GUARD] == SENT_D).all() and (od[-GUARD:] == SENT_D).all(), 'out_dets: written outside the array'
    assert (ok[:GUARD] == SENT_K).all() and (ok[-GUARD:] == SENT_K).all(), 'out_keep: written outside the array'
    return od[GUARD:-GUARD].reshape(batch, n, dc), ok[GUARD:-GUARD].reshape(batch, n + 1)


def _frame_levels(rs, g, b, levels, K, dc):
    """The K rows of every level of frame b, in RESIZED-frame coordinates of that level.  Frame kinds by b % 5: continuous scores;
    scores quantised to 1/8 (ties within and ACROSS levels); every 7th score NaN; the same rows at every level (identical boxes and
    scores after the map when the transforms are equal -- see _xforms); rows of the decode fixture."""
    kind = b % 5
    if kind == 4:
        src = g['a_parse_DetLMLOC'] if dc == 13 else g['a_parse_out_MN_K50']
        out = []
        for l in range(levels):
            d = np.resize(src, (K, dc)).copy()
            d[:, :4] += (np.arange(K) // len(src))[:, None] * 3.0 + l          # repeated fixture rows drift apart a little
            out.append(d)
        return out
    if kind == 3:
        d = P.random_frame(rs, K, dc, span=700.0)
        return [d.copy() for _ in range(levels)]
    return [P.random_frame(rs, K, dc, span=1920.0 / XFORMS[l % 4][0], quantise=8 if kind == 1 else None, nan_every=7 if kind == 2 else 0)
            for l in range(levels)]


def _xforms(levels, batch):
    """[levels][batch]: the level's transform, except that frames of kind 3 use ONE transform at every level (identical boxes at
    several levels) and odd frames swap in the portrait transform with its odd offset at level 0."""
    out = []
    for l in range(levels):
        row = []
        for b in range(batch):
            t = XFORMS[l % 4]
            if b % 5 == 3:
                t = XFORMS[1]
            elif b % 2 == 1 and l == 0:
                t = XFORMS[3]
            row.append(t)
        out.append(row)
    return out


CASES = [(lv, K) for lv in (1, 2, 3, 4) for K in (10, 100, 300)] + [(1, 1000)]


@pytest.mark.parametrize('dc', [5, 13])
@pytest.mark.parametrize('batch', [1, 3, 5])
def test_merge_kernel_is_bitwise_the_restatement_and_the_single_nms(golden, batch, dc):
    """n = levels * K covers the greedy path (n <= 64), the suppression-matrix path (64 < n <= 1024) and the global path (n = 1200) of
    nms_block.  NaN scores included: the NMS ranks them where NumPy's sort does (first), so nms_stable holds there too."""
    g = golden('decode')
    paths = set()
    for levels, K in CASES:
        rs = np.random.RandomState(1000 * levels + K + 7 * batch + dc)
        n = levels * K
        paths.add('greedy' if n <= 64 else ('matrix' if n <= 1024 else 'global'))
        frames = [_frame_levels(rs, g, b if batch > 1 else (levels + K // 10) % 5, levels, K, dc) for b in range(batch)]
        level_np = [np.stack([frames[b][l] for b in range(batch)]) for l in range(levels)]
        xf = _xforms(levels, batch) if batch > 1 else [[XFORMS[l % 4]] for l in range(levels)]
        od, ok = _merge_abi(level_np, xf)
        for b in range(batch):
            want = P.merge(frames[b], [xf[l][b] for l in range(levels)])
            assert _same(od[b], want), (levels, K, b, 'rows')
            assert _same(od[b][:, 4], np.concatenate([f[:, 4] for f in frames[b]])), (levels, K, b, 'scores')
            keep = _keep_list(ok[b])
            assert 1 <= ok[b, 0] <= n and all(0 <= k < n for k in keep) and len(set(keep)) == len(keep), (levels, K, b)
            single = DC.NMS(od[b], 0.4)
            ref = P.nms_stable(want, 0.4)
            print('levels %d K %d frame %d: %d rows, %d kept (single %d, restatement %d)' % (levels, K, b, n, len(keep), len(single), len(ref)))
            assert keep == single, (levels, K, b, 'dbx_nms')
            assert keep == ref, (levels, K, b, 'nms_stable')
    assert paths == {'greedy', 'matrix', 'global'}


def test_merge_kernel_other_thresholds_and_a_second_call():
    rs = np.random.RandomState(77)
    frames = [[P.random_frame(rs, 100, 13, span=400.0, quantise=16) for _ in range(3)] for _ in range(4)]
    level_np = [np.stack([f[l] for f in frames]) for l in range(3)]
    xf = [[XFORMS[l]] * 4 for l in range(3)]
    for th in (0.0, 0.4, 0.7):
        od, ok = _merge_abi(level_np, xf, th)
        od2, ok2 = _merge_abi(level_np, xf, th)
        for b in range(4):
            keep = _keep_list(ok[b])
            assert keep == P.nms_stable(od[b], th) == DC.NMS(od[b], th), (th, b)
            assert _same(od[b], od2[b]) and keep == _keep_list(ok2[b])           # no order dependence between calls
        assert len({len(_keep_list(k)) for k in ok}) > 1 or th == 0.0


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


def _composition(net, frames, sizes, K=10, th=0.4):
    """What a user composes from the single-size call: detect_batch_resized per size, a host concatenate, decode.NMS per frame."""
    per = [net.detect_batch_resized(frames, size=s, K=K, nms_thresh=th) for s in sizes]
    out = []
    for i in range(len(per[0])):
        d = np.concatenate([per[l][i][0] for l in range(len(sizes))], axis=0)
        out.append((d, DC.NMS(d, th)))
    return out


def _assert_results(got, want, what):
    assert len(got) == len(want), what
    for i, ((dg, kg), (dw, kw)) in enumerate(zip(got, want)):
        assert dg.dtype == np.float64 and _same(dg, dw), (what, i, 'rows')
        assert kg == kw, (what, i, 'keep')


@pytest.mark.parametrize('dtype', ['f32', 'f16'])
@pytest.mark.parametrize('kind', KINDS)
def test_detect_pyramid_is_the_composition_bit_for_bit(kind, dtype):
    net = _net(kind, dtype)
    rs = np.random.RandomState(31)
    frames = [_img(rs, h, w) for h, w in MIXED]
    want = _composition(net, frames, SIZES)
    got = net.detect_pyramid(frames, sizes=SIZES, K=10)
    _assert_results(got, want, 'numpy list')
    dc = 5 if kind == 'DenseBox' else 13
    assert all(d.shape == (30, dc) for d, _ in got) and sum(len(k) for _, k in got) > 0
    _assert_results(net.detect_pyramid(frames, sizes=SIZES, K=10), want, 'replay')
    _assert_results(DC.detect_pyramid(net, [torch.from_numpy(f) for f in frames], sizes=SIZES), want, 'CPU tensors')
    _assert_results(net.detect_pyramid([torch.from_numpy(f).cuda() for f in frames], sizes=SIZES), want, 'CUDA tensors')
    # one level: detect_batch_resized's rows (its keep lists are NOT compared: they come from an NMS in resized-frame geometry, and
    # the +1 pixel convention of the IoU is not scale invariant)
    one = net.detect_pyramid(frames, sizes=(240,), K=10)
    for (d, keep), (d0, _) in zip(one, net.detect_batch_resized(frames, size=240, K=10)):
        assert _same(d, d0) and keep == DC.NMS(d0, 0.4)
    # a [B,H,W,3] tensor, on the host and on the device
    batch = np.stack([_img(rs, 120, 200) for _ in range(3)])
    want_b = _composition(net, torch.from_numpy(batch), SIZES)
    _assert_results(net.detect_pyramid(torch.from_numpy(batch), sizes=SIZES), want_b, 'CPU batch tensor')
    _assert_results(net.detect_pyramid(torch.from_numpy(batch).cuda(), sizes=SIZES), want_b, 'CUDA batch tensor')
    _assert_results(net.detect_pyramid(list(batch), sizes=SIZES), want_b, 'the same frames as a list')


def _graphs(net):
    return {k: id(v[1]) for k, v in net.__dict__.get('_detect_graphs', {}).items()}


def test_chunking_graph_cache_and_the_other_entries():
    """f32: the chunk size changes the batch of every forward, and only the fp32 forward is bit for bit independent of its batch (the
    16-bit kernels pick their tiling by problem size; tests/test_hip_resize_batch.py compares chunk sizes in f32 for the same reason)."""
    net = _net('DenseBoxLMLOC', 'f32')
    rs = np.random.RandomState(32)
    frames = [_img(rs, *MIXED[i % 5]) for i in range(7)]
    x1 = synth.synth_images(1, 240, 240, seed=3).cuda()
    x4 = synth.synth_images(4, 240, 240, seed=4).cuda()
    d_before = net.detect(x1, K=10)
    b_before = net.detect_batch(x4, K=10)
    whole = net.detect_pyramid(frames, sizes=SIZES, K=10, max_batch=32)
    assert len(net.__dict__['_detect_graphs']) <= DC._MAX_GRAPHS
    chunked = net.detect_pyramid(frames, sizes=SIZES, K=10, max_batch=3)           # chunks of 3, 3, 1
    _assert_results(chunked, whole, 'max_batch 3 against 32')
    cache = net.__dict__['_detect_graphs']
    assert len(cache) <= DC._MAX_GRAPHS
    level_keys = [k for k in cache if k[0] == 'level']
    assert {k[1] for k in level_keys} >= {(b, s, s, 3) for b in (3, 1) for s in SIZES}, list(cache)
    snap = _graphs(net)
    _assert_results(net.detect_pyramid(frames, sizes=SIZES, K=10, max_batch=3), whole, 'second identical call')
    assert _graphs(net) == snap, 'the second identical call captured a graph'
    # the cache is one LRU over all tags: detect()'s and detect_batch()'s entries may have been evicted and are re-captured; what
    # they return may not change
    d_after = net.detect(x1, K=10)
    assert _same(d_after[0], d_before[0]) and d_after[1] == d_before[1]
    _assert_results(net.detect_batch(x4, K=10), b_before, 'detect_batch after the pyramid calls')
    assert len(net.__dict__['_detect_graphs']) <= DC._MAX_GRAPHS
    _assert_results(net.detect_pyramid(frames, sizes=SIZES, K=10, max_batch=3), whole, 'after detect() / detect_batch()')
    d_again = net.detect(x1, K=10)
    assert _same(d_again[0], d_before[0]) and d_again[1] == d_before[1]
    # four levels with a tail chunk: eight level shapes, the whole cache
    four = net.detect_pyramid(frames[:4], sizes=(96, 160, 240, 320), K=10, max_batch=3)
    assert len(net.__dict__['_detect_graphs']) <= DC._MAX_GRAPHS
    _assert_results(four, _composition(net, frames[:4], (96, 160, 240, 320)), 'four levels')


def test_one_resize_launch_per_call_and_one_merge_launch_per_chunk(monkeypatch):
    net = _net('DenseBoxLM', 'f16')
    rs = np.random.RandomState(33)
    frames = [_img(rs, *MIXED[i % 5]) for i in range(7)]
    L = _lib.lib()
    calls = {'dbx_resize_cubic_batch_u8': [], 'dbx_merge_nms_batch': [], 'dbx_nms': [], 'dbx_detect_batch': []}

    def wrap(name):
        real = getattr(L, name)

        def f(*a):
            calls[name].append(a)
            return real(*a)
        monkeypatch.setattr(L, name, f)
    for name in calls:
        wrap(name)
    for max_batch, chunks in ((32, 1), (3, 3), (7, 1), (4, 2)):
        for rep in range(2):                                 # the capturing call warms up through more decode launches; the replay is bare
            for v in calls.values():
                del v[:]
            res = net.detect_pyramid(frames, sizes=SIZES, K=10, max_batch=max_batch)
            assert len(res) == 7
            assert len(calls['dbx_resize_cubic_batch_u8']) == 1, (max_batch, rep)
            assert calls['dbx_resize_cubic_batch_u8'][0][1] == 7 * len(SIZES)          # B * L jobs
            assert len(calls['dbx_merge_nms_batch']) == chunks, (max_batch, rep)
            assert [c[3] for c in calls['dbx_merge_nms_batch']] == [min(max_batch, 7 - i) for i in range(0, 7, max_batch)]
            assert len(calls['dbx_nms']) == 0
        assert len(calls['dbx_detect_batch']) == 0, 'a replay launches the decode from the graph, not through the binding'
    with monkeypatch.context() as m:
        m.setenv('DBX_GRAPH', '0')
        for v in calls.values():
            del v[:]
        net.detect_pyramid(frames, sizes=SIZES, K=10, max_batch=3)
        assert (len(calls['dbx_resize_cubic_batch_u8']), len(calls['dbx_merge_nms_batch']), len(calls['dbx_nms'])) == (1, 3, 0)
        assert len(calls['dbx_detect_batch']) == 3 * len(SIZES)                          # one per level per chunk


def test_eager_and_graph_replay_agree(monkeypatch):
    rs = np.random.RandomState(34)
    frames = [_img(rs, *MIXED[i % 5]) for i in range(5)]
    for kind in KINDS:
        net = _net(kind, 'f16')
        with monkeypatch.context() as m:
            m.setenv('DBX_GRAPH', '0')
            eager = net.detect_pyramid(frames, sizes=SIZES, K=10, max_batch=2)
            assert not [k for k in net.__dict__.get('_detect_graphs', {}) if k[0] == 'level']
        _assert_results(net.detect_pyramid(frames, sizes=SIZES, K=10, max_batch=2), eager, kind + ' capture')
        _assert_results(net.detect_pyramid(frames, sizes=SIZES, K=10, max_batch=2), eager, kind + ' replay')
    # train mode runs the same launches eagerly (its forward draws dropout masks, so only the structure is checked)
    net = _net('DenseBoxLMLOC', 'f16')
    net.train()
    res = net.detect_pyramid(frames, sizes=SIZES, K=10)
    assert not net.__dict__.get('_detect_graphs')
    for d, keep in res:
        assert d.shape == (30, 13) and keep == DC.NMS(d, 0.4)
