"""The top-K decode order of detect_kernel on each of its five selection paths, on both sides of every map size at which the path
switches: larger score first, lower index on ties, -0 == +0, -inf above NaN, NaN below every number (lower index first among NaN),
every index at most once.  dbx_detect / dbx_detect_batch against plain NumPy -- indices equal, rows bit for bit -- on crafted maps:
ties cut by index, constant maps, signed zeros, maxima on bucket and thread-lane edges, -inf blocks, +inf ties and NaN.

    path 1  register tournament                      K <= 48 and n <= 16384
    path 2  radix select + bitonic sort              49 <= K <= 1024, any n
    path 3  arg-max rounds, working copy in LDS      K > 1024 and n <= 16384
    path 4  arg-max rounds, working copy in scratch  (K <= 48 or K > 1024) and 16384 < n <= 262144
    path 5  arg-max rounds, flat per-thread rescan   (K <= 48 or K > 1024) and n > 262144
"""
import functools

import numpy as np
import pytest
import torch

from densebox_amd import _lib, decode as DC
from densebox_amd._lib import check, ptr, stream_ptr

pytestmark = pytest.mark.gpu

GUARD = 512                     # sentinel bytes behind every output and the scratch
BK, THREADS = 64, 1024          # the kernel's bucket of consecutive scores; its threads (thread t owns the indices t mod 1024)
SMALL = [(128, 128), (129, 128), (131, 127)]     # last LDS / tournament size; first global-scratch size; a ragged last bucket on path 4
LARGE = [(512, 512), (513, 512)]                 # last two-level size; first flat-rescan size
KS_SMALL = (1, 10, 48, 49, 1024, 1025, 1500)
KS_LARGE = (10, 48, 1025)
CONTENTS = ('random', 'quantised', 'constant', 'signed_zero', 'bucket_edges', 'neg_inf_0', 'neg_inf_1', 'neg_inf_km1', 'pos_inf', 'nan',
            'nan_few', 'all_nan')
NINF = np.float32(-np.inf)


def path_of(K, n):
    """the selection path detect_kernel takes for K detections on a map of n scores"""
    if 49 <= K <= 1024:
        return 2
    if n <= 16 * THREADS:
        return 1 if K <= 48 else 3
    return 4 if (n + BK - 1) // BK <= 4096 else 5


def _cases():
    out = []
    for sizes, ks in ((SMALL, KS_SMALL), (LARGE, KS_LARGE)):
        for rows, cols in sizes:
            for K in ks:
                for content in CONTENTS:
                    if K == 1 and content in ('neg_inf_1', 'neg_inf_km1'):
                        continue                                    # m = min(1, K - 1) = K - 1 = 0: the neg_inf_0 case
                    out.append((rows, cols, K, content))
    return out


CASES = _cases()


def _seed(rows, cols, content):
    return 1000 * CONTENTS.index(content) + rows + cols


def _edge_indices(n):
    """indices on the edges of the kernel's structures: the map's first and last score, lane 0 and lane 63 of a bucket, two buckets
    of one thread's share of the bucket maxima (1024 buckets apart where the map has that many), the same thread lane twice (1024
    apart) and a neighbouring lane; the last one lies in the last (possibly ragged) bucket"""
    nb = (n + BK - 1) // BK
    b2 = 5 + THREADS if nb > 5 + THREADS else 11
    idx = [0, n - 1, BK * 3, BK * 7 + 63, BK * 5 + 9, BK * b2 + 9, 5 * THREADS + 7, 9 * THREADS + 7, 3 * THREADS + 8, BK * (nb - 1)]
    assert len(set(idx)) == len(idx) and max(idx) < n
    return np.array(sorted(idx))


def make_score(rows, cols, K, content):
    n = rows * cols
    rs = np.random.RandomState(_seed(rows, cols, content))
    if content == 'random':
        sc = ((rs.permutation(n) - n // 2).astype(np.float32) * np.float32(1.0 / 1024)) ** 3      # n distinct values of both signs
        # (not randn: 262656 fp32 draws of it repeat values, and 'no ties' is this content's premise; check_premise asserts it)
    elif content == 'quantised':
        sc = (rs.randint(0, 7, size=n) / 4.0).astype(np.float32)
    elif content == 'constant':
        sc = np.full(n, 0.25, np.float32)
    elif content == 'signed_zero':
        sc = np.where(rs.rand(n) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        sc[rs.randint(2, n, 30)] = -1.0
        sc[0], sc[1] = -0.0, 0.0
    elif content == 'bucket_edges':
        sc = (rs.rand(n) * 0.5).astype(np.float32)
        e = _edge_indices(n)
        sc[e] = 2.0                                                # the maximum, ten times
        sc[np.minimum(e + 1, n - 2)] = 1.5                         # the runner-up right behind each (lane 1, the next bucket's lane 0, ...)
    elif content.startswith('neg_inf'):
        m = {'neg_inf_0': 0, 'neg_inf_1': min(1, K - 1), 'neg_inf_km1': K - 1}[content]
        sc = np.full(n, NINF, np.float32)
        at = rs.choice(np.arange(BK, n), m, replace=False)         # bucket 0 is all -inf: the rounds walk over retired scores
        sc[at] = rs.randn(m).astype(np.float32)
    elif content == 'pos_inf':
        sc = rs.randn(n).astype(np.float32)
        sc[[BK * 2, BK * 2 + 63, THREADS + 5, 2 * THREADS + 5, n - 1]] = np.inf
    elif content == 'nan':
        sc = rs.randn(n).astype(np.float32)
        sc[rs.rand(n) < 0.32] = np.nan
        sc[0] = np.nan
        sc[BK * np.array([1, 2, 5, 100, 255, (n - 1) // BK])] = np.nan            # lane 0 of several buckets, the last one included
        sc[BK * 9:BK * 10] = np.nan                                # a whole bucket
        sc[np.arange(0, n, THREADS)[::3]] = np.nan                 # the first score thread 0 reads in every third stride
    elif content == 'nan_few':
        f = K // 2                                                 # fewer numbers than K: K - f NaN rows must come out
        sc = np.full(n, np.nan, np.float32)
        sc[rs.choice(n, f, replace=False)] = rs.randn(f).astype(np.float32)
    elif content == 'all_nan':
        sc = np.full(n, np.nan, np.float32)
    else:
        raise AssertionError(content)
    return sc


def reference_order(sc):
    """score descending, index ascending on ties; NaN last, lower index first, -inf just above (= the descending order of the
    kernel's (det_key << 32 | ~index) composites)"""
    return np.lexsort((np.arange(sc.size), -sc.astype(np.float64)))


def check_premise(sc, order, K, content):
    """what the case is for, asserted from the reference alone"""
    n, top = sc.size, sc[order[:K]]
    assert n > K
    if content == 'random':
        assert np.unique(sc).size == n                                                  # no ties at all
    elif content in ('quantised', 'constant'):
        kth = top[-1]
        assert (sc == kth).sum() > K - (sc > kth).sum()                                 # more copies of the K-th value than places
        assert content == 'quantised' or np.array_equal(order[:K], np.arange(K))
    elif content == 'signed_zero':
        assert (top == 0).all() and (sc == 0).sum() > K                                 # cut inside the zeros
        assert K == 1 or (np.signbit(top).any() and not np.signbit(top).all())          # both signs among the K
        assert np.array_equal(order[:K], np.nonzero(sc == 0)[0][:K])                    # ... ranked by index alone
    elif content == 'bucket_edges':
        e = _edge_indices(n)
        assert np.array_equal(np.nonzero(sc == 2.0)[0], e)
        assert np.array_equal(order[:min(K, e.size)], e[:K])
        assert e[0] % BK == 0 and (e % BK == 63).any() and e[-1] == n - 1 and len(set(e // BK)) >= 8
        lanes = e % THREADS
        assert np.unique(lanes).size < lanes.size                                       # two maxima in one thread lane
    elif content.startswith('neg_inf'):
        m = int((sc > NINF).sum())
        assert m in (0, min(1, K - 1), K - 1) and m < K
        assert np.isneginf(top[m:]).all() and np.array_equal(order[m:K], np.nonzero(np.isneginf(sc))[0][:K - m])
    elif content == 'pos_inf':
        p = np.nonzero(np.isposinf(sc))[0]
        assert p.size == 5 and np.array_equal(order[:min(K, 5)], p[:K])
    elif content == 'nan':
        nan = np.isnan(sc)
        assert 0.3 * n < nan.sum() < 0.4 * n and n - nan.sum() > K and not np.isnan(top).any()
        assert nan[0] and nan[::BK].sum() >= 6 and nan.reshape(-1)[BK * 9:BK * 10].all() and nan[::THREADS].sum() >= 2
    elif content == 'nan_few':
        f = int((~np.isnan(sc)).sum())
        assert f == K // 2 < K
        assert np.isnan(top[f:]).all() and np.array_equal(order[f:K], np.nonzero(np.isnan(sc))[0][:K - f])
    elif content == 'all_nan':
        assert np.isnan(sc).all() and np.array_equal(order[:K], np.arange(K))


@functools.lru_cache(maxsize=None)
def _loc(rows, cols):
    """(host [4, n], device [1, 4, rows, cols]) box offsets of a map size, made once"""
    rs = np.random.RandomState(7 * rows + cols)
    loc = (rs.randn(4, rows * cols) * 8).astype(np.float32)
    loc.setflags(write=False)
    return loc, torch.from_numpy(loc).view(1, 4, rows, cols).cuda()


@functools.lru_cache(maxsize=None)
def _lm_loc(rows, cols):
    rs = np.random.RandomState(11 * rows + cols)
    lm = (rs.randn(8, rows * cols) * 8).astype(np.float32)
    lm.setflags(write=False)
    return lm, torch.from_numpy(lm).view(1, 8, rows, cols).cuda()


def expected_rows(sc, loc, idx, cols, lm_loc=None, lm_arg=None):
    """det_write_row in NumPy: fp32 subtraction, then * 4.0 in float64"""
    xi, yi = (idx % cols).astype(np.float32), (idx // cols).astype(np.float32)
    d = np.empty((idx.size, 5 if lm_loc is None and lm_arg is None else 13), np.float64)
    for c in range(4):
        d[:, c] = ((yi if c & 1 else xi) - loc[c, idx]).astype(np.float32).astype(np.float64) * 4.0
    d[:, 4] = sc[idx].astype(np.float64)
    if lm_loc is not None:
        for c in range(8):
            d[:, 5 + c] = ((yi if c & 1 else xi) - lm_loc[c, idx]).astype(np.float32).astype(np.float64) * 4.0
    elif lm_arg is not None:
        for j in range(4):
            d[:, 5 + 2 * j] = np.float64(np.float32(lm_arg[j] % cols)) * 4.0
            d[:, 6 + 2 * j] = np.float64(np.float32(lm_arg[j] // cols)) * 4.0
    return d


def _banded(nbytes):
    buf = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    return buf, buf[:nbytes]


def run_detect(score, loc, K, lm_heat=None, lm_loc=None, nms=0.4, batched=False):
    """dbx_detect (or dbx_detect_batch) on device maps [B, C, rows, cols] with a sentinel band behind dets, topk, keep and the
    scratch; per image (dets [K, dc], topk [K], keep list) after the bands were found untouched"""
    B, _, rows, cols = score.shape
    assert batched or B == 1
    dc = 5 if lm_heat is None and lm_loc is None else 13
    L = _lib.lib()
    g_d, dets = _banded(B * K * dc * 8)
    g_t, topk = _banded(B * K * 8)
    g_k, keep = _banded(B * (K + 1) * 4)
    if batched:
        g_s, scratch = _banded(L.dbx_detect_batch_scratch_bytes(B, rows, cols, K))
        check(L.dbx_detect_batch(ptr(score), ptr(loc), ptr(lm_heat), ptr(lm_loc), B, rows, cols, K, nms, ptr(dets), dc, ptr(topk),
                                 ptr(keep), ptr(scratch), stream_ptr()))
    else:
        g_s, scratch = _banded(L.dbx_detect_scratch_bytes(rows, cols, K))
        check(L.dbx_detect(ptr(score), ptr(loc), ptr(lm_heat), ptr(lm_loc), rows, cols, K, nms, ptr(dets), dc, ptr(topk), ptr(keep),
                           ptr(scratch), stream_ptr()))
    torch.cuda.synchronize()
    for name, g in (('dets', g_d), ('topk', g_t), ('keep', g_k), ('scratch', g_s)):
        assert bool((g[-GUARD:] == 0xA5).all()), 'the band behind %s was written' % name
    d = dets.cpu().numpy().view(np.float64).reshape(B, K, dc)
    t = topk.cpu().numpy().view(np.int64).reshape(B, K)
    k = keep.cpu().numpy().view(np.int32).reshape(B, K + 1)
    out = []
    for b in range(B):
        assert 0 <= k[b, 0] <= K
        out.append((d[b], t[b], [int(v) for v in k[b, 1:1 + int(k[b, 0])]]))
    return out


def assert_selection(got_d, got_t, sc, loc, order, K, cols, tag, lm_loc=None, lm_arg=None):
    want = order[:K]
    assert np.array_equal(got_t, want), (tag, 'indices', np.nonzero(got_t != want)[0][:5], got_t[:8], want[:8])
    assert np.unique(got_t).size == K, (tag, 'an index came out twice')
    exp = expected_rows(sc, loc, want, cols, lm_loc, lm_arg)
    assert got_d.shape == exp.shape
    same = got_d.view(np.uint64) == exp.view(np.uint64)
    assert same.all(), (tag, 'rows', np.argwhere(~same)[:5])


def _dev(a, c, rows, cols):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).view(1, c, rows, cols).cuda()


def test_every_content_reaches_every_path():
    """the grid below puts every score content on each of the five paths, on both sides of every switch"""
    for content in CONTENTS:
        seen = {path_of(K, r * c) for r, c, K, ct in CASES if ct == content}
        assert seen == {1, 2, 3, 4, 5}, (content, seen)
    by_size = {(r, c): {path_of(K, r * c) for r2, c2, K, _ in CASES if (r2, c2) == (r, c)} for r, c in SMALL + LARGE}
    assert by_size[(128, 128)] == {1, 2, 3} and by_size[(129, 128)] == {2, 4} and by_size[(131, 127)] == {2, 4}
    assert by_size[(512, 512)] == {4} and by_size[(513, 512)] == {5}
    assert 131 * 127 % BK != 0 and 128 * 128 == 16 * THREADS and 512 * 512 == 4096 * BK
    assert path_of(48, 16384) == 1 and path_of(48, 16385) == 4 and path_of(1025, 16384) == 3 and path_of(1025, 16385) == 4
    assert path_of(10, 262144) == 4 and path_of(10, 262145) == 5 and path_of(49, 262656) == 2 and path_of(1024, 16384) == 2


@pytest.mark.parametrize('rows,cols,K,content', CASES, ids=['%dx%d-K%d-%s' % c for c in CASES])
def test_topk_order_and_rows(rows, cols, K, content):
    n = rows * cols
    sc = make_score(rows, cols, K, content)
    order = reference_order(sc)
    check_premise(sc, order, K, content)
    loc, loc_d = _loc(rows, cols)
    [(d, t, _)] = run_detect(_dev(sc, 1, rows, cols), loc_d, K)
    assert_selection(d, t, sc, loc, order, K, cols, ('path', path_of(K, n), content))


LM_CASES = [(128, 128, 10), (128, 128, 1024), (128, 128, 1025), (131, 127, 48), (131, 127, 1500), (513, 512, 10)]


@pytest.mark.parametrize('rows,cols,K', LM_CASES)
@pytest.mark.parametrize('content', ['quantised', 'nan_few'])
def test_thirteen_column_rows_from_offsets(rows, cols, K, content):
    """det_cols = 13 with parse_DetLMLOC's eight offset columns, on every path"""
    assert {path_of(k, r * c) for r, c, k in LM_CASES} == {1, 2, 3, 4, 5}
    sc = make_score(rows, cols, K, content)
    order = reference_order(sc)
    check_premise(sc, order, K, content)
    (loc, loc_d), (lm, lm_d) = _loc(rows, cols), _lm_loc(rows, cols)
    heat = torch.zeros((1, 4, rows, cols), dtype=torch.float32, device='cuda')
    [(d, t, _)] = run_detect(_dev(sc, 1, rows, cols), loc_d, K, lm_heat=heat, lm_loc=lm_d)
    assert_selection(d, t, sc, loc, order, K, cols, ('path', path_of(K, rows * cols), content), lm_loc=lm)


BATCH_CONTENTS = ('quantised', 'neg_inf_1', 'nan')


@pytest.mark.parametrize('K', [10, 1025])
def test_batch_images_have_their_own_scratch_slice(K):
    """three different images in one dbx_detect_batch launch on the first global-scratch size: each equals its own NumPy reference
    and its own dbx_detect run bit for bit, keep list included; nothing is written behind dets, topk, keep or the scratch"""
    rows, cols = 129, 128
    assert path_of(K, rows * cols) == 4
    scs = [make_score(rows, cols, K, c) for c in BATCH_CONTENTS]
    loc, loc_d = _loc(rows, cols)
    locs = [np.roll(loc, 17 * b, axis=1) for b in range(3)]                        # a different box per image at every pixel
    s_d = torch.cat([_dev(s, 1, rows, cols) for s in scs])
    l_d = torch.cat([_dev(l, 4, rows, cols) for l in locs])
    got = run_detect(s_d, l_d, K, batched=True)
    for b, content in enumerate(BATCH_CONTENTS):
        order = reference_order(scs[b])
        check_premise(scs[b], order, K, content)
        d, t, k = got[b]
        assert_selection(d, t, scs[b], locs[b], order, K, cols, ('batch', b, content))
        [(d1, t1, k1)] = run_detect(s_d[b:b + 1], l_d[b:b + 1], K)
        assert np.array_equal(t, t1) and d.tobytes() == d1.tobytes() and k == k1, ('batch against single', b, content)


def _heat(rows, cols):
    """four finite heat maps whose maximum is repeated: in one thread lane (1024 apart), at a later index of an earlier lane, on the
    last score; a constant map; a +0 / -0 maximum"""
    n = rows * cols
    rs = np.random.RandomState(rows + 3 * cols)
    h = (rs.rand(4, n) * 0.5).astype(np.float32)
    h[0, [5 * THREADS + 700, 6 * THREADS + 700, 7 * THREADS + 3, n - 1]] = 1.0
    h[1] = 0.125
    h[2, [n - 1 - THREADS, n - 1]] = 3.0
    h[3] = -h[3] - 0.25
    h[3, [2 * THREADS + 50, 2 * THREADS + 100, BK * ((n - 1) // BK)]] = [0.0, -0.0, 0.0]
    return h


@pytest.mark.parametrize('rows,cols', [(129, 128), (513, 512)])
def test_landmark_argmax_takes_the_first_maximum(rows, cols):
    """parse_DetLM: the four shared landmark columns are np.argmax (first occurrence) of each heat map"""
    n, K = rows * cols, 10
    h = _heat(rows, cols)
    assert np.isfinite(h).all()
    arg = [int(np.argmax(h[j])) for j in range(4)]
    assert all((h[j] == h[j, arg[j]]).sum() >= 2 for j in range(4))                # every maximum is repeated
    assert arg == [5 * THREADS + 700, 0, n - 1 - THREADS, 2 * THREADS + 50]
    sc = make_score(rows, cols, K, 'random')
    order = reference_order(sc)
    loc, loc_d = _loc(rows, cols)
    [(d, t, _)] = run_detect(_dev(sc, 1, rows, cols), loc_d, K, lm_heat=_dev(h, 4, rows, cols))
    assert_selection(d, t, sc, loc, order, K, cols, ('heat', rows, cols), lm_arg=arg)


NMS_CASES = [(128, 128, 10), (128, 128, 49), (128, 128, 1025), (131, 127, 48), (129, 128, 1025), (513, 512, 10), (513, 512, 1025)]


def _cluster_maps(rows, cols, K):
    """random scores whose best pixels sit in 2 x 2 clusters, cluster c outranking cluster c + 1, and boxes of five cells"""
    n = rows * cols
    rs = np.random.RandomState(rows * 5 + cols + K)
    sc = rs.rand(n).astype(np.float32)
    ys, xs = np.meshgrid(np.arange(3, rows - 4, 7), np.arange(3, cols - 4, 7), indexing='ij')
    centres = np.stack([ys.reshape(-1), xs.reshape(-1)], 1)
    rs.shuffle(centres)
    need = (K + 3) // 4 + 1
    assert need <= len(centres)
    for c, (y, x) in enumerate(centres[:need]):
        for j, p in enumerate(rs.permutation(4)):                                  # four distinct scores per cluster
            sc[(y + p // 2) * cols + x + p % 2] = np.float32(10 + 2 * (need - c) + 0.25 * j + 0.1 * rs.rand())
    half = (2.5 + rs.rand(4, n) * 0.2).astype(np.float32)
    return sc, np.stack([half[0], half[1], -half[2], -half[3]])                    # box = pixel -+ 2.5 cells


@pytest.mark.parametrize('rows,cols,K', NMS_CASES)
def test_keep_list_on_overlapping_boxes(rows, cols, K):
    """the neighbours of a cluster suppress each other, the clusters do not: keep == decode.NMS of the reference rows"""
    assert {path_of(k, r * c) for r, c, k in NMS_CASES} == {1, 2, 3, 4, 5}
    n = rows * cols
    sc, loc = _cluster_maps(rows, cols, K)
    order = reference_order(sc)
    assert np.unique(sc[order[:K + 1]]).size == K + 1
    [(d, t, keep)] = run_detect(_dev(sc, 1, rows, cols), _dev(loc, 4, rows, cols), K)
    assert_selection(d, t, sc, loc, order, K, cols, ('nms', path_of(K, n)))
    want = DC.NMS(expected_rows(sc, loc, order[:K], cols))
    assert 1 < len(want) < K                                                       # some rows are kept, some suppressed
    assert keep == want
