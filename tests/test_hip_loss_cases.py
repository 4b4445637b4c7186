"""The fused loss (csrc/loss.hip: loss_kernel, loss_apply_kernel, loss_finish_kernel) on edge geometry, ties and large batches, against
oracle/densebox_oracle.py::loss_step on the same inputs.  tests/loss_cases.py holds the tables and the references, tests/test_loss_cases.py
their premises (asserted on the CPU from the reference alone).

Every case asserts: neg_idx, lm_neg_idx, mask_cls, mask_lm and pos_count bit-exact; every gradient exactly 0 wherever its mask is 0;
elsewhere |got - ref| <= 1e-5 |ref| + 1e-5 max|ref| with the maximum taken per patch and tensor (one far-outside box must not loosen
the others); the loss within 2**-22 relative of loss64 -- the float64 sum of the float32 terms m * (d * d): the kernel rounds a double sum
of non-negative terms to float32 once, 2**-24; the rest is margin for reassociation and for the lambdas, which the kernel holds in float32.
The hard-negative lists are the documented rule (loss descending, lower index first on equal losses: loss_cases.tie_order) and are handed
to loss_step as hard_neg / lm_hard_neg, since torch.topk leaves the order of equal losses open; where the inputs have no ties the oracle's
own top-k is asserted to be the same list.

Sensitivity.  Six in-bounds mutants of loss.hip, each run once against this file: a negative start clamped to 0 instead of wrapped (30
tests fail), `ey + 1` read as `ey` (40), block_argmax preferring the higher index on equal losses (8: every tie case and K = 3600), the
tournament doing so (6), the finish kernel dropping the last patch of a full group of 256 (4: every n >= 256), the landmark zero-block
losing its last row (1; the random landmark negatives now visit every cell of the 5 x 5 block).

Cost on an MI355X host (16 threads), oracle runs included: the 35 tests of this file took 5.3 s in all; the slowest five:
batch sizes DenseBoxLMLOC-257 0.60 s, DenseBox-513 0.34 s, geometry DenseBox 0.31 s (the first launch of the process), batch sizes
DenseBox-255 0.17 s, DenseBox-256 0.16 s.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_cases as L                                  # noqa: E402
import densebox_amd.labels as LB                        # noqa: E402
from densebox_amd import _lib                           # noqa: E402
from densebox_amd.loss import densebox_loss             # noqa: E402
from oracle import densebox_oracle as O                 # noqa: E402

pytestmark = pytest.mark.gpu
T = torch.from_numpy
NAMES = {'DenseBox': ('score', 'loc'), 'DenseBoxLM': ('score', 'loc', 'lm', 'rf'), 'DenseBoxLMLOC': ('score', 'rf', 'loc', 'lm', 'lmloc')}


def half_of(kind, bbox, lab, n, batch_global=None, positive_num_global=None, **_):
    P = int(O.init_score_map(bbox, lab if kind == 'DenseBoxLMLOC' else None).sum()) if positive_num_global is None else positive_num_global
    return O.neg_counts(P, n if batch_global is None else batch_global)[1]


def run_gpu(kind, outs, bbox, vert, lab, rand_neg, lm_rand, debug=True, **kw):
    """One launch; everything read back as NumPy: loss (float32 scalar), grads by name, and with ``debug`` the masks and index lists."""
    dev = [T(o).cuda().requires_grad_(True) for o in outs]
    r = densebox_loss(kind, tuple(dev), bbox, vert, lab, rand_neg_indices=rand_neg, lm_rand_neg_indices=lm_rand, return_debug=debug, **kw)
    loss, dbg = r if debug else (r, {})
    got = {k: v.cpu().numpy() for k, v in dbg.items() if torch.is_tensor(v)}
    got['half'] = dbg.get('half')
    got['loss'] = loss.detach().cpu().numpy().reshape(()).astype(np.float32)
    tensors, grads = loss._dbx_direct                                       # dL/d(out) as written, in the order score, loc, lm, rf, lmloc
    order = [k for k in ('score', 'loc', 'lm', 'rf', 'lmloc') if k in NAMES[kind]]
    assert all(t is dev[NAMES[kind].index(k)] for k, t in zip(order, tensors))
    got['grads'] = {k: g.cpu().numpy() for k, g in zip(order, grads)}
    return got


def run_oracle(kind, outs, bbox, vert, lab, rand_neg, lm_rand, ties=False, **kw):
    half = half_of(kind, bbox, lab, outs[0].shape[0], **kw)
    hard, lm_hard = L.hard_lists(kind, outs, bbox, vert, lab, half)
    leaf = [T(o).clone().requires_grad_(True) for o in outs]
    res = O.loss_step(kind, tuple(leaf), bbox, vert, lab, rand_neg=rand_neg, lm_rand_neg=lm_rand, hard_neg=hard, lm_hard_neg=lm_hard, **kw)
    assert res['half'] == half
    if not ties:                                   # no ties above the cut: the reference's own top-k is the rule's list
        assert np.array_equal(res['hard_own'], hard)
        assert kind == 'DenseBox' or np.array_equal(res['lm_hard_own'], lm_hard)
    res['loss'].backward()
    res['grads'] = {k: (l.grad.numpy() if l.grad is not None else np.zeros(l.shape, np.float32)) for k, l in zip(NAMES[kind], leaf)}
    lam = {k: kw[k] for k in ('lambda_loc', 'lambda_det', 'lambda_lm') if k in kw}
    res['loss64'] = L.loss64(res, outs, kind, **lam)
    return res


def assert_grad(name, got, ref, mask):
    mask = np.broadcast_to(mask, ref.shape)
    assert not got[mask == 0].any(), '%s: gradient outside its mask' % name
    amax = np.abs(ref).reshape(ref.shape[0], -1).max(axis=1).reshape(-1, 1, 1, 1)
    bad = np.abs(got - ref) > 1e-5 * np.abs(ref) + 1e-5 * amax
    assert not bad.any(), (name, np.argwhere(bad)[:4].tolist(), float(np.abs(got - ref).max()))


def assert_loss(got, ref64):
    print('loss %.9g  loss64 %.17g  rel %.3g' % (float(got), ref64, abs(float(got) - ref64) / max(ref64, 1e-300)))
    assert abs(float(got) - ref64) <= L.TOL_LOSS * ref64


def compare(kind, got, res):
    assert got['half'] == res['half']
    assert got['neg_idx'].dtype == np.int64 and np.array_equal(got['neg_idx'], res['neg_idx'])
    assert np.array_equal(got['mask_cls'], res['mask'])
    assert np.array_equal(got['pos_count'], res['gt'].sum(axis=(1, 2, 3)).astype(np.int32))
    if kind != 'DenseBox':
        assert np.array_equal(got['lm_neg_idx'], res['lm_neg_idx'])
        assert np.array_equal(got['mask_lm'], res['lm_mask'])
    gm = L.grad_masks(kind, res)
    for k in NAMES[kind]:
        assert_grad(k, got['grads'][k], res['grads'][k], gm[k])
    assert_loss(got['loss'], res['loss64'])


def check(kind, outs, bbox, vert, lab, rand_neg, lm_rand, ties=False, **kw):
    res = run_oracle(kind, outs, bbox, vert, lab, rand_neg, lm_rand, ties=ties, **kw)
    got = run_gpu(kind, outs, bbox, vert, lab, rand_neg, lm_rand, **kw)
    compare(kind, got, res)
    return got, res


def draws(kind, bbox, lab, n, seed, **kw):
    rs = np.random.RandomState(seed)
    return L.draw_rand_neg(rs, n, half_of(kind, bbox, lab, n, **kw)), L.draw_lm_rand_neg(rs, n)


# ------------------------------------------------------------------------------------------------ 1. geometry x kind
@pytest.mark.parametrize('kind', L.KINDS)
def test_geometry_table_by_kind(kind):
    """The whole box table with the landmark table (64 patches: every box at least twice, with different landmarks and labels; labels from
    {0, 1, 2, -1}, which DenseBox and DenseBoxLM must ignore)."""
    n = 64
    outs, bbox, vert, lab = L.make_batch(kind, n, seed=11)
    assert n >= 2 * len(L.box_table()) and {0., 1., 2., -1.} == set(lab.ravel().tolist())
    rn, lrn = draws(kind, bbox, lab, n, 12)
    got, res = check(kind, outs, bbox, vert, lab, rn, lrn)
    assert got['half'] > 0                                                  # either mining path: both are forced in the next test
    if kind != 'DenseBoxLMLOC':                                             # the labels are ignored
        other = run_gpu(kind, outs, bbox, vert, np.ones_like(lab), rn, lrn)
        assert other['loss'] == got['loss'] and all(np.array_equal(other['grads'][k], got['grads'][k]) for k in NAMES[kind])


@pytest.mark.parametrize('k', [20, 60])
def test_geometry_table_on_either_mining_path(k):
    """The same table with K = 20 (register tournament) and K = 60 > 48 (block_argmax rounds) forced through positive_num_global."""
    kind, n = 'DenseBoxLMLOC', 32
    outs, bbox, vert, lab = L.make_batch(kind, n, seed=13)
    kw = dict(batch_global=n, positive_num_global=L.p_for_half(k, n))
    rn, lrn = draws(kind, bbox, lab, n, 14, **kw)
    got, _ = check(kind, outs, bbox, vert, lab, rn, lrn, **kw)
    assert got['half'] == k


def test_stand_alone_label_ops_on_the_table():
    bt = L.box_table()
    n = len(bt)
    lab = np.asarray(L.LABEL_CYCLE, np.float32)[np.arange(n) % len(L.LABEL_CYCLE)].reshape(n, 1)
    eq = lambda a, ref: np.array_equal(a.cpu().numpy(), ref)               # noqa: E731
    assert eq(LB.init_score_map(T(bt), n), O.init_score_map(bt))
    assert eq(LB.init_score(T(bt), T(lab)), O.init_score_map(bt, lab))
    rs = np.random.RandomState(21)
    m0 = (rs.rand(n, 1, 60, 60) < 0.5).astype(np.float32)
    m = T(m0).cuda()
    LB.mask_gray_zone_cls(m, T(bt))
    assert eq(m, O.mask_gray_zone_cls(m0.copy(), bt))
    m = T(m0).cuda()
    LB.mask_gray_zone_cls_pn(m, T(bt), T(lab))
    assert eq(m, O.mask_gray_zone_cls(m0.copy(), bt, lab))
    for labels in (None, lab):
        cnt = torch.empty(n, dtype=torch.int32, device='cuda')
        bb, lb = T(bt).cuda(), (T(labels).cuda() if labels is not None else None)
        _lib.check(_lib.lib().dbx_count_positives(_lib.ptr(bb), _lib.ptr(lb), n, _lib.ptr(cnt), _lib.stream_ptr()))
        assert eq(cnt, O.init_score_map(bt, labels).sum(axis=(1, 2, 3)).astype(np.int32))
    # the landmark table through the stand-alone heat maps and 5 x 5 gray zones
    lt = L.landmark_table('DenseBoxLM')
    heat = O.init_lm_heatmap(lt)
    assert eq(LB.init_lm_heatmap(T(lt), len(lt)), heat)
    lt2 = L.landmark_table('DenseBoxLMLOC')
    lab2 = np.asarray(L.LABEL_CYCLE, np.float32)[np.arange(len(lt2)) % len(L.LABEL_CYCLE)].reshape(-1, 1)
    assert eq(LB.init_lm_heatmap_pn(T(lt2), T(lab2)), O.init_lm_heatmap(lt2, lab2))
    for j in range(4):
        pos = O.nonzero4(heat[:, j:j + 1])
        m0 = (rs.rand(len(lt), 1, 60, 60) < 0.5).astype(np.float32)
        m = T(m0).cuda()
        LB.mask_gray_zone_lm(m, T(pos), j)
        assert eq(m, O.mask_gray_zone_lm(m0.copy(), pos))


# ------------------------------------------------------------------------------------------------ 2. mining interactions
@pytest.mark.parametrize('kind', ['DenseBoxLM', 'DenseBoxLMLOC'])
def test_random_negatives_on_positives_gray_zones_hard_negatives_and_out_of_range(kind):
    n = 48
    outs, bbox, vert, lab = L.make_batch(kind, n, seed=31)
    pn = kind == 'DenseBoxLMLOC'
    half = half_of(kind, bbox, lab, n)
    assert half >= 8
    rs = np.random.RandomState(32)
    rn, lrn = L.draw_rand_neg(rs, n, half), L.draw_lm_rand_neg(rs, n)
    hard, lm_hard = L.hard_lists(kind, outs, bbox, vert, lab, half)
    gt = O.init_score_map(bbox, lab if pn else None)
    hit = {'positive': 0, 'ring': 0}
    for i in range(n):
        if pn and lab[i, 0] == 0:
            continue
        s = L.spans(bbox[i])
        pos = np.flatnonzero(gt[i, 0])
        if len(pos):
            rn[i, 0] = pos[len(pos) // 2]; hit['positive'] += 1                               # noqa: E702
        (ya, yb), (xa, xb) = s['zero']
        ring = [y * 60 + x for y in range(ya, yb) for x in range(xa, xb)
                if not (s['recore'][0][0] <= y < s['recore'][0][1] and s['recore'][1][0] <= x < s['recore'][1][1])]
        if ring:
            rn[i, 1] = ring[len(ring) // 3]; hit['ring'] += 1                                 # noqa: E702
    rn[:, 2] = hard[:, 0]                                                                     # equal to a hard negative
    rn[:, 3], rn[:, 4], rn[:, 5] = -1, 3600, 2 ** 40                                          # skipped in the mask, echoed in neg_idx
    assert hit['positive'] >= 10 and hit['ring'] >= 10
    px = L.lm_pixels(vert, pn)
    cells = [(dy, dx) for dy in range(-2, 3) for dx in range(-2, 3) if (dy, dx) != (0, 0)]
    for j in range(4):
        for i in range(n):
            x, y = px[i, j]
            if i % 4 == 0:
                lrn[j, i, 0] = y * 60 + x                                                     # on the landmark
            elif i % 4 == 1:                                                                  # inside its 5 x 5 block: every cell of it in turn
                dy, dx = cells[(i // 4 * 4 + j) % 24]
                y2, x2 = (y + dy if 0 <= y + dy < 60 else y - dy), (x + dx if 0 <= x + dx < 60 else x - dx)
                lrn[j, i, 0] = y2 * 60 + x2
            elif i % 4 == 2:
                lrn[j, i, 0] = lm_hard[j, i, 0]                                               # equal to the hard negative
            else:
                lrn[j, i, 0] = (-1, 3600, 2 ** 40)[(i // 4) % 3]                              # out of range
    got, res = check(kind, outs, bbox, vert, lab, rn, lrn)
    assert np.array_equal(got['neg_idx'][:, half + 3:half + 6], np.tile(np.asarray([-1, 3600, 2 ** 40]), (n, 1)))
    assert (got['lm_neg_idx'][:, 3::4, 1] >= 3600).any() and (got['lm_neg_idx'][:, 3::4, 1] < 0).any()


# ------------------------------------------------------------------------------------------------ 3. ties
_TIE_GPU = {}


def tie_inputs(k):
    n = 8
    outs, bbox, vert, lab = L.tie_batch(n, constant_patch=4)                # patch 4: one all-constant score (and landmark) map
    assert lab[4, 0] != 0
    kw = dict(batch_global=n, positive_num_global=L.p_for_half(k, n))
    rs = np.random.RandomState(40)                                          # the same stream for every K
    return outs, bbox, vert, lab, L.draw_rand_neg(rs, n, k), L.draw_lm_rand_neg(np.random.RandomState(41), n), kw


@pytest.mark.parametrize('k', [1, 11, 47, 48, 49, 130])
def test_ties_follow_the_documented_order_on_both_paths(k):
    outs, bbox, vert, lab, rn, lrn, kw = tie_inputs(k)
    got, res = check('DenseBoxLMLOC', outs, bbox, vert, lab, rn, lrn, ties=True, **kw)
    assert got['half'] == k
    neg = L.neg_loss(outs[0], res['gt'])
    assert np.array_equal(got['neg_idx'][:, :k], L.tie_order(neg, k))
    heat = res['heat_gt']
    for j in range(4):                                                      # the landmark hard negative: the lowest index of the maximum
        nl = L.neg_loss(outs[3][:, j:j + 1], heat[:, j:j + 1])
        assert np.array_equal(got['lm_neg_idx'][j, :, 0], np.argmax(nl, axis=1))
    gt4 = res['gt'][4].reshape(-1)
    assert np.array_equal(got['neg_idx'][4, :k], np.flatnonzero(gt4 == 0)[:k])     # constant map: the first K non-positive pixels
    _TIE_GPU[k] = got['neg_idx'][:, :k].copy()


def test_tournament_list_is_a_prefix_of_the_arg_max_list():
    """K = 48 (register tournament) against K = 49 (block_argmax rounds) on the same inputs."""
    for k in (48, 49):
        if k not in _TIE_GPU:
            outs, bbox, vert, lab, rn, lrn, kw = tie_inputs(k)
            _TIE_GPU[k] = run_gpu('DenseBoxLMLOC', outs, bbox, vert, lab, rn, lrn, **kw)['neg_idx'][:, :k].copy()
    assert np.array_equal(_TIE_GPU[48], _TIE_GPU[49][:, :48])


# ------------------------------------------------------------------------------------------------ 4. K extremes
def test_k_3600_selects_every_pixel_in_order():
    kind, n = 'DenseBoxLMLOC', 3
    names = [b[0] for b in L.BOXES]
    boxes = L.box_table()[[names.index('whole-grid'), names.index('left-top-wrap'), names.index('right-edge-block')]]
    outs, bbox, vert, lab = L.make_batch(kind, n, seed=51, boxes=boxes)
    assert (lab != 0).all()
    kw = dict(batch_global=n, positive_num_global=L.p_for_half(3600, n))
    rs = np.random.RandomState(52)
    rn, lrn = np.stack([rs.permutation(3600) for _ in range(n)]).astype(np.int64), L.draw_lm_rand_neg(rs, n)
    got, res = check(kind, outs, bbox, vert, lab, rn, lrn, ties=True, **kw)      # the positives' zeros tie at the end of the list
    assert got['half'] == 3600 and got['neg_idx'].shape == (n, 7200)
    neg = L.neg_loss(outs[0], res['gt'])
    for i in range(n):
        hard = got['neg_idx'][i, :3600]
        assert np.array_equal(np.sort(hard), np.arange(3600)) and (np.diff(neg[i, hard]) <= 0).all()


@pytest.mark.parametrize('kind', L.KINDS)
def test_k_0_on_a_batch_with_positives(kind):
    n = 28
    outs, bbox, vert, lab = L.make_batch(kind, n, seed=53)
    kw = dict(batch_global=10 ** 6)
    assert half_of(kind, bbox, lab, n, **kw) == 0 and half_of(kind, bbox, lab, n) > 0
    got, res = check(kind, outs, bbox, vert, lab, np.zeros((n, 0), np.int64), L.draw_lm_rand_neg(np.random.RandomState(54), n), **kw)
    assert got['half'] == 0 and got['neg_idx'].size == 0 and got['pos_count'].sum() > 0


# ------------------------------------------------------------------------------------------------ 5. the finish kernel's groups of 256
@pytest.mark.parametrize('kind,n', [('DenseBox', 1), ('DenseBox', 255), ('DenseBox', 256), ('DenseBox', 257), ('DenseBox', 513),
                                    ('DenseBoxLMLOC', 257)])
def test_batch_sizes_across_the_finish_groups(kind, n):
    outs, bbox, vert, lab = L.make_batch(kind, n, seed=60 + n)
    P = int(O.init_score_map(bbox, lab if kind == 'DenseBoxLMLOC' else None).sum())
    kw = dict(batch_global=n, positive_num_global=P)                        # what the call computes itself, so sub-batches mine alike
    rn, lrn = draws(kind, bbox, lab, n, 61, **kw)
    got, res = check(kind, outs, bbox, vert, lab, rn, lrn, **kw)
    # a sample of 8 patches (first and last included) run one at a time with the batch's K: the same masks and gradients bit for bit,
    # each loss within the bar of its share of loss64, and so their float64 sum
    per = L.loss64(res, outs, kind, per_patch=True)
    assert abs(per.sum() - res['loss64']) <= 1e-12 * res['loss64']
    sample = sorted({0, n - 1} | set(np.random.RandomState(n).choice(n, min(n, 8), replace=False)[:6].tolist()))
    alone = []
    for i in sample:
        one = run_gpu(kind, [o[i:i + 1] for o in outs], bbox[i:i + 1], vert[i:i + 1], lab[i:i + 1], rn[i:i + 1], lrn[:, i:i + 1], **kw)
        assert np.array_equal(one['mask_cls'][0], got['mask_cls'][i]) and np.array_equal(one['neg_idx'][0], got['neg_idx'][i])
        assert all(np.array_equal(one['grads'][k][0], got['grads'][k][i]) for k in NAMES[kind])
        assert abs(float(one['loss']) - per[i]) <= L.TOL_LOSS * per[i]
        alone.append(float(one['loss']))
    assert abs(float(np.sum(np.asarray(alone, np.float64))) - per[sample].sum()) <= L.TOL_LOSS * per[sample].sum()


# ------------------------------------------------------------------------------------------------ 6. lambdas
@pytest.mark.parametrize('kind', L.KINDS)
def test_lambdas_other_than_the_defaults(kind):
    n = 30
    outs, bbox, vert, lab = L.make_batch(kind, n, seed=71)
    kw = dict(lambda_det=0.7, lambda_loc=2.5, lambda_lm=0.3)
    rn, lrn = draws(kind, bbox, lab, n, 72)
    got, res = check(kind, outs, bbox, vert, lab, rn, lrn, **kw)
    default = run_gpu(kind, outs, bbox, vert, lab, rn, lrn)
    assert default['loss'] != got['loss'] and np.array_equal(default['mask_cls'], got['mask_cls'])
    if kind == 'DenseBox':                                                  # train_online has no lambda_det (DenseBox.py:2917)
        other = run_gpu(kind, outs, bbox, vert, lab, rn, lrn, **dict(kw, lambda_det=123.0))
        assert other['loss'] == got['loss'] and all(np.array_equal(other['grads'][k], got['grads'][k]) for k in NAMES[kind])


# ------------------------------------------------------------------------------------------------ 7. debug outputs are optional
@pytest.mark.parametrize('kind', L.KINDS)
def test_debug_outputs_are_optional_and_launches_repeat_bitwise(kind):
    n = 20
    outs, bbox, vert, lab = L.make_batch(kind, n, seed=81)
    rn, lrn = draws(kind, bbox, lab, n, 82)
    a = run_gpu(kind, outs, bbox, vert, lab, rn, lrn, debug=True)
    b = run_gpu(kind, outs, bbox, vert, lab, rn, lrn, debug=False)
    c = run_gpu(kind, outs, bbox, vert, lab, rn, lrn, debug=True)
    for other in (b, c):
        assert other['loss'].tobytes() == a['loss'].tobytes()
        assert all(other['grads'][k].tobytes() == a['grads'][k].tobytes() for k in NAMES[kind])
    assert all(np.array_equal(a[k], c[k]) for k in ('mask_cls', 'neg_idx', 'pos_count'))


# ------------------------------------------------------------------------------------------------ landmarks outside the grid
BAD = {'DenseBoxLM': (17, 2, 0, 59.5, 59.0),        # patch, landmark, 0 = x / 1 = y, the value (x rounds to 60), the value moved in range
       'DenseBoxLMLOC': (17, 2, 1, -3.0, 3.0)}      # y = -3: int(-2.5) = -2


def bad_batch(kind):
    p, c, ax, bad, ok = BAD[kind]
    outs, bbox, vert, lab = L.make_batch(kind, 24, seed=91)
    assert lab[p, 0] != 0 and L.BRANCH['inside'](L.spans(bbox[p]))
    v_bad, v_ok = vert.copy(), vert.copy()
    v_bad[p, 2 * c + ax], v_ok[p, 2 * c + ax] = bad, ok
    rn, lrn = draws(kind, bbox, lab, 24, 92)
    return outs, bbox, v_bad, v_ok, lab, rn, lrn


@pytest.mark.parametrize('kind', ['DenseBoxLM', 'DenseBoxLMLOC'])
def test_host_resident_vertices_outside_the_grid_raise_before_the_launch(kind):
    outs, bbox, v_bad, v_ok, lab, rn, lrn = bad_batch(kind)
    dev = [T(o).cuda().requires_grad_(True) for o in outs]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for v in (v_bad, T(v_bad)):
        with pytest.raises(IndexError, match='is out of bounds for dimension with size 60'):
            densebox_loss(kind, tuple(dev), bbox, v, lab, rand_neg_indices=rn, lm_rand_neg_indices=lrn, return_debug=True)
    assert torch.cuda.memory_allocated() == before                          # no output buffer was even made, none written
    assert all(d.grad is None for d in dev)


@pytest.mark.parametrize('kind', ['DenseBoxLM', 'DenseBoxLMLOC'])
def test_device_resident_landmark_outside_the_grid_is_never_an_index(kind):
    """That (patch, channel) has no positive pixel and no gray zone: its mask is what mining alone leaves, its heat map is zero.  Every
    other patch and channel is bit-identical to the same batch with the landmark moved in range."""
    p, c, ax, _, _ = BAD[kind]
    outs, bbox, v_bad, v_ok, lab, rn, lrn = bad_batch(kind)
    pn = kind == 'DenseBoxLMLOC'
    res = run_oracle(kind, outs, bbox, v_ok, lab, rn, lrn)
    ok = run_gpu(kind, outs, bbox, v_ok, lab, rn, lrn)
    compare(kind, ok, res)
    got = run_gpu(kind, outs, bbox, T(v_bad).cuda(), lab, rn, lrn)
    # the reference for (p, c), assembled from the oracle's pieces: zero heat map, top-1 by the rule, the random draw, no gray zone
    lm = outs[NAMES[kind].index('lm')]
    nl = L.neg_loss(lm[p:p + 1, c:c + 1], np.zeros((1, 1, 60, 60), np.float32))
    hard = L.tie_order(nl, 1).reshape(1, 1)
    plane = np.zeros((1, 1, 60, 60), np.float32)
    O.mask_by_sel(plane, np.zeros((0, 4), np.int64), np.concatenate([hard, lrn[c, p].reshape(1, 1)], axis=1))
    assert 1 <= int(plane.sum()) <= 2
    want = dict(res)
    want['heat_gt'], want['lm_mask'], want['lm_neg_idx'] = res['heat_gt'].copy(), res['lm_mask'].copy(), res['lm_neg_idx'].copy()
    want['heat_gt'][p, c] = 0
    want['lm_mask'][p, c] = plane[0, 0]
    want['lm_neg_idx'][c, p, 0] = hard[0, 0]
    grads = {k: g.copy() for k, g in res['grads'].items()}
    grads['lm'][p, c] = (2.0 * np.float32(0.5)) * plane[0, 0] * lm[p, c]                    # lambda_lm = 0.5, target 0
    if pn:
        want['lmloc_gt'] = O.init_lm_locmap(v_bad, lab)                                      # the offsets take the vertex as it is
        mg = (res['mask'] * res['gt'])[p, 0]
        assert mg.any()
        ch = 2 * c + ax
        grads['lmloc'][p, ch] = 2.0 * mg * (outs[4][p, ch] - want['lmloc_gt'][p, ch])
    want['grads'] = grads
    want['loss64'] = L.loss64(want, outs, kind)
    assert want['loss64'] != res['loss64']
    compare(kind, got, want)
    # everything but (p, c) -- and the one offset channel of that vertex -- bit-identical to the in-range batch
    keep = np.ones((24, 4), bool)
    keep[p, c] = False
    assert np.array_equal(got['mask_lm'][keep], ok['mask_lm'][keep]) and got['grads']['lm'][keep].tobytes() == ok['grads']['lm'][keep].tobytes()
    lni = np.ones((4, 24), bool)
    lni[c, p] = False
    assert np.array_equal(got['lm_neg_idx'][lni], ok['lm_neg_idx'][lni])
    for k in ('score', 'loc', 'rf'):
        assert got['grads'][k].tobytes() == ok['grads'][k].tobytes()
    assert np.array_equal(got['mask_cls'], ok['mask_cls']) and np.array_equal(got['neg_idx'], ok['neg_idx'])
    if pn:
        keep8 = np.ones((24, 8), bool)
        keep8[p, 2 * c + ax] = False
        assert got['grads']['lmloc'][keep8].tobytes() == ok['grads']['lmloc'][keep8].tobytes()
        # the stand-alone heat map never indexes with it either
        heat = LB.init_lm_heatmap_pn(T(v_bad).cuda(), T(lab)).cpu().numpy()
        assert np.array_equal(heat, want['heat_gt'])
