"""The training patch warp on the GPU: dbx_patch_warp == the NumPy restatement (tests/warp_aug_ref.py) bit for bit on a table of 16
records (identity, shifts, rotations, scales, shear, keystones, a quad wholly outside, degenerate and non-convex quads), both borders,
c = 1..4, input and output at odd byte addresses; a zero-border slot == dbx_warp_perspective_u8 with the slot's fwd; dbx_patch_warp_plan's
records, labels and matrices == the restatement's and the host export's in injected and in device mode; slots past the count are left
alone; overlap is refused; a PatchSampler with a Warp replays in a captured graph, its batch is the restatement of its own raw patches,
the augmenter reads the warp's output, warp=None is the sampler it was, and net.loss gets the restatement's labels; the band store at
every destination offset 0..15, c = 1..4."""
import functools
import gc
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug_ref as A                                     # noqa: E402
import warp_aug_ref as W                                # noqa: E402
from patch_stage_util import GAMMAS, SENTINEL, _at_offset, _augment, _scene, _snap, _untouched      # noqa: E402
from warp_host import host_plan, host_warp, same_plan  # noqa: E402

import densebox_amd as D                                # noqa: E402
from densebox_amd import data, rectify, synth           # noqa: E402

pytestmark = pytest.mark.gpu

FILL = W.pack_fill(11, 22, 33, 244)


def _cfg_dict(warp):
    f = warp.cfg()
    return {k: getattr(f, k) for k in W.CFG_DEFAULT}


def _launch(host_patches, recs, rows, count=None, in_off=33, out_off=17, cfg=None):
    """Injected records through both launches; returns (out view, out arena, WarpPlan)."""
    n, c = host_patches.shape[0], host_patches.shape[3]
    _, src = _at_offset(n, c, in_off, host_patches)
    arena, out = _at_offset(n, c, out_off)
    d_count = torch.tensor([n if count is None else count], dtype=torch.int32, device='cuda')
    params = torch.from_numpy(np.stack([W.to_row(r) for r in recs])).cuda()
    plan = data.plan_warp(torch.from_numpy(rows).cuda(), d_count, cfg if cfg is not None else data.Warp().cfg(), params=params)
    data.apply_warp(src, plan.params, plan.inv, d_count, out)
    torch.cuda.synchronize()
    return out, arena, plan


def _plan_host(plan, count):
    g = lambda t: np.ascontiguousarray(t.cpu().numpy()[:count])     # noqa: E731
    return dict(params=g(plan.params), labels=g(plan.labels_i32), bbox=g(plan.bbox), vertices=g(plan.vertices), label=g(plan.labels),
                fwd=g(plan.fwd), inv=g(plan.inv))


@pytest.mark.parametrize('c', [1, 2, 3, 4])
@pytest.mark.parametrize('border', [0, 1])
def test_pixels_equal_the_restatement_at_odd_addresses(c, border):
    n = len(W.CASES)
    assert n == 16
    patches = np.random.RandomState(10 * c + border).randint(0, 256, size=(n, 240, 240, c)).astype(np.uint8)
    recs = [W.record(q, border=border, fill=FILL) for _, q in W.CASES]
    rows = np.zeros((n, 12), np.int32)                  # negatives: the label rule refuses nothing
    out, arena, plan = _launch(patches, recs, rows)
    assert out.data_ptr() % 2 == 1
    want = W.plan(W.CFG_DEFAULT, rows, n, params_in=recs)
    same_plan(_plan_host(plan, n), want)
    flags = dict(zip([name for name, _ in W.CASES], want['params'][:, 0].tolist()))
    assert flags['outside'] == 1 and flags['degenerate_equal_corners'] == 4 and flags['rot_-15'] == 1
    got = out.cpu().numpy()
    for s, (name, _) in enumerate(W.CASES):
        ref = W.warp(patches[s], want['params'][s], want['inv'][s])
        bad = np.argwhere(got[s] != ref)
        assert len(bad) == 0, (name, c, border, len(bad), bad[:4].tolist())
        assert np.array_equal(ref, patches[s]) == (name == 'identity' or flags[name] != 1), name
    assert _untouched(arena, 17, n * 240 * 240 * c)


@pytest.mark.parametrize('in_off,out_off', [(0, 0), (1, 0), (0, 15), (2, 4), (3, 8)])
def test_other_alignments(in_off, out_off):
    """n = 3, c = 3: a rotation with each border and a copy, on patches whose rows differ (so a wrong row at a band seam shows)."""
    quads = dict(W.CASES)
    recs = [W.record(quads['rot_+15'], border=0, fill=FILL), W.record(quads['aspect_shear'], border=1), W.record(quads['rot_-15'], flags=0)]
    patches = np.random.RandomState(in_off * 16 + out_off).randint(0, 256, size=(3, 240, 240, 3)).astype(np.uint8)
    out, arena, plan = _launch(patches, recs, np.zeros((3, 12), np.int32), in_off=in_off, out_off=out_off)
    got, ph = out.cpu().numpy(), _plan_host(plan, 3)
    for s in range(3):
        assert np.array_equal(got[s], W.warp(patches[s], ph['params'][s], ph['inv'][s])), s
    assert np.array_equal(got[2], patches[2]) and _untouched(arena, out_off, patches.size)


@pytest.mark.parametrize('c', [1, 3, 4])
def test_a_zero_border_slot_is_the_pinned_warp_kernel_with_the_slot_s_fwd(c):
    names = ('rot_+15', 'scale_0.85', 'strong_keystone', 'shift_frac', 'outside')
    quads = dict(W.CASES)
    recs = [W.record(quads[k], border=0, fill=0) for k in names]
    patches = np.random.RandomState(c).randint(0, 256, size=(len(recs), 240, 240, c)).astype(np.uint8)
    out, _, plan = _launch(patches, recs, np.zeros((len(recs), 12), np.int32))
    fwd = plan.fwd.cpu().numpy()
    for s, name in enumerate(names):
        pinned = rectify.warp_perspective(torch.from_numpy(patches[s]).cuda(), fwd[s].reshape(3, 3), (240, 240))
        assert torch.equal(out[s], pinned), name
        assert np.array_equal(host_warp(patches[s], W.to_row(recs[s]), plan.inv[s].cpu().numpy()), pinned.cpu().numpy()), name


@pytest.mark.parametrize('n,count', [(1, 1), (7, 3)])
def test_slots_past_the_count_are_left_alone(n, count):
    patches = np.random.RandomState(5 + n).randint(0, 256, size=(n, 240, 240, 3)).astype(np.uint8)
    recs = [W.record(q, border=s % 2, fill=FILL) for s, (_, q) in enumerate(W.CASES[5:5 + n])]
    rows = W.label_rows(n, seed=8)
    d_rows, d_count = torch.from_numpy(rows).cuda(), torch.tensor([count], dtype=torch.int32, device='cuda')
    src = torch.from_numpy(patches).cuda()
    arena, out = _at_offset(n, 3, 5)
    plan = data.WarpPlan(n, 'cuda')
    outs = (plan.params, plan.labels_i32, plan.bbox, plan.vertices, plan.labels, plan.fwd, plan.inv)
    for t in outs:
        t.fill_(-7)
    params = torch.from_numpy(np.stack([W.to_row(r) for r in recs])).cuda()
    cfg = data.Warp().cfg()
    data.plan_warp(d_rows, d_count, cfg, params=params, out=plan)
    data.apply_warp(src, plan.params, plan.inv, d_count, out)
    torch.cuda.synchronize()
    want = W.plan(W.CFG_DEFAULT, rows, count, params_in=recs)
    same_plan(_plan_host(plan, count), want)
    for t in outs:
        assert bool((t[count:] == -7).all())
    got = out.cpu().numpy()
    for s in range(count):
        assert np.array_equal(got[s], W.warp(patches[s], want['params'][s], want['inv'][s])), s
    assert bool((out[count:] == SENTINEL).all()) and _untouched(arena, 5, patches.size)
    # a count above n is n
    eye = torch.tensor(W.EYE, dtype=torch.float64, device='cuda').repeat(n, 1)
    d_count.fill_(100)
    data.apply_warp(src, params, eye, d_count, out)
    torch.cuda.synchronize()
    assert np.array_equal(out[n - 1].cpu().numpy(), W.warp(patches[n - 1], recs[n - 1], W.EYE))
    # count = 0 and a negative count write nothing, neither pixels nor rows, and the plan still counts its launch
    for t in outs:
        t.fill_(-7)
    state = torch.tensor([3, 9], dtype=torch.int64, device='cuda')
    bank = torch.from_numpy(W.rot_bank(-15, 15)).cuda()
    for cnt in (0, -1):
        out.fill_(SENTINEL)
        d_count.fill_(cnt)
        data.apply_warp(src, params, eye, d_count, out)
        data.plan_warp(d_rows, d_count, cfg, params=params, out=plan)
        data.plan_warp(d_rows, d_count, cfg, bank=bank, state=state, out=plan)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and all(bool((t == -7).all()) for t in outs)
    assert state.tolist() == [3, 11]


@pytest.mark.parametrize('n', [1, 7])
def test_records_labels_and_matrices_in_both_modes_and_the_counter(n):
    warp = data.Warp(p=0.9, seed=31 + n)
    cfg, bank = _cfg_dict(warp), warp.bank()
    rows = W.label_rows(n, seed=n)
    rows[0] = [40, 50, 240, 120, 42, 52, 236, 50, 240, 118, 40, 120]                   # 240 is past the margin: refused when on
    d_rows, d_count = torch.from_numpy(rows).cuda(), torch.tensor([n], dtype=torch.int32, device='cuda')
    d_bank = torch.from_numpy(bank).cuda()
    state = torch.tensor([warp.seed, 5], dtype=torch.int64, device='cuda')
    seen = []
    for k in range(3):                                  # device mode: a launch per counter value
        plan = data.plan_warp(d_rows, d_count, warp.cfg(), bank=d_bank, state=state)
        torch.cuda.synchronize()
        assert state.tolist() == [warp.seed, 6 + k]
        want = W.plan(cfg, rows, n, bank=bank, seed=warp.seed, counter=5 + k)
        same_plan(_plan_host(plan, n), want)
        same_plan(host_plan(cfg, rows, n, bank=bank, seed=warp.seed, counter=5 + k), want)
        seen.append(want['params'])
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    assert all(int(p[0, 0]) in (0, 2) for p in seen) and any(int(p[0, 0]) == 2 for p in seen)
    # injected mode: refusal bits set on input are ignored (flags & 1); the state is not touched
    quads = [q for _, q in W.CASES[1:1 + n]]
    recs = [W.record(q, flags=(1, 3, 5, 7, 2, 4, 6)[s], border=s % 3, fill=FILL) for s, q in enumerate(quads)]
    params = torch.from_numpy(np.stack([W.to_row(r) for r in recs])).cuda()
    plan = data.plan_warp(d_rows, d_count, warp.cfg(), params=params, state=state)
    torch.cuda.synchronize()
    want = W.plan(cfg, rows, n, params_in=recs)
    same_plan(_plan_host(plan, n), want)
    same_plan(host_plan(cfg, rows, n, params_in=recs), want)
    assert want['params'][0, 0] == 2 and state.tolist() == [warp.seed, 8]
    if n == 7:
        assert want['params'][4:, 0].tolist() == [0, 0, 0] and (want['params'][1:4, 0] & 1).all()


def test_warp_patches_front_end():
    n = 4
    patches = np.random.RandomState(77).randint(0, 256, size=(n, 240, 240, 3)).astype(np.uint8)
    rows = W.label_rows(n, seed=12)
    warp = data.Warp(p=1.0, border='constant', fill=(9, 8, 7), seed=9)
    out, lab_i32, bbox, vert, lab, params, fwd, inv = data.warp_patches(patches, rows, warp=warp, counter=4)
    torch.cuda.synchronize()
    want = W.plan(_cfg_dict(warp), rows, n, bank=warp.bank(), seed=9, counter=4)
    got = dict(params=params, labels=lab_i32, bbox=bbox, vertices=vert, label=lab, fwd=fwd, inv=inv)
    same_plan({k: v.cpu().numpy() for k, v in got.items()}, want)
    for s in range(n):
        assert np.array_equal(out[s].cpu().numpy(), W.warp(patches[s], want['params'][s], want['inv'][s])), s
    assert (want['params'][:, 0] & 1).any() and (want['params'][:, 1] == 0).all() and (want['params'][:, 2] == W.pack_fill(9, 8, 7)).all()
    # injected: the records that came out give the same output (a refused slot is then simply not asked for)
    again = data.warp_patches(torch.from_numpy(patches).cuda(), rows, warp=warp, params=want['params'])
    assert torch.equal(again[0], out) and torch.equal(again[7], inv) and torch.equal(again[5][:, 1:], params[:, 1:])
    # Warp.identity() draws nothing but copies
    got = data.warp_patches(patches, rows, warp=data.Warp.identity(seed=4), counter=2)
    assert torch.equal(got[0].cpu(), torch.from_numpy(patches)) and np.array_equal(got[1].cpu().numpy(), rows) and not got[5][:, 0].any()


def test_overlapping_input_and_output_is_refused():
    arena = torch.zeros(4 * 240 * 240 * 3, dtype=torch.uint8, device='cuda')
    size = 3 * 240 * 240 * 3
    a = arena[:size].view(3, 240, 240, 3)
    params = torch.from_numpy(np.stack([W.to_row(W.record(W.shifted(48, 0)))] * 3)).cuda()
    eye = torch.tensor(W.EYE, dtype=torch.float64, device='cuda').repeat(3, 1)
    count = torch.tensor([3], dtype=torch.int32, device='cuda')
    for off in (0, 1, 240 * 240 * 3):
        with pytest.raises(RuntimeError, match='overlap'):
            data.apply_warp(a, params, eye, count, arena[off:off + size].view(3, 240, 240, 3))
    torch.cuda.synchronize()
    assert not arena.any()


BAND_RECORDS = {'rot_+15, replicate': W.record(dict(W.CASES)['rot_+15'], border=1),
                'bit 0 clear (the copy path)': W.record(dict(W.CASES)['rot_+15'], flags=0, border=1)}


@functools.lru_cache(maxsize=None)
def _band_case(c, kind):
    """(patch, restatement) of one slot through BAND_RECORDS[kind]: made once per c and kind, shared by the 16 offsets."""
    patch = np.random.RandomState(40 + c).randint(0, 256, size=(1, 240, 240, c)).astype(np.uint8)
    p = W.plan(W.CFG_DEFAULT, np.zeros((1, 12), np.int32), 1, params_in=[BAND_RECORDS[kind]])
    want = W.warp(patch[0], p['params'][0], p['inv'][0])
    want.setflags(write=False)
    return patch, want


@pytest.mark.parametrize('kind', sorted(BAND_RECORDS))
@pytest.mark.parametrize('out_off', range(16))
@pytest.mark.parametrize('c', [1, 2, 3, 4])
def test_the_band_store_at_every_destination_offset(c, out_off, kind):
    """n = 1 (15 workgroups): patch_band_store's 16-byte words, dwords and bytes at every offset of the destination inside a 16-byte
    word, source at offset 33; the output is the restatement bit for bit and no byte outside the view is written."""
    patch, want = _band_case(c, kind)
    out, arena, _ = _launch(patch, [BAND_RECORDS[kind]], np.zeros((1, 12), np.int32), in_off=33, out_off=out_off)
    assert out.data_ptr() % 16 == out_off
    bad = np.argwhere(out[0].cpu().numpy() != want)
    assert len(bad) == 0, (kind, c, out_off, len(bad), bad[:4].tolist())
    assert _untouched(arena, out_off, patch.size)
    assert (kind == 'bit 0 clear (the copy path)') == np.array_equal(want, patch[0])


def _warp():
    return data.Warp(p=0.8, seed=41)


def _sampler(seed, n=7, **kw):
    frames, plates = _scene()
    return data.PatchSampler(frames, plates, n, oversample=4.0, neg_frac=0.2, seed=seed, **kw)


def test_three_eager_calls_equal_three_replays_of_one_captured_graph():
    a, b = _sampler(11, warp=_warp(), augment=_augment()), _sampler(11, warp=_warp(), augment=_augment())
    a.launch()                                          # warm up outside the capture
    torch.cuda.synchronize()
    for name in ('state', 'aug_state', 'warp_state'):
        getattr(b, name).copy_(getattr(a, name))
    g = torch.cuda.CUDAGraph()
    gc.collect()
    with torch.cuda.graph(g):
        a.launch()
    seen = []
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        got = _snap(a)
        batch = b.next_batch()
        want = _snap(b)
        assert batch[4] == 7 and batch[0] is b.aug_patches and batch[1] is b.aug.bbox
        assert all(torch.equal(p, q) for p, q in zip(got, want)), k
        assert all(not torch.equal(got[0], s) for s in seen)
        seen.append(got[0])
    assert a.warp_state.tolist() == b.warp_state.tolist() == [41, 4] and a.aug_state.tolist() == [23, 4] and a.state.tolist() == [11, 4]


def test_a_sampler_batch_is_the_restatement_of_its_own_raw_patches():
    s = _sampler(5, warp=_warp())
    plain = _sampler(5)
    flags = set()
    for k in range(2):
        patches, bbox, vertices, labels, count = s.next_batch()
        raw_plain = plain.next_batch()
        assert count == 7 and patches is s.warped and patches is not s.raw and bbox is s.warp_plan.bbox
        assert torch.equal(s.raw, raw_plain[0]) and torch.equal(s.plan.bbox, raw_plain[1])      # the plan's draws do not depend on the warper
        rows = s.plan.labels_i32.cpu().numpy()
        want = W.plan(_cfg_dict(s.warp), rows, count, bank=s.warp.bank(), seed=41, counter=k)
        same_plan(_plan_host(s.warp_plan, count), want)
        assert torch.equal(s.warp_params, s.warp_plan.params)
        bits = lambda t: t.cpu().numpy().view(np.uint32)                                           # noqa: E731
        assert np.array_equal(bits(bbox), want['bbox'].view(np.uint32)) and np.array_equal(bits(vertices), want['vertices'].view(np.uint32))
        assert np.array_equal(bits(labels), want['label'].view(np.uint32))
        raw, got = s.raw.cpu().numpy(), patches.cpu().numpy()
        for i in range(count):
            assert np.array_equal(got[i], W.warp(raw[i], want['params'][i], want['inv'][i])), (k, i)
        flags |= set(want['params'][:, 0].tolist())
        assert not np.array_equal(got, raw)
    assert 1 in flags


def test_the_augmenter_reads_the_warp_s_labels_and_pixels():
    host_bank = A.gamma_bank(GAMMAS)
    s = _sampler(6, warp=_warp(), augment=_augment())
    patches, bbox, vertices, labels, count = s.next_batch()
    assert count == 7 and patches is s.aug_patches and bbox is s.aug.bbox
    f = s.augment.cfg()
    aug_cfg = {k: (tuple(f.kind_w) if k == 'kind_w' else getattr(f, k)) for k in A.CFG_DEFAULT}
    warp_rows = s.warp_plan.labels_i32.cpu().numpy()
    assert not np.array_equal(warp_rows, s.plan.labels_i32.cpu().numpy())
    want = A.plan(aug_cfg, warp_rows, count, seed=23, counter=0)
    assert np.array_equal(s.aug_params.cpu().numpy(), want['params']) and np.array_equal(s.aug.labels_i32.cpu().numpy(), want['labels'])
    assert np.array_equal(bbox.cpu().numpy(), want['bbox']) and np.array_equal(vertices.cpu().numpy(), want['vertices'])
    assert np.array_equal(labels.cpu().numpy(), want['label'])
    warped, got = s.warped.cpu().numpy(), patches.cpu().numpy()
    for i in range(count):
        assert np.array_equal(got[i], A.augment(warped[i], want['params'][i], host_bank)), i
    # and the warped patches are the restatement of the raw ones
    ww = W.plan(_cfg_dict(s.warp), s.plan.labels_i32.cpu().numpy(), count, bank=s.warp.bank(), seed=41, counter=0)
    raw = s.raw.cpu().numpy()
    for i in range(count):
        assert np.array_equal(warped[i], W.warp(raw[i], ww['params'][i], ww['inv'][i])), i


@pytest.mark.parametrize('with_augment', [False, True])
def test_without_a_warp_the_sampler_is_what_it_was(with_augment):
    """warp=None adds no launch: the batch is dbx_patch_plan + dbx_patch_cut (+ the augmenter on the cut's own rows and pixels), as
    sample_patches and augment_patches make it from the same seeds."""
    frames, plates = _scene()
    s = _sampler(9, augment=_augment() if with_augment else None)
    assert s.warp is None and s.warped is None and s.warp_plan is None and s.warp_params is None
    for k in range(2):
        batch = s.next_batch()
        ref_patches, ref_plan = data.sample_patches(frames, plates, 7, neg_frac=0.2, seed=9, counter=k, m=s.M)
        assert torch.equal(s.raw, ref_patches) and torch.equal(s.plan.labels_i32, ref_plan.labels_i32) and batch[4] == 7
        if with_augment:
            ref = data.augment_patches(ref_patches, ref_plan, augment=_augment(), counter=k)
            assert batch[0] is s.aug_patches and torch.equal(batch[0], ref[0]) and torch.equal(batch[1], ref[2])
            assert torch.equal(batch[2], ref[3]) and torch.equal(batch[3], ref[4]) and torch.equal(s.aug_params, ref[5])
        else:
            assert batch[0] is s.patches and batch[1] is s.plan.bbox and batch[3] is s.plan.labels


def test_net_loss_on_a_warped_sampler_batch_equals_net_loss_on_the_restated_labels():
    net = D.DenseBoxLMLOC(synth.vgg19_standin(seed=0))
    synth.fill_params_(net, 11)
    net = net.cuda().eval()
    net.compute_dtype = 'f32'
    frames, plates = _scene()
    warp = data.Warp(p=1.0, seed=2)
    s = data.PatchSampler(frames, plates, 2, oversample=4.0, neg_frac=0.0, seed=3, warp=warp)
    patches, bbox, vertices, labels, count = s.next_batch()
    assert count == 2 and patches.dtype == torch.uint8 and tuple(patches.shape) == (2, 240, 240, 3)
    want = W.plan(_cfg_dict(warp), s.plan.labels_i32.cpu().numpy(), 2, bank=warp.bank(), seed=2, counter=0)
    assert (want['params'][:, 0] == 1).any()
    with torch.no_grad():
        outs = net(patches)
    got = net.loss(outs, bbox, vertices, labels, rng=np.random.RandomState(4))
    b2, v2, l2 = (torch.from_numpy(want[k]) for k in ('bbox', 'vertices', 'label'))
    ref = net.loss(outs, b2, v2, l2, rng=np.random.RandomState(4))
    assert torch.equal(bbox.cpu(), b2) and torch.equal(vertices.cpu(), v2) and torch.equal(labels.cpu(), l2)
    assert not torch.equal(s.plan.vertices.cpu(), v2)                                  # the warp moved the landmarks
    assert float(got) > 0 and np.float32(float(got)).tobytes() == np.float32(float(ref)).tobytes()
