"""Patch augmentation on the GPU: dbx_patch_augment == the NumPy restatement (tests/aug_ref.py) bit for bit -- each op alone at both
ends of its range, each blur kind (band seams and the four edges), all ops together, c = 1, 3, 4, input and output at odd byte
addresses; dbx_patch_aug_plan's records and labels == the restatement's in injected and in device mode; slots past the count are left
alone; the identity copies; overlap is refused; a PatchSampler with an Augment replays in a captured graph, and its batch is the
restatement of its own raw patches and gives net.loss the restatement's labels; the band store at every destination offset 0..15, c = 1..4."""
import functools
import gc
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug_ref as A                                     # noqa: E402
from patch_stage_util import GAMMAS, SENTINEL, _at_offset, _augment, _scene, _snap, _untouched      # noqa: E402

import densebox_amd as D                                # noqa: E402
from densebox_amd import data, synth                    # noqa: E402

pytestmark = pytest.mark.gpu

GROUPS = [A.CASES[k:k + 7] for k in range(0, len(A.CASES), 7)]       # 21 cases: three launches of n = 7


@pytest.fixture(scope='module')
def bank():
    host = A.gamma_bank(GAMMAS)
    return host, torch.from_numpy(host).cuda()


def _cfg_dict(augment):
    f = augment.cfg()
    return {k: (tuple(f.kind_w) if k == 'kind_w' else getattr(f, k)) for k in A.CFG_DEFAULT}


def _launch(host_patches, recs, rows, dbank, count=None, in_off=33, out_off=17):
    """Injected records through both launches; returns (out view, out arena, AugPlan)."""
    n, c = host_patches.shape[0], host_patches.shape[3]
    _, src = _at_offset(n, c, in_off, host_patches)
    arena, out = _at_offset(n, c, out_off)
    d_count = torch.tensor([n if count is None else count], dtype=torch.int32, device='cuda')
    params = torch.from_numpy(np.stack([A.to_row(r) for r in recs])).cuda()
    cfg = data.Augment(gammas=GAMMAS).cfg()
    plan = data.plan_augment(torch.from_numpy(rows).cuda(), d_count, cfg, params=params)
    data.apply_augment(src, plan.params, d_count, dbank, out)
    torch.cuda.synchronize()
    return out, arena, plan


@pytest.mark.parametrize('c', [1, 3, 4])
@pytest.mark.parametrize('group', [0, 1, 2])
def test_pixels_equal_the_restatement_at_odd_addresses(bank, c, group):
    host_bank, dbank = bank
    cases = GROUPS[group]
    n = len(cases)
    assert n == 7
    patches = np.random.RandomState(10 * c + group).randint(0, 256, size=(n, 240, 240, c)).astype(np.uint8)
    rows = np.zeros((n, 12), np.int32)                  # negatives: a flip is never refused
    out, arena, plan = _launch(patches, [r for _, r in cases], rows, dbank)
    assert out.data_ptr() % 2 == 1
    got = out.cpu().numpy()
    for s, (name, rec) in enumerate(cases):
        want = A.augment(patches[s], rec, host_bank)
        bad = np.argwhere(got[s] != want)
        assert len(bad) == 0, (name, c, len(bad), bad[:4].tolist())
    assert _untouched(arena, 17, n * 240 * 240 * c)
    assert np.array_equal(plan.params.cpu().numpy(), np.stack([A.to_row(A.sanitize(r, 4)) for _, r in cases]))


@pytest.mark.parametrize('in_off,out_off', [(0, 0), (1, 0), (0, 15), (2, 4), (3, 8)])
def test_every_blur_kind_at_other_alignments(bank, in_off, out_off):
    """n = 3: the three blur kinds with a flip, on a patch whose rows differ (so a wrong row at a band seam shows)."""
    host_bank, dbank = bank
    recs = [A.record(blur=1, flags=1), A.record(blur=2), A.record(blur=3, box_len=5, flags=1)]
    patches = np.random.RandomState(in_off * 16 + out_off).randint(0, 256, size=(3, 240, 240, 3)).astype(np.uint8)
    out, arena, _ = _launch(patches, recs, np.zeros((3, 12), np.int32), dbank, in_off=in_off, out_off=out_off)
    got = out.cpu().numpy()
    for s in range(3):
        assert np.array_equal(got[s], A.augment(patches[s], recs[s], host_bank)), s
    assert _untouched(arena, out_off, patches.size)


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('c', [1, 2, 3, 4])
def test_the_identity_record_gives_the_input(bank, n, c):
    _, dbank = bank
    patches = np.random.RandomState(n + c).randint(0, 256, size=(n, 240, 240, c)).astype(np.uint8)
    out, arena, plan = _launch(patches, [A.record()] * n, A.label_rows(n, seed=c), dbank)
    assert np.array_equal(out.cpu().numpy(), patches) and _untouched(arena, 17, patches.size)
    assert np.array_equal(plan.labels_i32.cpu().numpy(), A.label_rows(n, seed=c))
    # and Augment.identity() in device mode draws nothing but identity records
    ident = data.Augment.identity(seed=4)
    got = data.augment_patches(torch.from_numpy(patches).cuda(), A.label_rows(n, seed=c), augment=ident, counter=2)
    assert torch.equal(got[0].cpu(), torch.from_numpy(patches)) and np.array_equal(got[1].cpu().numpy(), A.label_rows(n, seed=c))


def test_slots_past_the_count_are_left_alone(bank):
    host_bank, dbank = bank
    n, count = 7, 3
    patches = np.random.RandomState(5).randint(0, 256, size=(n, 240, 240, 3)).astype(np.uint8)
    recs = [r for _, r in GROUPS[2]]
    rows = A.label_rows(n, seed=8)
    d_count = torch.tensor([count], dtype=torch.int32, device='cuda')
    src = torch.from_numpy(patches).cuda()
    arena, out = _at_offset(n, 3, 5)
    plan = data.AugPlan(n, 'cuda')
    for t in (plan.params, plan.labels_i32, plan.bbox, plan.vertices, plan.labels):
        t.fill_(-7)
    params = torch.from_numpy(np.stack([A.to_row(r) for r in recs])).cuda()
    data.plan_augment(torch.from_numpy(rows).cuda(), d_count, data.Augment(gammas=GAMMAS).cfg(), params=params, out=plan)
    data.apply_augment(src, plan.params, d_count, dbank, out)
    torch.cuda.synchronize()
    want = A.plan(dict(A.CFG_DEFAULT), rows, count, params_in=recs)
    assert np.array_equal(plan.params.cpu().numpy()[:count], want['params']) and np.array_equal(plan.labels_i32.cpu().numpy()[:count], want['labels'])
    for t in (plan.params, plan.labels_i32, plan.bbox, plan.vertices, plan.labels):
        assert bool((t[count:] == -7).all())
    got = out.cpu().numpy()
    for s in range(count):
        assert np.array_equal(got[s], A.augment(patches[s], want['params'][s], host_bank)), s
    assert bool((out[count:] == SENTINEL).all()) and _untouched(arena, 5, patches.size)
    # a count above n is n; a negative count writes nothing
    d_count.fill_(100)
    data.apply_augment(src, params, d_count, dbank, out)
    torch.cuda.synchronize()
    assert np.array_equal(out[6].cpu().numpy(), A.augment(patches[6], recs[6], host_bank))
    out.fill_(SENTINEL)
    d_count.fill_(-1)
    data.apply_augment(src, params, d_count, dbank, out)
    data.plan_augment(torch.from_numpy(rows).cuda(), d_count, data.Augment(gammas=GAMMAS).cfg(), params=params, out=plan)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((plan.params[count:] == -7).all())


def _same_plan(plan, want, count):
    assert np.array_equal(plan.params.cpu().numpy()[:count], want['params'])
    assert np.array_equal(plan.labels_i32.cpu().numpy()[:count], want['labels'])
    bits = lambda t: np.ascontiguousarray(t.cpu().numpy()[:count]).view(np.uint32)     # noqa: E731
    assert np.array_equal(bits(plan.bbox), want['bbox'].view(np.uint32))
    assert np.array_equal(bits(plan.vertices), want['vertices'].view(np.uint32))
    assert np.array_equal(bits(plan.labels), want['label'].view(np.uint32))


@pytest.mark.parametrize('n', [1, 3, 7])
def test_records_and_labels_in_both_modes_and_the_counter(n):
    aug = data.Augment(flip=0.7, blur=0.8, curve=0.6, noise_p=0.7, gammas=GAMMAS, seed=31 + n)
    cfg = _cfg_dict(aug)
    rows = A.label_rows(n, seed=n)
    rows[0] = [40, 50, 240, 120, 42, 52, 236, 50, 240, 118, 40, 120]                   # a flip of this one is refused
    d_rows, d_count = torch.from_numpy(rows).cuda(), torch.tensor([n], dtype=torch.int32, device='cuda')
    state = torch.tensor([aug.seed, 5], dtype=torch.int64, device='cuda')
    seen = []
    for k in range(3):                                  # device mode: a launch per counter value
        plan = data.plan_augment(d_rows, d_count, aug.cfg(), state=state)
        torch.cuda.synchronize()
        assert state.tolist() == [aug.seed, 6 + k]
        want = A.plan(cfg, rows, n, seed=aug.seed, counter=5 + k)
        _same_plan(plan, want, n)
        seen.append(want['params'])
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    # injected mode: every record asks for the flip; the state is not touched
    recs = [dict(r, flags=1) for _, r in GROUPS[1][:n]]
    params = torch.from_numpy(np.stack([A.to_row(r) for r in recs])).cuda()
    plan = data.plan_augment(d_rows, d_count, aug.cfg(), params=params, state=state)
    torch.cuda.synchronize()
    want = A.plan(cfg, rows, n, params_in=recs)
    _same_plan(plan, want, n)
    assert want['params'][0, 0] == 2 and state.tolist() == [aug.seed, 8]


def test_augment_patches_front_end(bank):
    host_bank, _ = bank
    n = 3
    patches = np.random.RandomState(77).randint(0, 256, size=(n, 240, 240, 3)).astype(np.uint8)
    rows = A.label_rows(n, seed=12)
    aug = data.Augment(flip=1.0, blur=1.0, curve=1.0, noise_p=1.0, noise=(6, 12), gammas=GAMMAS, seed=9)
    out, lab_i32, bbox, vert, lab, params = data.augment_patches(patches, rows, augment=aug, counter=4)
    torch.cuda.synchronize()
    want = A.plan(_cfg_dict(aug), rows, n, seed=9, counter=4)
    assert np.array_equal(params.cpu().numpy(), want['params']) and np.array_equal(lab_i32.cpu().numpy(), want['labels'])
    assert np.array_equal(bbox.cpu().numpy(), want['bbox']) and np.array_equal(vert.cpu().numpy(), want['vertices'])
    assert np.array_equal(lab.cpu().numpy(), want['label'])
    for s in range(n):
        assert np.array_equal(out[s].cpu().numpy(), A.augment(patches[s], want['params'][s], host_bank)), s
    assert (want['params'][:, 1] > 0).all() and (want['params'][:, 7] >= 6).all()
    # injected: the same records give the same output
    again = data.augment_patches(patches, rows, augment=aug, params=want['params'])     # (a refused flip is then simply not asked for)
    assert torch.equal(again[0], out) and torch.equal(again[5][:, 1:], params[:, 1:])


def test_overlapping_input_and_output_is_refused(bank):
    _, dbank = bank
    arena = torch.zeros(4 * 240 * 240 * 3, dtype=torch.uint8, device='cuda')
    size = 3 * 240 * 240 * 3
    a = arena[:size].view(3, 240, 240, 3)
    params = torch.from_numpy(np.stack([A.to_row(A.record())] * 3)).cuda()
    count = torch.tensor([3], dtype=torch.int32, device='cuda')
    for off in (0, 1, 240 * 240 * 3):
        with pytest.raises(RuntimeError, match='overlap'):
            data.apply_augment(a, params, count, dbank, arena[off:off + size].view(3, 240, 240, 3))
    torch.cuda.synchronize()
    assert not arena.any()


BAND_RECORDS = {'flip + binomial 3 x 3': A.record(blur=1, flags=1), 'identity (the copy path)': A.record()}


@functools.lru_cache(maxsize=None)
def _band_case(c, kind):
    """(patch, restatement) of one slot through BAND_RECORDS[kind]: made once per c and kind, shared by the 16 offsets."""
    patch = np.random.RandomState(40 + c).randint(0, 256, size=(1, 240, 240, c)).astype(np.uint8)
    want = A.augment(patch[0], BAND_RECORDS[kind], A.gamma_bank(GAMMAS))
    want.setflags(write=False)
    return patch, want


@pytest.mark.parametrize('kind', sorted(BAND_RECORDS))
@pytest.mark.parametrize('out_off', range(16))
@pytest.mark.parametrize('c', [1, 2, 3, 4])
def test_the_band_store_at_every_destination_offset(bank, c, out_off, kind):
    """n = 1 (15 workgroups): patch_band_store's 16-byte words, dwords and bytes at every offset of the destination inside a 16-byte
    word, source at offset 33; the output is the restatement bit for bit and no byte outside the view is written."""
    patch, want = _band_case(c, kind)
    out, arena, _ = _launch(patch, [BAND_RECORDS[kind]], np.zeros((1, 12), np.int32), bank[1], in_off=33, out_off=out_off)
    assert out.data_ptr() % 16 == out_off
    bad = np.argwhere(out[0].cpu().numpy() != want)
    assert len(bad) == 0, (kind, c, out_off, len(bad), bad[:4].tolist())
    assert _untouched(arena, out_off, patch.size)
    assert (kind == 'identity (the copy path)') == np.array_equal(want, patch[0])


def _sampler(seed, n=7, **kw):
    frames, plates = _scene()
    return data.PatchSampler(frames, plates, n, oversample=4.0, neg_frac=0.2, seed=seed, augment=_augment(), **kw)


def test_three_eager_calls_equal_three_replays_of_one_captured_graph():
    a, b = _sampler(11), _sampler(11)
    a.launch()                                          # warm up outside the capture
    torch.cuda.synchronize()
    b.state.copy_(a.state)
    b.aug_state.copy_(a.aug_state)
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
    assert a.aug_state.tolist() == b.aug_state.tolist() == [23, 4] and a.state.tolist() == b.state.tolist() == [11, 4]


def test_a_sampler_batch_is_the_restatement_of_its_own_raw_patches(bank):
    host_bank, _ = bank
    s = _sampler(5)
    plain = data.PatchSampler(*_scene(), 7, oversample=4.0, neg_frac=0.2, seed=5)
    flags = set()
    for k in range(2):
        patches, bbox, vertices, labels, count = s.next_batch()
        raw_plain = plain.next_batch()
        assert count == 7 and patches is not s.raw
        assert torch.equal(s.raw, raw_plain[0]) and torch.equal(s.plan.bbox, raw_plain[1])      # the plan's draws do not depend on the augmenter
        rows = s.plan.labels_i32.cpu().numpy()
        want = A.plan(_cfg_dict(s.augment), rows, count, seed=23, counter=k)
        assert np.array_equal(s.aug_params.cpu().numpy(), want['params'])
        assert np.array_equal(s.aug.labels_i32.cpu().numpy(), want['labels'])
        bits = lambda t: t.cpu().numpy().view(np.uint32)                                           # noqa: E731
        assert np.array_equal(bits(bbox), want['bbox'].view(np.uint32)) and np.array_equal(bits(vertices), want['vertices'].view(np.uint32))
        assert np.array_equal(bits(labels), want['label'].view(np.uint32))
        raw, got = s.raw.cpu().numpy(), patches.cpu().numpy()
        for i in range(count):
            assert np.array_equal(got[i], A.augment(raw[i], want['params'][i], host_bank)), (k, i)
        flags |= set(want['params'][:, 0].tolist())
        assert not np.array_equal(got, raw)
    assert 1 in flags and 0 in flags


def test_net_loss_on_a_sampler_batch_equals_net_loss_on_the_restated_labels():
    net = D.DenseBoxLMLOC(synth.vgg19_standin(seed=0))
    synth.fill_params_(net, 11)
    net = net.cuda().eval()
    net.compute_dtype = 'f32'
    frames, plates = _scene()
    aug = data.Augment(flip=1.0, gammas=GAMMAS, seed=2)
    s = data.PatchSampler(frames, plates, 2, oversample=4.0, neg_frac=0.0, seed=3, augment=aug)
    patches, bbox, vertices, labels, count = s.next_batch()
    assert count == 2 and patches.dtype == torch.uint8 and tuple(patches.shape) == (2, 240, 240, 3)
    want = A.plan(_cfg_dict(aug), s.plan.labels_i32.cpu().numpy(), 2, seed=2, counter=0)
    assert (want['params'][:, 0] != 0).all() and (want['params'][:, 0] == 1).any()
    with torch.no_grad():
        outs = net(patches)
    got = net.loss(outs, bbox, vertices, labels, rng=np.random.RandomState(4))
    b2, v2, l2 = (torch.from_numpy(want[k]) for k in ('bbox', 'vertices', 'label'))
    ref = net.loss(outs, b2, v2, l2, rng=np.random.RandomState(4))
    assert torch.equal(bbox.cpu(), b2) and torch.equal(vertices.cpu(), v2) and torch.equal(labels.cpu(), l2)
    assert not torch.equal(s.plan.bbox.cpu(), b2)                                      # a flip moved the boxes
    assert float(got) > 0 and np.float32(float(got)).tobytes() == np.float32(float(ref)).tobytes()
