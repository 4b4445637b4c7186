"""Training patches on the GPU: dbx_patch_plan == the Python restatement (tests/patch_ref.py) bit for bit -- status, slot, labels,
job windows, count, tallies and the draws themselves -- in injected mode on the reference fixture and in device mode; every patch
dbx_patch_cut writes is bit for bit resize.crop_resize_batch on the planned window, every negative the frame's own pixels; the state
advances, reproduces and replays in a captured graph; a PatchSampler batch gives net.loss what collate_labels gives it."""
import gc
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patch_ref as R                                   # noqa: E402

import densebox_amd as D                                # noqa: E402
from densebox_amd import _lib, data, rectify, resize, synth   # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'patch_plan.npz')
SENTINEL = 0xA5
SIZES = [(97, 131), (300, 300), (260, 900), (1080, 1920)]            # (H, W)
JOB = np.dtype([('src', '<u8'), ('dst', '<u8'), ('scale_x', '<f8'), ('scale_y', '<f8'), ('row_bytes', '<i4'), ('cx0', '<i4'),
                ('cy0', '<i4'), ('cw', '<i4'), ('ch', '<i4'), ('pad_l', '<i4'), ('pad_t', '<i4'), ('vw', '<i4'), ('vh', '<i4'),
                ('dh', '<i4'), ('dw', '<i4'), ('pad_value', '<i4'), ('tiles_x', '<i4'), ('frame', '<i4'), ('kind', '<i4'),
                ('reserved', '<i4')])
assert JOB.itemsize == 96


def _plate(rs, W, H):
    w, h = int(rs.randint(4, min(200, W // 3) + 1)), int(rs.randint(4, min(80, H // 3) + 1))
    x, y = int(rs.randint(0, W - w)), int(rs.randint(0, H - h))
    pts = [(x, y), (x + w, y), (x + w, y + h), (x, y + h)]
    pts = [(min(max(px + int(rs.randint(-4, 5)), 0), W - 1), min(max(py + int(rs.randint(-4, 5)), 0), H - 1)) for px, py in pts]
    return [v for k in rs.permutation(4) for v in pts[k]]


def _scene(c, seed=3):
    """Frames of SIZES with c channels and 5 / 4 / 6 / 12 plates; frame 0 also holds a plate with two equal vertices and frame 1 one
    with a vertex outside the frame."""
    rs = np.random.RandomState(seed)
    frames = [rs.randint(0, 256, size=(h, w, c)).astype(np.uint8) for h, w in SIZES]
    plates = [[_plate(rs, w, h) for _ in range(k)] for (h, w), k in zip(SIZES, (5, 4, 6, 12))]
    plates[0].append([10, 10, 10, 10, 40, 30, 12, 31])
    plates[1].append([100, 100, 300, 100, 160, 120, 100, 121])
    return frames, plates


@pytest.fixture(scope='module')
def scene3():
    frames, plates = _scene(3)
    dev = [torch.from_numpy(f).cuda() for f in frames]
    rows, plate0 = data.plate_tables(plates, len(dev))
    return dict(frames=frames, dev=dev, plates=plates, rows=rows, plate0=plate0, table=rectify.frame_table(dev),
                d_rows=torch.from_numpy(rows).cuda(), d_plate0=torch.from_numpy(plate0).cuda())


def _check_plan(plan, want, srcs, sizes, c):
    """Every output of one launch against the restatement's dict."""
    torch.cuda.synchronize()
    count = int(plan.count.item())
    assert count == want['count']
    assert np.array_equal(plan.tally.cpu().numpy(), want['tally'])
    assert np.array_equal(plan.status.cpu().numpy(), want['status'])
    assert np.array_equal(plan.slot.cpu().numpy(), want['slot'])
    assert np.array_equal(plan.cand.cpu().numpy(), want['cand'])
    assert np.array_equal(plan.draws.cpu().numpy().view(np.uint64), want['draws'].view(np.uint64))
    assert np.array_equal(plan.labels_i32.cpu().numpy()[:count], want['labels'])
    bits = lambda t: np.ascontiguousarray(t.cpu().numpy()[:count]).view(np.uint32)     # noqa: E731
    assert np.array_equal(bits(plan.bbox), want['bbox'].view(np.uint32).reshape(count, 4))
    assert np.array_equal(bits(plan.vertices), want['vertices'].view(np.uint32).reshape(count, 8))
    assert np.array_equal(bits(plan.labels), want['label'].view(np.uint32).reshape(count, 1))
    jobs = plan.jobs.cpu().numpy().reshape(-1).view(JOB)[:count]
    win = want['windows']
    assert np.array_equal(np.stack([jobs['cx0'], jobs['cy0'], jobs['cx0'] + jobs['cw'], jobs['cy0'] + jobs['ch']], axis=1)
                          if count else np.zeros((0, 4), np.int32), win)
    assert np.array_equal(jobs['frame'], want['frames']) and np.array_equal(jobs['kind'], want['kinds'])
    assert np.array_equal(jobs['src'], np.array([srcs[f] for f in want['frames']], dtype=np.uint64))
    assert np.array_equal(jobs['row_bytes'], np.array([sizes[f][1] * c for f in want['frames']], dtype=np.int32))
    assert np.array_equal(jobs['scale_x'], (win[:, 2] - win[:, 0]) / 240.0) and np.array_equal(jobs['scale_y'], (win[:, 3] - win[:, 1]) / 240.0)
    for k, v in (('vw', jobs['cw']), ('vh', jobs['ch']), ('dh', 240), ('dw', 240), ('tiles_x', 4), ('pad_l', 0), ('pad_t', 0), ('pad_value', 0)):
        assert np.all(jobs[k] == v), k
    # rows at or past the count were not written (PatchPlan starts zeroed)
    assert not plan.labels_i32[count:].any() and not plan.jobs[count:].any() and not plan.bbox[count:].any()
    return count


@pytest.fixture(scope='module')
def fixture_tables():
    """The whole reference fixture as ONE scene: a frame per case (the plan reads only the sizes of the frame records, so they share
    one small buffer as their source), the positives' plates and the negatives' plates in frame order."""
    g = np.load(GOLDEN)
    npos, nneg = len(g['pos_status']), len(g['neg_status'])
    sizes = [(int(h), int(w)) for w, h in g['pos_size']] + [(int(h), int(w)) for w, h in g['neg_size']]
    rows = [[i] + g['pos_verts'][i].tolist() for i in range(npos)]
    cand = [[0, i] for i in range(npos)]
    for j in range(nneg):
        rows += [[npos + j] + p.tolist() for p in g['neg_plates'][j][:g['neg_nplates'][j]]]
        cand.append([1, npos + j])
    rows = np.asarray(rows, dtype=np.int32)
    draws = np.concatenate([g['pos_draws'], g['neg_centre'].astype(np.float64)])
    # one candidate order that interleaves kinds and statuses
    order = np.random.RandomState(0).permutation(npos + nneg)
    cand, draws = np.asarray(cand, dtype=np.int32)[order], np.ascontiguousarray(draws[order])
    expect = np.concatenate([g['pos_status'], g['neg_status']])[order]
    th0 = np.concatenate([np.zeros(npos, np.int32), g['neg_th']])[order] == 0
    rows, plate0 = data.plate_tables(rows, len(sizes))
    dummy = torch.zeros(64, dtype=torch.uint8, device='cuda')
    rec = (_lib.CropFrame * len(sizes))()
    for r, (h, w) in zip(rec, sizes):
        r.src, r.sh, r.sw = dummy.data_ptr(), h, w
    table = torch.frombuffer(rec, dtype=torch.uint8).cuda()
    return dict(sizes=sizes, rows=rows, plate0=plate0, cand=cand, draws=draws, expect=expect, th0=th0, table=table, dummy=dummy,
                d_rows=torch.from_numpy(rows).cuda(), d_plate0=torch.from_numpy(plate0).cuda())


@pytest.mark.parametrize('M,n', [(M, n) for M in (1, 63, 64, 65, 1025, 4096) for n in (1, 7, 64)] + [(4096, 4096)],
                         ids=lambda v: str(v))
def test_plan_injected_on_the_reference_fixture(fixture_tables, M, n):
    """The fixture's 2 500 candidates, repeated up to 4 096 (more candidates than threads); n = 4096 keeps every label row.  th = 0 here:
    the fixture's negatives with another TH are pinned through dbx_patch_plan_host."""
    T = fixture_tables
    reps = -(-M // len(T['cand']))
    cand, draws = np.tile(T['cand'], (reps, 1))[:M], np.tile(T['draws'], (reps, 1))[:M]
    expect, th0 = np.tile(T['expect'], reps)[:M], np.tile(T['th0'], reps)[:M]
    plan = data.plan_patches(T['table'], len(T['sizes']), 3, T['d_rows'], T['d_plate0'], M, n,
                             cand=torch.from_numpy(cand).cuda(), draws=torch.from_numpy(draws).cuda())
    want = R.plan(T['sizes'], T['rows'], T['plate0'], M, n, cand=cand, draws=draws)
    count = _check_plan(plan, want, [T['dummy'].data_ptr()] * len(T['sizes']), T['sizes'], 3)
    got = plan.status.cpu().numpy()
    seen = np.where(got == 7, 0, got)
    assert np.array_equal(seen[th0], expect[th0])                      # what the reference itself returned
    assert count == min(n, int((seen == 0).sum()))
    if M >= 1025:
        assert ((got == 7).sum() > 0) == (n < 4096) and {0, 1, 2, 6} <= set(seen.tolist()) and (M < 4096 or 3 in seen)


@pytest.mark.parametrize('M', [1, 63, 64, 65, 1025, 4096])
@pytest.mark.parametrize('n', [1, 7, 64])
def test_plan_device_mode_equals_the_restated_hash(scene3, M, n):
    S = scene3
    seed, counter = 1234 + M, 7 * n
    state = torch.tensor([seed, counter], dtype=torch.int64, device='cuda')
    plan = data.plan_patches(S['table'], 4, 3, S['d_rows'], S['d_plate0'], M, n, state=state, neg_frac=0.25)
    want = R.plan(SIZES, S['rows'], S['plate0'], M, n, seed=seed, counter=counter, neg_frac=0.25)
    _check_plan(plan, want, [d.data_ptr() for d in S['dev']], SIZES, 3)
    assert state.tolist() == [seed, counter + 1]
    # and the exported draws, injected, give the same plan
    again = data.plan_patches(S['table'], 4, 3, S['d_rows'], S['d_plate0'], M, n, cand=plan.cand, draws=plan.draws)
    for k in ('status', 'slot', 'labels_i32', 'count', 'tally', 'jobs'):
        assert torch.equal(getattr(again, k), getattr(plan, k)), k
    if M >= 1025:
        st = want['status']
        assert (st == 7).any() and {0, 1, 2, 4, 5, 6} <= set(st.tolist())      # every path of the scene was taken


def test_plan_all_rejected_and_no_candidates(scene3):
    S = scene3
    corner = [[[0, 0, 6, 0, 6, 4, 0, 4]], [[0, 0, 6, 0, 6, 4, 0, 4]], [], []]       # the landmark rule rejects a plate in the corner
    rows, plate0 = data.plate_tables(corner, 4)
    state = torch.tensor([9, 0], dtype=torch.int64, device='cuda')
    d_rows, d_plate0 = torch.from_numpy(rows).cuda(), torch.from_numpy(plate0).cuda()
    plan = data.plan_patches(S['table'], 4, 3, d_rows, d_plate0, 65, 7, state=state, neg_frac=0.0)
    _check_plan(plan, R.plan(SIZES, rows, plate0, 65, 7, seed=9, counter=0, neg_frac=0.0), [d.data_ptr() for d in S['dev']], SIZES, 3)
    assert int(plan.count.item()) == 0 and plan.tally.tolist() == [0, 65, 0, 0, 0, 0, 0, 0]
    patches = torch.full((7, 240, 240, 3), SENTINEL, dtype=torch.uint8, device='cuda')
    data.cut_patches(plan, 3, patches)
    assert bool((patches == SENTINEL).all())
    plan.count.fill_(5)                                                  # M == 0 writes count = 0 and a zero tally
    data.plan_patches(S['table'], 4, 3, d_rows, d_plate0, 0, 7, state=state, out=plan)
    assert int(plan.count.item()) == 0 and plan.tally.tolist() == [0] * 8 and state.tolist() == [9, 2]
    # no plates at all: every candidate is a negative
    e_rows, e_plate0 = data.plate_tables([[], [], [], []], 4)
    plan = data.plan_patches(S['table'], 4, 3, torch.from_numpy(e_rows).cuda(), torch.from_numpy(e_plate0).cuda(), 64, 64, state=state)
    want = R.plan(SIZES, e_rows, e_plate0, 64, 64, seed=9, counter=2)
    _check_plan(plan, want, [d.data_ptr() for d in S['dev']], SIZES, 3)
    assert set(want['cand'][:, 0].tolist()) == {1} and want['count'] > 0


@pytest.mark.parametrize('c', [3, 1])
def test_cut_is_bitwise_crop_resize_batch_at_an_odd_offset(c):
    frames, plates = _scene(c, seed=5 + c)
    n, M = 64, 80
    patches0, plan = data.sample_patches(frames, plates, n, neg_frac=0.3, seed=21, m=M)
    torch.cuda.synchronize()
    count = int(plan.count.item())
    rows, plate0 = data.plate_tables(plates, 4)
    want = R.plan(SIZES, rows, plate0, M, n, seed=21, counter=0, neg_frac=0.3)
    assert count == want['count'] and 8 < count < n and (want['kinds'] == 1).sum() >= 2 and (want['kinds'] == 0).sum() >= 8
    assert np.array_equal(plan.status.cpu().numpy(), want['status'])
    # the same jobs again into a tensor at an odd byte offset inside a prefilled arena
    size = n * 240 * 240 * c
    arena = torch.full((size + 64,), SENTINEL, dtype=torch.uint8, device='cuda')
    odd = arena[33:33 + size].view(n, 240, 240, c)
    assert odd.data_ptr() % 2 == 1
    data.cut_patches(plan, c, odd)
    torch.cuda.synchronize()
    assert torch.equal(odd[:count], patches0[:count])
    assert bool((odd[count:] == SENTINEL).all()) and bool((arena[:33] == SENTINEL).all()) and bool((arena[33 + size:] == SENTINEL).all())
    assert not patches0[count:].any()
    # every patch is crop_resize_batch on its planned window (image-then-window order), every negative the frame's own pixels
    windows = [[tuple(int(v) for v in want['windows'][s]) for s in range(count) if want['frames'][s] == f] for f in range(4)]
    ref = resize.crop_resize_batch(frames, windows)
    order = [s for f in range(4) for s in range(count) if want['frames'][s] == f]
    assert torch.equal(odd[order], ref)
    got = odd.cpu().numpy()
    for s in range(count):
        if want['kinds'][s] == 1:
            x0, y0, x1, y1 = want['windows'][s]
            assert np.array_equal(got[s], frames[want['frames'][s]][y0:y1, x0:x1])


def _sampler(seed, n=16, **kw):
    frames, plates = _scene(3)
    return data.PatchSampler(frames, plates, n, oversample=4.0, neg_frac=0.2, seed=seed, **kw)


def _snap(batch):
    patches, bbox, vertices, labels, count = batch
    return patches.clone(), bbox.clone(), vertices.clone(), labels.clone(), count


def test_state_advances_and_reproduces():
    a, b = _sampler(5), _sampler(5)
    a1, a2 = _snap(a.next_batch()), _snap(a.next_batch())
    b1, b2 = _snap(b.next_batch()), _snap(b.next_batch())
    assert a1[4] == 16 and not torch.equal(a1[0], a2[0]) and not torch.equal(a1[1], a2[1])
    for x, y in ((a1, b1), (a2, b2)):
        assert all(torch.equal(p, q) for p, q in zip(x[:4], y[:4])) and x[4] == y[4]
    assert a.state.tolist() == [5, 2]
    c = _sampler(6)
    assert not torch.equal(_snap(c.next_batch())[0], a1[0])
    c.state.copy_(torch.tensor([5, 1]))                                    # the same seed and counter: the same batch
    c2 = _snap(c.next_batch())
    assert all(torch.equal(p, q) for p, q in zip(c2[:4], a2[:4]))
    tally = a.status_tally()
    assert sum(tally.values()) == 2 * a.M and tally['accepted'] + tally['accepted beyond the capacity'] >= 32


def test_graph_replay_equals_eager_calls_from_a_copy_of_the_state():
    a, b = _sampler(11), _sampler(11)
    a.launch()                                                             # warm up outside the capture
    torch.cuda.synchronize()
    b.state.copy_(a.state)
    g = torch.cuda.CUDAGraph()
    gc.collect()
    with torch.cuda.graph(g):
        a.launch()
    seen = []
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        got = (a.patches.clone(), a.plan.bbox.clone(), a.plan.vertices.clone(), a.plan.labels.clone(), int(a.plan.count.item()))
        want = _snap(b.next_batch())
        assert all(torch.equal(p, q) for p, q in zip(got[:4], want[:4])) and got[4] == want[4] == 16, k
        assert all(not torch.equal(got[0], s) for s in seen)
        seen.append(got[0])
    assert a.state.tolist() == b.state.tolist() == [11, 4]


def test_sampler_batch_gives_net_loss_what_collate_labels_gives_it():
    net = D.DenseBoxLMLOC(synth.vgg19_standin(seed=0))
    synth.fill_params_(net, 11)
    net = net.cuda().eval()
    net.compute_dtype = 'f32'
    frames, plates = _scene(3)
    s = data.PatchSampler(frames, plates, 2, oversample=4.0, neg_frac=0.0, seed=3)
    patches, bbox, vertices, labels, count = s.next_batch()
    assert count == 2 and patches.dtype == torch.uint8 and tuple(patches.shape) == (2, 240, 240, 3)
    with torch.no_grad():
        outs = net(patches)
    got = net.loss(outs, bbox, vertices, labels, rng=np.random.RandomState(4))
    names = [R.label_name(r) for r in s.plan.labels_i32.cpu().numpy()]
    b2, v2, l2 = data.collate_labels(names)
    want = net.loss(outs, b2, v2, l2, rng=np.random.RandomState(4))
    assert torch.equal(bbox.cpu(), b2) and torch.equal(vertices.cpu(), v2) and torch.equal(labels.cpu(), l2)
    assert float(got) > 0 and np.float32(float(got)).tobytes() == np.float32(float(want)).tobytes()


def test_next_batch_raises_on_a_short_batch():
    frames, _ = _scene(3)
    corner = [[[0, 0, 6, 0, 6, 4, 0, 4]], [], [], []]
    s = data.PatchSampler(frames, corner, 4, oversample=2.0, neg_frac=0.0, seed=1)
    with pytest.raises(RuntimeError, match='fewer than n=4'):
        s.next_batch()
    assert s.next_batch(allow_short=True)[4] == 0
    assert data.PatchSampler(frames, corner, 4, oversample=2.0, neg_frac=0.0, seed=1, allow_short=True).next_batch()[4] == 0
    assert s.status_tally()['landmark rule'] == 16                     # 2 batches of 8 candidates
