"""The training patch warp without a GPU: hand-computed pixel values (ramps, steps, corner dots) pin the NumPy restatement
(tests/warp_aug_ref.py); the restated solve and the restated zero-border pixels equal the oracle's cv2 restatement bit for bit; the host
exports dbx_patch_warp_params_host / dbx_patch_warp_host (the kernels' own __host__ __device__ functions) equal the restatement bit for
bit -- records, refusal bits, labels, both matrices and pixels, in injected and in device mode; and the default Warp leaves at least half
of the golden plan's accepted positives warped."""
import os
import sys

import numpy as np
import pytest

from oracle import densebox_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_aug_ref as W                                # noqa: E402

from warp_host import host_plan, host_warp, same_plan  # noqa: E402

from densebox_amd import data                           # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'patch_plan.npz')


def _both(patch, rec):
    """The restatement's and the host export's output of one injected record on a negative slot; they must agree."""
    want = W.plan(W.CFG_DEFAULT, np.zeros((1, 12), np.int32), 1, params_in=[rec])
    got = host_plan({}, np.zeros((1, 12), np.int32), 1, params_in=[rec])
    same_plan(got, want)
    a, b = W.warp(patch, want['params'][0], want['inv'][0]), host_warp(patch, got['params'][0], got['inv'][0])
    assert np.array_equal(a, b)
    return a, int(want['params'][0, 0])


def _ramp(c=3):
    """Every pixel differs from its neighbours: x in channel 0, y in channel 1, a step at x = 100 and four corner dots in channel 2."""
    img = np.zeros((240, 240, c), np.uint8)
    img[..., 0] = np.arange(240)[None, :]
    if c > 1:
        img[..., 1] = np.arange(240)[:, None]
    if c > 2:
        img[:, 100:, 2] = 200
        for y, x in ((0, 0), (0, 239), (239, 239), (239, 0)):
            img[y, x, 2] = 255 - 10 * (y // 239) - 20 * (x // 239)
    return img


@pytest.mark.parametrize('border', [0, 1])
def test_the_identity_quad_is_a_copy(border):
    img = _ramp()
    out, flags = _both(img, W.record(border=border, fill=W.pack_fill(9, 9, 9)))
    assert flags == 1 and np.array_equal(out, img)
    out, flags = _both(img, W.record(W.shifted(48, 0), flags=0))       # not asked for: a copy whatever the quad
    assert flags == 0 and np.array_equal(out, img)


def test_an_integer_shift_by_hand_with_both_borders():
    img = _ramp()
    fill = W.pack_fill(7, 77, 177)
    out, flags = _both(img, W.record(W.shifted(48, 0), border=0, fill=fill))
    assert flags == 1
    assert np.array_equal(out[:, 3:], img[:, :-3])                     # input pixel x lands on output pixel x + 3
    assert (out[:, :3] == np.array([7, 77, 177], np.uint8)).all()
    out, _ = _both(img, W.record(W.shifted(48, 0), border=1, fill=fill))
    assert np.array_equal(out[:, 3:], img[:, :-3])
    assert np.array_equal(out[:, :3], np.repeat(img[:, :1], 3, axis=1))     # the edge pixel, not the fill
    # down and to the left
    out, _ = _both(img, W.record(W.shifted(-80, 32), border=0, fill=0))
    assert np.array_equal(out[2:, :-5], img[:-2, 5:]) and not out[:2].any() and not out[:, -5:].any()


def test_a_half_pixel_shift_is_the_rounded_mean_of_two_neighbours():
    img = np.random.RandomState(3).randint(0, 256, size=(240, 240, 3)).astype(np.uint8)
    out, _ = _both(img, W.record(W.shifted(8, 0), border=1))
    p0 = np.concatenate([img[:, :1], img[:, :-1]], axis=1).astype(np.int64)        # in(x - 1), the edge replicated
    assert np.array_equal(out, ((p0 + img + 1) >> 1).astype(np.uint8))
    out, _ = _both(img, W.record(W.shifted(8, 0), border=0, fill=W.pack_fill(100, 100, 100)))
    p0[:, 0] = 100
    assert np.array_equal(out, ((p0 + img + 1) >> 1).astype(np.uint8))


def test_a_quad_wholly_outside_gives_the_fill_or_the_edge():
    img = _ramp(4)
    img[..., 3] = 50
    fill = W.pack_fill(1, 2, 3, 250)
    out, flags = _both(img, W.record(W.shifted(16 * 600, 0), border=0, fill=fill))
    assert flags == 1 and (out == np.array([1, 2, 3, 250], np.uint8)).all()
    out, _ = _both(img, W.record(W.shifted(16 * 600, 0), border=1, fill=fill))
    assert np.array_equal(out, np.repeat(img[:, :1], 240, axis=1))     # column 0 everywhere
    out, _ = _both(img, W.record(W.shifted(-16 * 600, -16 * 300), border=1, fill=fill))
    assert (out == img[239, 239]).all()                                # the corner dot


def _seeded_quads(n, seed, spread=400):
    rs = np.random.RandomState(seed)
    return [[int(v) for v in np.array(W.IDENTITY_QUAD) + rs.randint(-spread, spread + 1, size=8)] for _ in range(n)]


def test_the_restated_solve_is_the_oracle_s_bit_for_bit():
    for quad in _seeded_quads(40, 1) + [q for _, q in W.CASES[:12]]:
        dst = [q / 16.0 for q in quad]
        assert all(np.float32(v) == v for v in dst)                    # the oracle rounds its input to float32: exact here
        m = W.solve(W.SQUARE, dst)
        want = O.get_perspective_matrix(np.array(W.SQUARE).reshape(4, 2), np.array(dst).reshape(4, 2))
        assert np.array_equal(np.array(m).view(np.uint64), want.reshape(9).view(np.uint64)), quad


@pytest.mark.parametrize('c', [1, 3])
def test_the_restated_zero_border_pixels_are_the_oracle_s_bit_for_bit(c):
    img = np.random.RandomState(c).randint(0, 256, size=(240, 240, c)).astype(np.uint8)
    for quad in _seeded_quads(3, 2 + c) + [q for n, q in W.CASES if n in ('rot_+15', 'strong_keystone', 'shift_frac')]:
        m, im = W.matrices(quad)
        got = W.warp(img, W.record(quad, border=0, fill=0), im)
        assert np.array_equal(got, O.warp_perspective_u8(img, np.array(m).reshape(3, 3), (240, 240))), quad
        assert not np.array_equal(got, img)


def _positive(x0=80, y0=90, x1=160, y1=130):
    return [x0, y0, x1, y1, x0, y0, x1, y0, x1, y1, x0, y1]


def _pixels_agree(patches, plan_rows, slots):
    for s in slots:
        patch = patches[s % len(patches)]
        want = W.warp(patch, plan_rows['params'][s], plan_rows['inv'][s])
        assert np.array_equal(host_warp(patch, plan_rows['params'][s], plan_rows['inv'][s]), want), s
        if not plan_rows['params'][s, 0] & 1:
            assert np.array_equal(want, patch)


@pytest.mark.parametrize('c', [1, 3, 4])
@pytest.mark.parametrize('border', [0, 1])
def test_host_exports_equal_the_restatement_on_the_shared_cases(c, border):
    """Injected mode, count = 16: every shared case on a positive slot (some refused, some degenerate) and pixels for all of them."""
    fill = W.pack_fill(11, 22, 33, 44)
    recs = [W.record(q, border=border, fill=fill, rot=5, scale=300, aspect=200, shear=-9, reserved=77) for _, q in W.CASES]
    rows = np.array([_positive()] * len(recs), np.int32)
    want = W.plan(W.CFG_DEFAULT, rows, len(recs), params_in=recs)
    got = host_plan({}, rows, len(recs), params_in=recs)
    same_plan(got, want)
    flags = dict(zip([n for n, _ in W.CASES], want['params'][:, 0].tolist()))
    assert flags['identity'] == 1 and flags['rot_+15'] == 1 and flags['scale_0.85'] == 1 and flags['jitter_keystone'] == 1
    assert flags['outside'] == 2 and flags['degenerate_equal_corners'] == 4 and flags['degenerate_collinear'] == 4
    assert (want['params'][:, 3] == 5).all() and (want['params'][:, 12:15] == [300, 200, -9]).all() and not want['params'][:, 15].any()
    eye = np.array(W.EYE)
    for s in np.flatnonzero(want['params'][:, 0] != 1):
        assert np.array_equal(want['fwd'][s], eye) and np.array_equal(want['inv'][s], eye) and np.array_equal(want['labels'][s], rows[s])
    patches = np.random.RandomState(10 * c + border).randint(0, 256, size=(2, 240, 240, c)).astype(np.uint8)
    _pixels_agree(patches, got, range(len(recs)))


def test_sanitising_and_refusal_bits_on_input():
    q = W.shifted(16, 16)
    recs = [W.record(q, flags=3), W.record(q, flags=6), W.record(q, flags=-1, border=2), W.record(q, border=-1),
            W.record([1 << 24, -(1 << 24)] + q[2:], flags=1), W.record(q, flags=4)]
    rows = np.zeros((len(recs), 12), np.int32)
    want = W.plan(W.CFG_DEFAULT, rows, len(recs), params_in=recs)
    same_plan(host_plan({}, rows, len(recs), params_in=recs), want)
    assert want['params'][:, 0].tolist() == [1, 0, 1, 1, 1, 0]         # flags & 1 on input; (the clamped quad still solves)
    assert want['params'][:, 1].tolist() == [0, 0, 0, 0, 0, 0]
    assert want['params'][4, 4:6].tolist() == [1 << 20, -(1 << 20)]


def test_the_label_rule_by_hand():
    """A pure translation by (+16, -8) pixels moves every label by that; the margin is inclusive; W <= 0 at a vertex, a non-convex quad
    and label coordinates above 239 are refused."""
    q = W.shifted(256, -128)
    inside = _positive(8, 16, 215, 100)                 # lands on x = 24 .. 231, y = 8 .. 92: on the margin on three sides
    past_x = _positive(8, 16, 216, 100)                 # 232 > 239 - 8
    past_y = _positive(8, 15, 215, 100)                 # 7 < 8
    above = _positive(100, 100, 240, 140)               # the plan's 240 on the right edge
    rows = np.array([inside, past_x, past_y, above, _positive(), [0] * 12], np.int32)
    recs = [W.record(q)] * 4 + [W.record(dict(W.CASES)['non_convex']), W.record(q)]
    want = W.plan(W.CFG_DEFAULT, rows, 6, params_in=recs)
    same_plan(host_plan({}, rows, 6, params_in=recs), want)
    assert want['params'][:, 0].tolist() == [1, 2, 2, 2, 2, 1]
    assert want['labels'][0].tolist() == [24, 8, 231, 92, 24, 8, 231, 8, 231, 92, 24, 92]
    assert want['bbox'][0].tolist() == [6.0, 2.0, 57.75, 23.0] and want['label'].reshape(-1).tolist() == [1, 1, 1, 1, 1, 0]
    assert np.array_equal(want['labels'][1:], rows[1:])
    assert not np.array_equal(want['fwd'][5], np.array(W.EYE))         # the negative is warped, its row stays zero
    # margin 0 lets the two near misses through; a margin of 9 refuses the first as well
    want0 = W.plan(dict(W.CFG_DEFAULT, margin=0), rows, 4, params_in=recs[:4])
    same_plan(host_plan(dict(margin=0), rows, 4, params_in=recs[:4]), want0)
    assert want0['params'][:, 0].tolist() == [1, 1, 1, 2]
    want9 = W.plan(dict(W.CFG_DEFAULT, margin=9), rows, 1, params_in=recs[:1])
    same_plan(host_plan(dict(margin=9), rows, 1, params_in=recs[:1]), want9)
    assert want9['params'][0, 0] == 2
    # a concave quad's horizon crosses the patch: W is 1 at corner (0, 0) and negative around the corner that was folded inwards
    horizon = dict(W.CASES)['non_convex']
    m, _ = W.matrices(horizon)
    far = _positive(20, 20, 230, 230)
    assert m[6] * 230 + m[7] * 230 + m[8] < 0 < m[6] * 20 + m[7] * 20 + m[8]
    rows2 = np.array([far], np.int32)
    want2 = W.plan(dict(W.CFG_DEFAULT, margin=0), rows2, 1, params_in=[W.record(horizon)])
    same_plan(host_plan(dict(margin=0), rows2, 1, params_in=[W.record(horizon)]), want2)
    assert want2['params'][0, 0] == 2 and np.array_equal(want2['labels'][0], far)


def _golden_rows():
    z = np.load(GOLDEN)
    rows = z['pos_labels'][z['pos_status'] == 0]
    assert rows.shape == (1638, 12) and rows.max() == 570
    return rows


@pytest.mark.parametrize('count', [1, 7, 300])
@pytest.mark.parametrize('mode', ['device', 'injected'])
def test_host_exports_equal_the_restatement_on_plan_rows_in_both_modes(count, mode):
    """The fixture's accepted positives (coordinates up to 570) with every fifth slot a negative."""
    rows = _golden_rows()[100:100 + count].copy()
    rows[4::5] = 0
    warp = data.Warp(seed=12 + count)
    bank = W.rot_bank(-15, 15)
    assert np.array_equal(warp.bank(), bank)
    cfg = {k: getattr(warp.cfg(), k) for k in W.CFG_DEFAULT}
    assert cfg == W.CFG_DEFAULT
    if mode == 'device':
        want = W.plan(cfg, rows, count, bank=bank, seed=warp.seed, counter=3)
        got = host_plan(cfg, rows, count, bank=bank, seed=warp.seed, counter=3)
        other = W.plan(cfg, rows, count, bank=bank, seed=warp.seed, counter=4)
        assert not np.array_equal(other['params'], want['params'])
    else:
        rs = np.random.RandomState(count)
        recs = [W.record(W.CASES[rs.randint(len(W.CASES))][1] if rs.randint(3) == 0 else _seeded_quads(1, 100 + s, 200)[0],
                         flags=int(rs.randint(8)), border=int(rs.randint(-1, 3)), fill=W.pack_fill(*rs.randint(0, 256, size=4)))
                for s in range(count)]
        want = W.plan(cfg, rows, count, params_in=recs)
        got = host_plan(cfg, rows, count, params_in=recs)
    same_plan(got, want)
    if count == 300:
        seen = set(want['params'][:, 0].tolist())
        assert {0, 1, 2} <= seen, seen
    patches = np.random.RandomState(count).randint(0, 256, size=(3, 240, 240, 3)).astype(np.uint8)
    slots = set(range(0, count, 41)) | {int(np.flatnonzero(want['params'][:, 0] == f)[0]) for f in set(want['params'][:, 0].tolist())}
    _pixels_agree(patches, got, sorted(slots))


def test_a_slot_that_is_off_in_device_mode_gets_the_identity_quad_and_its_drawn_fields():
    cfg = dict(W.CFG_DEFAULT, p_warp=0.5)
    bank = W.rot_bank(-15, 15)
    rows = np.zeros((64, 12), np.int32)
    want = W.plan(cfg, rows, 64, bank=bank, seed=7, counter=0)
    same_plan(host_plan(cfg, rows, 64, bank=bank, seed=7, counter=0), want)
    off = want['params'][want['params'][:, 0] == 0]
    assert 8 < len(off) < 56 and (off[:, 4:12] == np.array(W.IDENTITY_QUAD)).all()
    assert len(set(off[:, 3].tolist())) > 3 and len(set(off[:, 12].tolist())) > 3          # rot and scale as drawn
    # p_warp = 0 never reads the bank: none is needed
    want = W.plan(dict(cfg, p_warp=0.0), rows, 8, bank=None, seed=7, counter=0)
    same_plan(host_plan(dict(p_warp=0.0), rows, 8, bank=None, seed=7, counter=0), want)
    assert not want['params'][:, 0].any()


def test_at_least_half_of_the_golden_positives_end_up_warped():
    """Keeps 'everything refused, so everything trivially equal' from passing: the default Warp in device mode on the fixture's 1 638
    accepted positives (as slots 0 .. 1637 of one launch)."""
    rows = _golden_rows()
    warp = data.Warp()
    bank = warp.bank()
    cfg = {k: getattr(warp.cfg(), k) for k in W.CFG_DEFAULT}
    got = host_plan(cfg, rows, len(rows), bank=bank, seed=warp.seed, counter=0)
    want = W.plan(cfg, rows, len(rows), bank=bank, seed=warp.seed, counter=0)
    same_plan(got, want)
    warped = int((got['params'][:, 0] & 1).sum())
    print('warped %d of %d, refused %d, degenerate %d' % (warped, len(rows), int((got['params'][:, 0] == 2).sum()),
                                                         int((got['params'][:, 0] == 4).sum())))
    assert 2 * warped >= len(rows)
    assert not (got['params'][:, 0] == 4).any()
    moved = got['params'][:, 0] == 1
    assert not np.array_equal(got['labels'][moved], rows[moved])
