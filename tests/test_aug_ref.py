"""The patch augmentation's restatement (tests/aug_ref.py) against values computed by hand, and the exported host functions
(dbx_patch_aug_params_host, dbx_patch_augment_host: the kernels' own __host__ __device__ code) against the restatement, bit for bit.
No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug_ref as A                                     # noqa: E402
import patch_ref as R                                   # noqa: E402

from densebox_amd import _lib, data                     # noqa: E402


def _ramp():
    """Channel 0 = x, channel 1 = y, channel 2 = 255 - x."""
    y, x = np.mgrid[0:240, 0:240]
    return np.stack([x, y, 255 - x], axis=2).astype(np.uint8)


def _random_patch(c, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(240, 240, c)).astype(np.uint8)


def test_identity_returns_the_input():
    for c in (1, 2, 3, 4):
        p = _random_patch(c, c)
        assert np.array_equal(A.augment(p, A.record()), p)
    assert np.array_equal(A.augment(_ramp(), A.record(curve=5), curves=A.gamma_bank((0.5,))), _ramp())      # a curve outside the bank is none


def test_flip_twice_returns_pixels_and_labels():
    p = _random_patch(4, 9)
    f = A.augment(p, A.record(flags=1))
    assert np.array_equal(f, p[:, ::-1]) and np.array_equal(A.augment(f, A.record(flags=1)), p)
    row = [40, 50, 200, 120, 42, 52, 199, 50, 200, 118, 40, 120]
    once = A.flip_labels(row)
    assert once == [39, 50, 199, 120, 40, 50, 197, 52, 199, 120, 39, 118]              # by hand: lu' = (239 - ru.x, ru.y), ...
    assert A.flip_labels(once) == row
    ramp = A.augment(_ramp(), A.record(flags=1))
    assert ramp[7, 0].tolist() == [239, 7, 16] and ramp[7, 239].tolist() == [0, 7, 255] and ramp[200, 100].tolist() == [139, 200, 116]


def test_a_label_of_240_refuses_the_flip():
    rows = np.array([[40, 50, 240, 120, 42, 52, 236, 50, 240, 118, 40, 120],            # bbox and rd on the right edge
                     [40, 50, 200, 120, 42, 52, 199, 50, 200, 118, 40, 120],
                     [0] * 12], dtype=np.int32)
    assert A.flip_labels(rows[0]) is None
    got = A.plan(dict(A.CFG_DEFAULT), rows, 3, params_in=[A.record(flags=1)] * 3)
    assert got['params'][:, 0].tolist() == [2, 1, 1]                                   # refused, applied, applied (a negative flips its pixels)
    assert np.array_equal(got['labels'][0], rows[0]) and got['labels'][1].tolist() == [39, 50, 199, 120, 40, 50, 197, 52, 199, 120, 39, 118]
    assert not got['labels'][2].any() and got['label'].reshape(-1).tolist() == [1.0, 1.0, 0.0]
    assert got['bbox'][1].tolist() == [9.75, 12.5, 49.75, 30.0]
    # the refused slot's pixels are not mirrored either
    p = _random_patch(3, 1)
    assert np.array_equal(A.augment(p, got['params'][0]), p) and np.array_equal(A.augment(p, got['params'][1]), p[:, ::-1])


def test_blur_values_by_hand_on_the_ramp():
    """Replicated edges and one rounding: every value below was worked out on paper from the weights (channel 0 = x, 1 = y, 2 = 255 - x).
    E.g. binomial 5 x 5 at column 0 of channel 0: the row taps are (0, 0, 0, 1, 2) . (1, 4, 6, 4, 1) = 6, all five rows alike: 6 * 16 = 96,
    (96 + 128) >> 8 = 0 (a mirrored edge would give 1); box 9 at column 0: 0 + 0 + 0 + 0 + 0 + 1 + 2 + 3 + 4 = 10, (20 + 9) / 18 = 1."""
    ramp = _ramp()
    b3 = A.augment(ramp, A.record(blur=1))
    b5 = A.augment(ramp, A.record(blur=2))
    for b in (b3, b5):                                  # a linear ramp is a fixed point, edges included (x: 0 -> 0, 239 -> 239)
        for y in (0, 1, 16, 100, 238, 239):
            for x in (0, 1, 2, 120, 237, 238, 239):
                assert b[y, x].tolist() == [x, y, 255 - x], (y, x)
    # columns of pixel values that are NOT a ramp: a step at x = 120 (0 -> 160) in channel 0
    step = np.zeros((240, 240, 1), np.uint8)
    step[:, 120:] = 160
    s3, s5 = A.augment(step, A.record(blur=1)), A.augment(step, A.record(blur=2))
    assert s3[5, 118:122, 0].tolist() == [0, 40, 120, 160]                              # (160 * 4 + 8) >> 4 = 40, (160 * 12 + 8) >> 4 = 120
    assert s5[0, 117:123, 0].tolist() == [0, 10, 50, 110, 150, 160]                     # 160 * (1, 5, 11, 15, 16) / 16, rounded once
    assert s5[239, 117:123, 0].tolist() == [0, 10, 50, 110, 150, 160]
    # a single bright pixel in the corner (0, 0): replication counts it again for every tap that falls outside
    dot = np.zeros((240, 240, 1), np.uint8)
    dot[0, 0] = 255
    d3, d5 = A.augment(dot, A.record(blur=1)), A.augment(dot, A.record(blur=2))
    assert d3[0:2, 0:2, 0].tolist() == [[143, 48], [48, 16]]                            # 255 * (9, 3, 3, 1) / 16 + 1/2
    assert d5[0:3, 0:3, 0].tolist() == [[121, 55, 11], [55, 25, 5], [11, 5, 1]]         # 255 * outer((11, 5, 1)) / 256 + 1/2
    dot = np.zeros((240, 240, 1), np.uint8)
    dot[239, 239] = 255
    assert A.augment(dot, A.record(blur=1))[238:, 238:, 0].tolist() == [[16, 48], [48, 143]]
    assert A.augment(dot, A.record(blur=2))[237:, 237:, 0].tolist() == [[1, 5, 11], [5, 25, 55], [11, 55, 121]]
    # the horizontal box: rows untouched (channel 1 = y, rows 0 and 239 included), columns averaged with (2 * sum + L) / (2 * L)
    x9 = A.augment(ramp, A.record(blur=3, box_len=9))
    assert x9[0, [0, 1, 2, 3, 4, 5, 120, 238, 239], 0].tolist() == [1, 2, 2, 3, 4, 5, 120, 237, 238]
    assert x9[239, [0, 239], 2].tolist() == [254, 17]
    assert x9[:, 7, 1].tolist() == list(range(240))
    x3 = A.augment(ramp, A.record(blur=3, box_len=3))
    assert x3[0, [0, 1, 239], 0].tolist() == [0, 1, 239] and x3[239, [0, 239], 2].tolist() == [255, 16]
    assert A.augment(dot, A.record(blur=3, box_len=9))[239, 230:, 0].tolist() == [0, 0, 0, 0, 0, 28, 57, 85, 113, 142]   # 255 * k / 9 + 1/2
    # a box length that is even, or a blur kind outside 0..3, is no blur
    assert np.array_equal(A.augment(ramp, A.record(blur=3, box_len=4)), ramp) and np.array_equal(A.augment(ramp, A.record(blur=7)), ramp)


def test_colour_ops_by_hand_on_the_ramp():
    """Pixel (x, y) = (100, 120) of the ramp is (100, 120, 155): Y = (100 + 240 + 155 + 2) >> 2 = 124."""
    ramp = _ramp()
    px = lambda **kw: A.augment(ramp, A.record(**{k: v for k, v in kw.items() if k != 'curves'}), curves=kw.get('curves'))[120, 100].tolist()   # noqa: E731
    assert px(sat=0) == [124, 124, 124]
    assert px(sat=384) == [88, 118, 171]                # 124 + ((-24 * 384 + 128) >> 8) = 124 - 36, 124 - 6, 124 + 47
    assert px(sat=256) == [100, 120, 155]
    assert px(gain=(282, 256, 230)) == [110, 120, 139]  # (28200 + 128) >> 8, ., (35650 + 128) >> 8
    assert px(contrast=333) == [92, 118, 163]           # ((-28 * 333 + 128) >> 8) + 128 = -36 + 128, -10 + 128, 35 + 128
    assert px(contrast=333, brightness=32) == [124, 150, 195]
    assert px(brightness=-255) == [0, 0, 0] and px(brightness=255) == [255, 255, 255]
    assert px(contrast=0) == [128, 128, 128]            # (0 + 128) >> 8 = 0
    invert = (255 - np.arange(256)).astype(np.uint8).reshape(1, 256)
    assert px(curve=0, curves=invert) == [155, 135, 100]
    assert px(curve=0, contrast=333, curves=invert) == [163, 137, 92]
    # a fourth channel is flipped and blurred and otherwise copied; one or two channels have no saturation step
    four = np.concatenate([ramp, ramp[..., 1:2]], axis=2)
    out = A.augment(four, A.record(flags=1, sat=0, brightness=50, contrast=300, noise_amp=12, key=5, gain=(300, 300, 300)))
    assert np.array_equal(out[..., 3], four[:, ::-1, 3])
    two = A.augment(ramp[..., :2].copy(), A.record(sat=0, brightness=10))
    assert two[120, 100].tolist() == [110, 130]
    bank = A.gamma_bank((0.6, 0.8, 1.25, 1.6))
    assert bank.shape == (4, 256) and bank[:, 0].tolist() == [0] * 4 and bank[:, 255].tolist() == [255] * 4
    assert bank[0, 64] == 111 and bank[3, 64] == 28     # 255 * (64 / 255) ** 0.6 = 111.3, ** 1.6 = 27.9
    assert np.array_equal(bank, data.Augment().curves())


def test_noise_by_hand_and_its_mean():
    """One pixel by hand from the sampler's mix, then the mean of the noise TERM (before the clamp) over one patch: within its own
    standard error of 0.  The amplitude is 128, where every odd t gives d = t * 128 with a fraction of exactly one half: the case that
    decides between roundings (a plain (d + 128) >> 8 rounds all of them upward, a mean of +1/4, which is two standard errors here)."""
    key = R.draw_hash(0, 0, 0, 11)
    rec = A.record(noise_amp=128, key=key)
    pix = 37 * 240 + 11
    h = R.mix((key + A.GOLD * (pix + 1)) & A.MASK)
    for k in range(3):
        t = ((h >> (16 * k)) & 255) + ((h >> (16 * k + 8)) & 255) - 255
        d = t * 128
        want = (d + 128) >> 8 if d >= 0 else -((-d + 128) >> 8)
        assert int(A.noise_term(rec, k)[37, 11]) == want
    grey = np.full((240, 240, 3), 128, np.uint8)
    out = A.augment(grey, rec).astype(np.int64)
    terms = np.stack([A.noise_term(rec, k) for k in range(3)], axis=2)
    assert np.array_equal(out, np.clip(128 + terms, 0, 255)) and int(out[37, 11, 0]) == min(255, max(0, 128 + int(terms[37, 11, 0])))
    mean, se = terms.mean(), terms.std() / np.sqrt(terms.size)
    print('noise term: mean %.4f, standard error %.4f, std %.2f' % (mean, se, terms.std()))
    assert 40.0 < terms.std() < 60.0                    # 128 / 256 * 255 / sqrt(6) = 52
    assert abs(mean) <= se


# ---- the exported host functions against the restatement ----
def _cfg_struct(cfg):
    f = _lib.PatchAugCfg()
    for k, v in cfg.items():
        if k == 'kind_w':
            f.kind_w[:] = v
        else:
            setattr(f, k, v)
    return f


def _params_host(cfg, seed, counter, rows, count, params_in=None):
    params, labels = np.full((count, 16), -7, np.int32), np.zeros((count, 12), np.int32)
    bbox, vert, lab = np.zeros((count, 4), np.float32), np.zeros((count, 8), np.float32), np.zeros((count, 1), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                              # noqa: E731
    _lib.check(_lib.lib().dbx_patch_aug_params_host(C.byref(_cfg_struct(cfg)), seed, counter, p(params_in) if params_in is not None else None,
                                                    p(rows), count, p(params), p(labels), p(bbox), p(vert), p(lab)))
    return dict(params=params, labels=labels, bbox=bbox, vertices=vert, label=lab)


def _same(got, want):
    for k in ('params', 'labels'):
        assert np.array_equal(got[k], want[k]), k
    for k in ('bbox', 'vertices', 'label'):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k


@pytest.mark.parametrize('count', [1, 7, 300])
@pytest.mark.parametrize('seed,counter', [(0, 0), (1234, 7), (-5, (1 << 40) + 3)])
def test_params_host_equals_the_restatement(count, seed, counter):
    cfg = dict(A.CFG_DEFAULT)
    rows = A.label_rows(count, seed=count)
    got = _params_host(cfg, seed, counter, rows, count)
    _same(got, A.plan(cfg, rows, count, seed=seed & A.MASK, counter=counter))
    if count == 300:                                    # every op was drawn on and off, every blur kind, a refused flip
        P = got['params']
        assert set(P[:, 0].tolist()) == {0, 1, 2} and set(P[:, 1].tolist()) == {0, 1, 2, 3} and set(P[:, 2].tolist()) == {3, 5, 7, 9}
        assert set(P[:, 6].tolist()) == {-1, 0, 1, 2, 3} and (P[:, 7] == 0).any() and P[:, 7].max() == 12
        assert P[:, 3].min() == 154 and P[:, 3].max() == 358 and P[:, 5].min() == -32 and P[:, 5].max() == 32
        # the same records, injected, give the same plan
        asked = P.copy()
        asked[:, 0] = np.where(P[:, 0] == 2, 1, P[:, 0])                # a refused flip was asked for
        _same(_params_host(cfg, 0, 0, rows, count, params_in=asked), got)


def test_params_host_sanitises_injected_records():
    cfg = dict(A.CFG_DEFAULT)
    rows = A.label_rows(6, seed=2)
    wild = np.array([A.to_row(A.record(flags=7, blur=9, sat=-4, contrast=1 << 20, brightness=900, curve=4, noise_amp=-1, gain=(-1, 70000, 256))),
                     A.to_row(A.record(blur=3, box_len=4, curve=-9, brightness=-900)), A.to_row(A.record(blur=3, box_len=11)),
                     A.to_row(A.record(blur=3, box_len=9, curve=3)), A.to_row(A.record(flags=2)), A.to_row(A.record(res0=5, res2=-1))])
    got = _params_host(cfg, 0, 0, rows, 6, params_in=wild)
    _same(got, A.plan(cfg, rows, 6, params_in=wild))
    assert got['params'][0].tolist()[1:8] == [0, 3, 0, 65535, 255, -1, 0] and got['params'][0].tolist()[10:] == [0, 65535, 256, 0, 0, 0]
    assert got['params'][1, 1] == 0 and got['params'][2, 1] == 0 and got['params'][3].tolist()[1:3] == [3, 9] and got['params'][4, 0] == 0
    assert not got['params'][5, 13:].any()


def _augment_host(patch, rec, curves):
    out = np.full_like(patch, 0xA5)
    row = A.to_row(rec)
    G = len(curves)
    _lib.check(_lib.lib().dbx_patch_augment_host(patch.ctypes.data_as(C.c_void_p), row.ctypes.data_as(C.c_void_p),
                                                 curves.ctypes.data_as(C.c_void_p) if G else None, G, patch.shape[2],
                                                 out.ctypes.data_as(C.c_void_p)))
    return out


@pytest.mark.parametrize('c', [1, 3, 4])
@pytest.mark.parametrize('name,rec', A.CASES, ids=[n for n, _ in A.CASES])
def test_augment_host_equals_the_restatement(c, name, rec):
    patch = _random_patch(c, 40 + c)
    bank = A.gamma_bank((0.6, 0.8, 1.25, 1.6))
    want = A.augment(patch, rec, bank)
    assert np.array_equal(_augment_host(patch, rec, bank), want)
    assert not np.array_equal(want, patch) or (c < 3 and name.startswith('sat'))


def test_augment_host_identity_and_an_empty_bank():
    for c in (1, 2, 3, 4):
        patch = _random_patch(c, c)
        assert np.array_equal(_augment_host(patch, A.record(), np.zeros((0, 256), np.uint8)), patch)
        assert np.array_equal(_augment_host(patch, A.record(curve=2), np.zeros((0, 256), np.uint8)), patch)
    ramp = _ramp()
    assert np.array_equal(_augment_host(ramp, A.record(blur=2, flags=1), np.zeros((0, 256), np.uint8)), A.augment(ramp, A.record(blur=2, flags=1)))


def test_augment_config_builds_the_documented_cfg():
    f = data.Augment().cfg()
    for k, v in A.CFG_DEFAULT.items():
        assert (tuple(f.kind_w) if k == 'kind_w' else getattr(f, k)) == v, k
    i = data.Augment.identity()
    cfg = {k: (tuple(i.cfg().kind_w) if k == 'kind_w' else getattr(i.cfg(), k)) for k in A.CFG_DEFAULT}
    rows = A.label_rows(64, seed=3)
    got = _params_host(cfg, 5, 9, rows, 64)
    ident = A.to_row(A.record())
    assert all(np.array_equal(np.delete(r, [2, 8, 9]), np.delete(ident, [2, 8, 9])) for r in got['params']) and np.array_equal(got['labels'], rows)
