"""The NV12 restatement (tests/nv12_ref.py) itself, on the CPU: the header's coefficient constants are the derived ones; hand-computed
pixels in both directions; the 14-bit integers against the float64 formula rounded to nearest -- never more than 1 apart (before its one
rounding the fixed-point value is within 3 * 1020 * 0.5 / 2^16 < 0.03 of the exact one in the widest case, the chroma of a block; the
other sums are narrower) and different in at most 0.5 % of the values of a channel, which a systematically biased table would exceed --
over all 2^24 (Y, U, V) for 601 limited and 2^20 random triples for the other variants, and over 2^20 random blocks from RGB."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nv12_ref as N  # noqa: E402


def test_header_constants_are_the_derived_coefficients():
    consts = N.header_constants()
    assert sorted(consts) == sorted(N.VARIANTS)
    for v in N.VARIANTS:
        assert consts[v] == (N.to_rgb_coef(*v), N.from_rgb_coef(*v)), v
        f = N.from_rgb_coef(*v)
        assert sum(f[3:6]) == 0 and sum(f[6:9]) == 0, 'grey must give U = V = 128'
        assert sum(f[:3]) == (14071 if v[1] == 'limited' else 16384)
    assert N.to_rgb_coef(601, 'limited') == (19077, 26149, -6419, -13320, 33050)
    assert N.to_rgb_coef(601, 'full') == (16384, 22970, -5638, -11700, 29032)
    assert N.to_rgb_coef(709, 'limited') == (19077, 29372, -3494, -8731, 34610)
    assert N.to_rgb_coef(709, 'full') == (16384, 25802, -3069, -7670, 30402)
    assert N.from_rgb_coef(601, 'limited') == (4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026, -1170)


TO_RGB_PINS = [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((81, 90, 240), (254, 0, 0)), ((145, 54, 34), (0, 255, 1)),
               ((41, 240, 110), (0, 0, 255)), ((0, 0, 0), (0, 136, 0)), ((255, 255, 255), (255, 125, 255))]


def test_hand_pins_to_rgb():
    for (y, u, v), rgb in TO_RGB_PINS:
        got = N.yuv_to_rgb(np.array([y]), np.array([u]), np.array([v]))[0]
        assert tuple(int(c) for c in got) == rgb, ((y, u, v), got)
        bgr = N.yuv_to_rgb(np.array([y]), np.array([u]), np.array([v]), order='bgr')[0]
        assert tuple(int(c) for c in bgr) == rgb[::-1]
    frame = np.array([[81, 81], [81, 81], [90, 240]], np.uint8)              # a 2 x 2 frame: one block
    assert (N.nv12_to_rgb(frame) == np.array([254, 0, 0], np.uint8)).all()


FROM_RGB_PINS = [((0, 0, 0), (16, 128, 128)), ((255, 255, 255), (235, 128, 128)), ((255, 0, 0), (81, 90, 240)),
                 ((0, 255, 0), (145, 54, 34)), ((0, 0, 255), (41, 240, 110))]


def _uniform(rgb):
    return np.tile(np.array(rgb, np.uint8), (2, 2, 1))


def test_hand_pins_from_rgb_on_uniform_blocks():
    for rgb, (y, u, v) in FROM_RGB_PINS:
        Y, U, V = N.rgb_to_yuv_blocks(_uniform(rgb))
        assert (Y == y).all() and int(U[0, 0]) == u and int(V[0, 0]) == v, (rgb, Y, U, V)
        Y, U, V = N.rgb_to_yuv_blocks(_uniform(rgb[::-1]), order='bgr')
        assert (Y == y).all() and int(U[0, 0]) == u and int(V[0, 0]) == v
        assert N.rgb_to_nv12(_uniform(rgb)).tolist() == [[y, y], [y, y], [u, v]]
    Y, U, V = N.rgb_to_yuv_blocks(_uniform((255, 0, 0)), 709, 'limited')
    assert (int(Y[0, 0]), int(U[0, 0]), int(V[0, 0])) == (63, 102, 240)


def _compare(got, want, what):
    """got, want uint8 [..., channels]: never more than 1 apart, at most 0.5 % of a channel's values differ"""
    diff = np.abs(got.astype(np.int16) - want.astype(np.int16)).reshape(-1, got.shape[-1])
    assert int(diff.max()) <= 1, (what, int(diff.max()))
    share = (diff != 0).mean(axis=0)
    assert (share <= 0.005).all(), (what, share)
    return diff


def test_all_yuv_triples_601_limited_against_float64():
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    u, v = u.reshape(-1), v.reshape(-1)
    differing, total = np.zeros(3), 0
    for y0 in range(0, 256, 16):
        Y = np.repeat(np.arange(y0, y0 + 16), u.size)
        U, V = np.tile(u, 16), np.tile(v, 16)
        got, want = N.yuv_to_rgb(Y, U, V), N.yuv_to_rgb_float(Y, U, V)
        diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
        assert int(diff.max()) <= 1, y0
        differing += (diff != 0).sum(axis=0)
        total += Y.size
    assert total == 1 << 24
    assert (differing / total <= 0.005).all(), differing / total


@pytest.mark.parametrize('standard,rng', N.VARIANTS[1:])
def test_random_yuv_triples_against_float64(standard, rng):
    rs = np.random.RandomState(standard + len(rng))
    Y, U, V = (rs.randint(0, 256, 1 << 20) for _ in range(3))
    _compare(N.yuv_to_rgb(Y, U, V, standard, rng), N.yuv_to_rgb_float(Y, U, V, standard, rng), (standard, rng))


@pytest.mark.parametrize('standard,rng', N.VARIANTS)
def test_random_rgb_blocks_against_float64(standard, rng):
    rs = np.random.RandomState(7 * standard + len(rng))
    img = rs.randint(0, 256, size=(2048, 2048, 3)).astype(np.uint8)              # 2^20 blocks of four independent pixels
    Y, U, V = N.rgb_to_yuv_blocks(img, standard, rng)
    Yf, Uf, Vf = N.rgb_to_yuv_float(img, standard, rng)
    _compare(Y[..., None], Yf[..., None], (standard, rng, 'Y'))
    _compare(np.stack([U, V], axis=-1), np.stack([Uf, Vf], axis=-1), (standard, rng, 'UV'))


def test_chroma_of_a_block_with_four_different_pixels_is_the_formula_on_the_sums():
    block = np.array([[[255, 0, 0], [0, 255, 0]], [[0, 0, 255], [90, 60, 30]]], np.uint8)
    Rs, Gs, Bs = 345, 315, 285
    assert block.reshape(4, 3).sum(axis=0).tolist() == [Rs, Gs, Bs]
    Y, U, V = N.rgb_to_yuv_blocks(block)
    assert int(U[0, 0]) == ((-2428 * Rs - 4768 * Gs + 7196 * Bs + 32768) >> 16) + 128 == 124
    assert int(V[0, 0]) == ((7196 * Rs - 6026 * Gs - 1170 * Bs + 32768) >> 16) + 128 == 132
    assert Y.tolist() == [[81, 145], [41, ((4207 * 90 + 8260 * 60 + 1604 * 30 + 8192) >> 14) + 16]]
    # the round trip is not the identity: the block's four colours come back as one chroma
    back = N.nv12_to_rgb(N.rgb_to_nv12(block))
    assert not np.array_equal(back, block)
