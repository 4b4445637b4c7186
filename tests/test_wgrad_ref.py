"""CPU self-check of tests/wgrad_ref.py, the float64 oracle of tests/test_hip_wgrad_paths.py: the reference against a plain Python
loop, the impulse expectation against the reference, and the exact-integer premise assertion on operands built to break it."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_ref as R                                   # noqa: E402


def _naive(x, dz, k, pad):
    n, ci, h, w = x.shape
    co, ho, wo = dz.shape[1:]
    dw = [[[[0.0] * k for _ in range(k)] for _ in range(ci)] for _ in range(co)]
    A = [[[[0.0] * k for _ in range(k)] for _ in range(ci)] for _ in range(co)]
    db = [0.0] * co
    xl, zl = x.tolist(), dz.tolist()
    for b in range(n):
        for o in range(co):
            for y in range(ho):
                for xx in range(wo):
                    z = zl[b][o][y][xx]
                    db[o] += z
                    for i in range(ci):
                        for ky in range(k):
                            for kx in range(k):
                                sy, sx = y + ky - pad, xx + kx - pad
                                if 0 <= sy < h and 0 <= sx < w:
                                    dw[o][i][ky][kx] += z * xl[b][i][sy][sx]
                                    A[o][i][ky][kx] += abs(z * xl[b][i][sy][sx])
    return (torch.tensor(dw, dtype=torch.float64), torch.tensor(db, dtype=torch.float64), torch.tensor(A, dtype=torch.float64))


@pytest.mark.parametrize('shape', [(2, 3, 2, 4, 5, 3, 1), (2, 3, 4, 3, 4, 1, 0), (1, 2, 2, 6, 5, 5, 0)])
def test_wgrad_ref64_equals_a_plain_loop(shape):
    n, ci, co, h, w, k, pad = shape
    ho, wo = h + 2 * pad - k + 1, w + 2 * pad - k + 1
    x, dz = R.int_operands(5, n, ci, ci, co, co, h, w, ho, wo)
    assert x.abs().max() <= 3 and dz.abs().max() <= 3 and torch.equal(x, x.round()) and torch.equal(dz, dz.round())
    dw, db, A = R.wgrad_ref64(x, dz, k, pad)
    ndw, ndb, nA = _naive(x, dz, k, pad)
    assert dw.dtype == torch.float64 and db.dtype == torch.float64 and A.dtype == torch.float64
    assert torch.equal(dw, ndw) and torch.equal(db, ndb) and torch.equal(A, nA)
    assert float(dw.abs().sum()) > 0 and bool((A >= dw.abs()).all())
    # ... and torch's own weight gradient agrees
    tw = torch.nn.grad.conv2d_weight(x.double(), (co, ci, k, k), dz.double(), padding=pad)
    assert torch.equal(dw, tw)
    R.check_exact_premise(A, dz)
    R.check_exact_premise(A, dz, times=2)


def test_int_operands_zero_the_padding_channels():
    x, dz = R.int_operands(1, 2, 8, 3, 16, 9, 4, 5, 4, 5)
    assert x.shape == (2, 8, 4, 5) and dz.shape == (2, 16, 4, 5)
    assert float(x[:, 3:].abs().sum()) == 0 and float(dz[:, 9:].abs().sum()) == 0
    assert x[:, :3].unique().tolist() == [-3, -2, -1, 0, 1, 2, 3] and dz[:, :9].unique().tolist() == [-3, -2, -1, 0, 1, 2, 3]
    x2, dz2 = R.int_operands(1, 2, 8, 3, 16, 9, 4, 5, 4, 5)
    assert torch.equal(x, x2) and torch.equal(dz, dz2)             # seeded


@pytest.mark.parametrize('k,pad', [(3, 1), (1, 0)])
def test_impulse_expected_equals_the_reference(k, pad):
    n, ci, co, h, w = 2, 3, 2, 4, 5
    places = [((0, 0, 0, 0), (0, 0, 0, 0)), ((1, 2, 3, 4), (1, 1, 3, 4)), ((0, 1, 1, 1), (0, 1, 0, 0)), ((0, 1, 0, 0), (0, 0, 1, 1)),
              ((0, 2, 3, 4), (1, 0, 0, 0)), ((1, 0, 0, 0), (0, 1, 3, 4)), ((1, 1, 2, 4), (1, 0, 2, 3)), ((1, 1, 0, 4), (1, 0, 3, 0))]
    for xpos, zpos in places:
        x = torch.zeros(n, ci, h, w)
        dz = torch.zeros(n, co, h, w)
        x[xpos] = 1.0
        dz[zpos] = 1.0
        dw, db, _ = R.wgrad_ref64(x, dz, k, pad)
        edw, edb = R.impulse_expected(co, ci, k, pad, xpos, zpos)
        assert torch.equal(dw, edw) and torch.equal(db, edb), (xpos, zpos)
        assert int((edw != 0).sum()) <= 1


def test_exact_premise_fires_on_operands_built_to_break_it():
    # 4096 * 4096 = 2**24 in one product: not below the limit
    x = torch.zeros(1, 1, 2, 2)
    dz = torch.zeros(1, 1, 2, 2)
    x[0, 0, 0, 0] = 4096.0
    dz[0, 0, 0, 0] = 4096.0
    _, _, A = R.wgrad_ref64(x, dz, 1, 0)
    with pytest.raises(AssertionError, match='premise'):
        R.check_exact_premise(A, dz)
    # products fine, the bias sum is not: 2**12 pixels of 2**12 against an all-zero x
    dz = torch.full((1, 1, 64, 64), 4096.0)
    x = torch.zeros(1, 1, 64, 64)
    _, _, A = R.wgrad_ref64(x, dz, 1, 0)
    with pytest.raises(AssertionError, match=r'sum\|dz\|'):
        R.check_exact_premise(A, dz)
    # below the limit once, not when accumulated twice
    x = torch.full((1, 1, 1, 1), 4096.0)
    dz = torch.full((1, 1, 1, 1), 2048.0 + 1.0)
    _, _, A = R.wgrad_ref64(x, dz, 1, 0)
    R.check_exact_premise(A, dz)
    with pytest.raises(AssertionError, match='premise'):
        R.check_exact_premise(A, dz, times=2)
