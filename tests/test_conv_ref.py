"""tests/conv_ref.py (the float64 reference the exact conv-path tests compare kernels with) against a plain NumPy loop written from the
formula in include/densebox_hip.h, on shapes small enough to loop over; and its two premises shown firing."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as R                                    # noqa: E402


def loop_conv(x, w, bias, pad, relu=False, gate=None):
    """y[n][co][oy][ox] = sum_{ky,kx,ci} x[n][ci][oy + ky - pad][ox + kx - pad] w[co][ci][ky][kx] (+ bias[co]), one term at a time."""
    n, ci, h, wd = x.shape
    co, _, kh, kw = w.shape
    ho, wo = h + 2 * pad - kh + 1, wd + 2 * pad - kw + 1
    y = np.zeros((n, co, ho, wo))
    a = np.zeros((n, co, ho, wo))
    for i in range(n):
        for o in range(co):
            for oy in range(ho):
                for ox in range(wo):
                    s = bias[o] if bias is not None else 0.0
                    t = abs(s)
                    for ky in range(kh):
                        for kx in range(kw):
                            iy, ix = oy + ky - pad, ox + kx - pad
                            if 0 <= iy < h and 0 <= ix < wd:
                                for c in range(ci):
                                    s += x[i, c, iy, ix] * w[o, c, ky, kx]
                                    t += abs(x[i, c, iy, ix] * w[o, c, ky, kx])
                    y[i, o, oy, ox], a[i, o, oy, ox] = s, t
    post = np.maximum(y, 0) if relu else y.copy()
    if gate is not None:
        post = np.where(gate > 0, post, 0.0)
    return y, post, a


def loop_dgrad(dz, w, pad):
    """dx[n][ci][y][x] = sum over (co, ky, kx) of dz[n][co][y - ky + pad][x - kx + pad] w[co][ci][ky][kx]: the forward's formula solved
    for one input element, independent of any flip / transpose."""
    n, co, ho, wo = dz.shape
    _, ci, kh, kw = w.shape
    h, wd = ho - 2 * pad + kh - 1, wo - 2 * pad + kw - 1
    dx = np.zeros((n, ci, h, wd))
    for i in range(n):
        for o in range(co):
            for oy in range(ho):
                for ox in range(wo):
                    for ky in range(kh):
                        for kx in range(kw):
                            iy, ix = oy + ky - pad, ox + kx - pad
                            if 0 <= iy < h and 0 <= ix < wd:
                                dx[i, :, iy, ix] += dz[i, o, oy, ox] * w[o, :, ky, kx]
    return dx


CASES = [  # n, ci, co, h, w, k, pad
    (2, 3, 4, 5, 7, 3, 1), (1, 2, 3, 6, 7, 5, 0), (2, 5, 3, 4, 3, 1, 0), (1, 4, 2, 3, 5, 3, 1),
]


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('epi', [0, R.BIAS, R.BIAS | R.RELU, R.GATE])
def test_conv_ref_equals_the_loop(case, epi):
    n, ci, co, h, w, k, pad = case
    ho, wo = h + 2 * pad - k + 1, w + 2 * pad - k + 1
    x, wt, b, gate = R.int_operands(sum(case) + epi, n, ci, co, ci, k, h, w, 0.6, ho, wo, co)
    assert set(x.unique().tolist()) <= {-1.0, 0.0, 1.0} and float(wt.abs().max()) == 2 and float(gate.min()) < 0 and bool((gate == 0).any())
    ref = R.conv_ref(x, wt, b, k, pad, epi, gate=gate if epi & R.GATE else None)
    y, post, a = loop_conv(x.numpy(), wt.numpy(), b.numpy() if epi & R.BIAS else None, pad, bool(epi & R.RELU),
                           gate.numpy() if epi & R.GATE else None)
    assert ref.pre.dtype == torch.float64
    assert np.array_equal(ref.pre.numpy(), y) and np.array_equal(ref.post.numpy(), post) and np.array_equal(ref.absum.numpy(), a)
    assert float(np.abs(y).max()) > 0 and (not (epi & (R.RELU | R.GATE)) or not np.array_equal(y, post))
    R.assert_exact_premise(ref, 'bf16')


@pytest.mark.parametrize('case', [(2, 3, 4, 5, 7, 3, 1), (1, 4, 2, 4, 6, 1, 0)])
def test_transposed_form_is_the_data_gradient(case):
    n, ci, co, h, w, k, pad = case                      # the forward layer ci -> co; dz has co channels, the result ci
    dz, wt, b, gate = R.int_operands(sum(case), n, co, co, ci, k, h, w, 0.6, h, w, ci)
    ref = R.conv_ref(dz, wt, b, k, pad, R.GATE, gate=gate, transposed=True)
    dx = loop_dgrad(dz.numpy(), wt.numpy(), pad)
    assert np.array_equal(ref.pre.numpy(), dx)
    assert np.array_equal(ref.post.numpy(), np.where(gate.numpy() > 0, dx, 0.0))
    # ... and it is the forward of the weight dbx_pack_weight mode 1 describes
    we = R.effective_weight(wt, True)
    assert we.shape == (ci, co, k, k) and bool((we[1, 0, 0, :] == wt[0, 1, k - 1, :].flip(0)).all())


def test_premise_a_fires_on_sums_of_products_beyond_2_to_24():
    """Outputs that cancel to something small, but whose products add up to 2**24: fp32 need not carry the partial sums exactly."""
    x = torch.ones(1, 2, 1, 1)
    w = torch.tensor([2.0 ** 23, -2.0 ** 23]).view(1, 2, 1, 1)
    ref = R.conv_ref(x, w, torch.zeros(1), 1, 0, 0)
    assert float(ref.post.abs().max()) == 0 and float(ref.absum.max()) == 2.0 ** 24
    with pytest.raises(AssertionError, match=r'premise \(a\)'):
        R.assert_exact_premise(ref, 'f32')
    R.assert_exact_premise(R.conv_ref(x, w / 2, torch.zeros(1), 1, 0, 0), 'f32')


def test_premise_b_fires_on_outputs_the_dtype_cannot_hold():
    x = torch.ones(1, 129, 1, 1)
    w = torch.full((1, 129, 1, 1), 2.0)
    ref = R.conv_ref(x, w, torch.zeros(1), 1, 0, 0)                 # 258: beyond bf16's integers, fine in f16
    with pytest.raises(AssertionError, match=r'premise \(b\)'):
        R.assert_exact_premise(ref, 'bf16')
    R.assert_exact_premise(ref, 'f16')
    half = R.conv_ref(x[:, :128], w[:, :128], torch.zeros(1), 1, 0, 0)  # 256 holds once, not accumulated twice
    R.assert_exact_premise(half, 'bf16')
    with pytest.raises(AssertionError, match=r'premise \(b\)'):
        R.assert_exact_premise(half, 'bf16', times=2)
    with pytest.raises(AssertionError, match=r'premise \(b\)'):
        R.assert_exact_premise(R.conv_ref(x, w * 8, torch.zeros(1), 1, 0, 0), 'f16')
