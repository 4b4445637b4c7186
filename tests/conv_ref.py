"""Float64 CPU reference of the forward convolution (and its data-gradient form) on integer operands, with the premise under which a
kernel's result has ZERO tolerance.

Operands: x in {-1, 0, 1} (nonzero with a per-case density), w in [-2, 2], bias in [-3, 3], gate in [-2, 2] (zeros and negatives
included: the gate passes where gate > 0) -- all exactly representable in bf16, f16 and fp32, so one reference serves every dtype.

Premise (assert_exact_premise, checked from the reference alone before anything is launched):
 (a) every per-output sum of |x w| products plus |bias| is below 2**24.  Every partial sum, in whatever order and grouping a kernel
     accumulates (MFMA blocks, K tiles of a ring, taps), is then an integer of magnitude below 2**24 and exact in fp32: the fp32
     accumulator holds the exact integer.
 (b) every final output magnitude is at most 256 (bf16: 8 significand bits hold every integer to 256), 2048 (f16: 11 bits) or 2**24
     (fp32).  The expected value is then representable, the store conversion cannot round, and an error of 1 anywhere is visible.
The density of x is what keeps (b): the sum over K = taps x channels terms of density q has a standard deviation of sqrt(2 q K)
(E w^2 = 2), e.g. 34 for K = 9 x 512 at q = 1/8.  Densities are fixed in the callers' case tables and never adjusted at run time.

Reference times (float64 F.conv2d for the sums and for the |products|, plus the callers' sensitivity check; measured with 8 CPU threads)
for the case table of tests/test_hip_conv_paths.py: 0.00 - 0.07 s for the igemm / dma / c8 shapes, 0.2 - 1.6 s for the band, c64p
and pooled cases, 1.4 - 1.8 s for the 8-phase and ws cases at ~25 k - 46 k pixels, 3.0 s for p8-3x3-bias-roundup (57 771 pixels x
512 couts x K 1152) and 3.1 s for ws-3x3-wm2 (K 2880), 7.1 s and 8.0 s for the two tall band cases (524 172 frame positions cannot be
fewer; K is at its minimum of 576 / 1152) -- 46 s for the whole table.  With 16 threads the whole GPU file, references included,
runs in 27 s.  Every reference is computed once per case and shared by its dtypes and variants."""
import collections

import torch
import torch.nn.functional as F

BIAS, RELU, GATE = 1, 2, 4                                  # the epilogue bits of include/densebox_hip.h this reference knows
LIMIT = {'bf16': 256.0, 'f16': 2048.0, 'f32': float(2 ** 24)}

Ref = collections.namedtuple('Ref', 'pre post absum')       # float64 NCHW: sums (+ bias), after the epilogue, sum |products| + |bias|


def int_operands(seed, n, cx, co_w, ci_w, k, h, w, density, ho=None, wo=None, cg=None):
    """x [n][cx][h][w] in {-1, 0, 1}, w [co_w][ci_w][k][k] in [-2, 2], bias [max(co_w, ci_w)] in [-3, 3], gate [n][cg][ho][wo] in [-2, 2]."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    sign = torch.randint(0, 2, (n, cx, h, w), generator=g).double() * 2 - 1
    x = sign * (torch.rand(n, cx, h, w, generator=g) < density).double()
    wt = torch.randint(-2, 3, (co_w, ci_w, k, k), generator=g).double()
    bias = torch.randint(-3, 4, (max(co_w, ci_w),), generator=g).double()
    gate = None
    if cg:
        gate = torch.randint(-2, 3, (n, cg, ho if ho else h, wo if wo else w), generator=g).double()
    return x, wt, bias, gate


def effective_weight(w, transposed):
    """The OIHW weight the call convolves x with.  transposed: the data gradient of the layer w belongs to, as dbx_pack_weight mode 1
    lays it out (wp[ci][taps - 1 - tap][co] = w[co][ci][tap]): channel roles swapped, taps flipped."""
    return w.transpose(0, 1).flip(2, 3).contiguous() if transposed else w


def conv_ref(x, w, bias, k, pad, epilogue, gate=None, transposed=False):
    """y = epi(sum_{ky,kx,ci} x[n, oy + ky - pad, ox + kx - pad, ci] w'[co][ci][ky][kx] + bias[co]) in float64 on the CPU; x, w, bias,
    gate are (integer-valued) tensors of any float dtype.  Returns Ref(pre, post, absum)."""
    assert w.shape[2] == k and w.shape[3] == k
    x, w = x.double().cpu(), effective_weight(w.double().cpu(), transposed)
    b = bias.double().cpu()[:w.shape[0]] if (epilogue & BIAS) else None
    pre = F.conv2d(x, w, b, padding=pad)
    absum = F.conv2d(x.abs(), w.abs(), b.abs() if b is not None else None, padding=pad)
    post = pre
    if epilogue & RELU:
        post = post.clamp(min=0)
    if epilogue & GATE:
        assert gate is not None and gate.shape == pre.shape
        post = post * (gate.double().cpu() > 0)
    return Ref(pre, post, absum)


def assert_exact_premise(ref, dtype, times=1):
    """(a) and (b) of the module docstring for `times` accumulations of the result into one destination (DBX_EPI_ACCUM: times = 2)."""
    a = float(ref.absum.max()) * times
    assert a < 2 ** 24, 'premise (a): a sum of |products| + |bias| reaches %g >= 2**24: fp32 accumulation need not be exact' % a
    m = float(ref.post.abs().max()) * times
    assert m <= LIMIT[dtype], 'premise (b): an output of magnitude %g is beyond the integers %s represents (%g)' % (m, dtype, LIMIT[dtype])
    assert bool((ref.pre == ref.pre.round()).all())
