"""Float64 CPU reference of the stage-2 heads backward (csrc/aux_ops.hip: dbx_head2_dgrad / _wgrad / _backward / _backward_up), written
from the maths and not from the kernels, with the premise under which a kernel's result has ZERO tolerance, the case table of
tests/test_hip_head2_paths.py and a restatement of the host-side launch plan (h2u_plan and the grouping of heads into launches).

The operation, for nh <= 4 heads of k_h <= 8 outputs over P = n h w pixels (pixel index p row-major over (image, row, column)):
  d_hid[p, hd, c] = keep[p, 512 hd + c] * scale * sum_{j < k_hd} d_out[p, hd, j] * W2[hd][j, c]      scale 2 behind dropout, else 1
  dW2[hd][j, c]   = sum_p d_out[p, hd, j] * hid[p, 512 hd + c]              db2[hd][j] = sum_p d_out[p, hd, j]
  d_g44           = up^T(round_T(d_hid)): the transpose of the align_corners bilinear up-sampling hs x ws -> h x w, with the
                    coefficients of bilin_coef (ATen's float arithmetic, restated in NumPy float32) and float64 accumulation.
keep is a byte mask or bit (c % 32) of dbx_drop_hash32(seed, p, c / 32) (drop_keep below, shared with tests/test_hip_conv_paths.py,
whose p8-heads case pins it against the forward epilogue).

Operands (int_operands): d_out in {-2 .. 2}, hid in {-4 .. 4} with about half of it zero, W2 in {-2 .. 2}: exact in bf16, f16, fp32.
Premise (assert_premise, from the reference alone, before any launch):
 (a) every d_hid value is an integer of magnitude <= 64 = 2 x 8 x 2 x 2: exact in all three types, the store cannot round;
 (b) every sum over pixels of |d_out hid| and of |d_out| is below 2**24: every partial sum of dW2 / db2, in any order and grouping
     (lanes, pixel groups, workgroups, the reduce kernel's waves), is an integer below 2**24 and exact in fp32;
 (c) dyadic geometries ((hs - 1) / (h - 1) = (ws - 1) / (w - 1) = 1/2): every coefficient is 0, 1/2 or 1, d_g44 is a multiple of 1/4
     whose sum of |terms| stays below 2**24 / 4: every fp32 accumulation order yields it exactly and the expected output is that value
     rounded to T to nearest-even (round_np; torch's cast), bit for bit;
 (d) other geometries (60 -> 30, the workload's): d_hid, dW2, db2 as above; d_g44 within E = 16 x 2**-24 x sum |coef d_hid| of the
     float64 value before its rounding to T -- an output sums at most 16 terms (<= 4 destination rows x <= 4 columns carry weight at
     up-sampling by ~2: max_terms, asserted), reduced in two passes of fmas (over y, then over x) that round once per term -- i.e.
     inside [round_T(ref - E), round_T(ref + E)] (interval); the share of outputs whose interval holds more than one value of T
     must be below 1 %.  That share grows with the cancellation inside an output (E follows sum |terms|, the spacing of T follows
     the sum): with a gradient at every pixel it is 0.4 - 0.6 % in bf16 but 2.0 - 2.9 % in f16, so the case carries a gradient at
     one pixel in eight (Case.q, fixed in the table; the loss selects a minority of the pixels too): 0.09 - 0.21 % in bf16 and
     0.27 - 0.57 % in f16.

Reference times (NumPy float64): every case under 0.1 s except up-workload (7200 pixels x 2048 channels:
about 1 s per dropout form).  A reference is computed once per (case, dropout form, content) and shared by the dtypes."""
import collections

import numpy as np

MASK32 = np.uint64(0xFFFFFFFF)
FMT = {'bf16': (8, -126), 'f16': (11, -14), 'f32': (24, -126)}     # significand bits (hidden one included), exponent of the least normal


# ---------------------------------------------------------------------------------------------------------------- dropout keep bits
def drop_keep(seed, M, co):
    """dbx_drop_hash32 (csrc/common.hpp) restated: keep bit of (pixel m, channel ch) = bit ch % 32 of a lowbias32 finaliser over
    (seed, m, ch / 32).  Returns bool [M][co]."""
    m = np.arange(M, dtype=np.uint64)[:, None]
    c32 = (np.arange(co, dtype=np.uint64) // np.uint64(32))[None, :]
    mask = MASK32
    x = (np.uint64(seed) ^ ((m * np.uint64(0x9E3779B1)) & mask) ^ ((c32 * np.uint64(0x85EBCA77)) & mask)) & mask
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & mask
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & mask
    x ^= x >> np.uint64(16)
    bit = (np.arange(co, dtype=np.uint64) % np.uint64(32))[None, :]
    return ((x >> bit) & np.uint64(1)).astype(bool)


# ---------------------------------------------------------------------------------------------------------------- number formats
def round_np(x, dtn):
    """float64 -> the nearest value of the format (ties to even, gradual underflow), as float64.  One rounding straight from float64:
    a cast through float32 first could round twice."""
    p, emin = FMT[dtn]
    x = np.asarray(x, dtype=np.float64)
    _, e = np.frexp(x)                                      # x = m 2**e, 0.5 <= |m| < 1: the leading bit has weight 2**(e - 1)
    ulp = np.ldexp(1.0, np.maximum(e - 1, emin) - (p - 1))
    return np.rint(x / ulp) * ulp                           # (scaling by a power of two is exact; rint rounds half to even)


# ---------------------------------------------------------------------------------------------------------------- bilinear up^T
def bilin_coef(out_size, in_size):
    """ATen's align_corners coefficients in float32, as bilin_coef (csrc/aux_ops.hip) documents them: scale = (in - 1) / (out - 1) in
    float; src = scale * dst (ONE float product, no contraction); i0 = (int)src clamped to in - 1; i1 = i0 + (i0 < in - 1);
    l1 = src - i0; l0 = 1 - l1.  Returns (i0, i1, l0, l1), one entry per destination index."""
    scale = np.float32(in_size - 1) / np.float32(out_size - 1) if out_size > 1 else np.float32(0)
    d = np.arange(out_size)
    src = (scale * d.astype(np.float32)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), in_size - 1)      # (truncation: src >= 0)
    i1 = i0 + (i0 < in_size - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1) - l1).astype(np.float32)
    return i0, i1, l0, l1


def up_matrix(out_size, in_size, swap=False):
    """U [out][in] float64: destination d = l0 source i0 + l1 source i1 (swap: the two weights exchanged, a sensitivity probe)."""
    i0, i1, l0, l1 = bilin_coef(out_size, in_size)
    if swap:
        l0, l1 = l1, l0
    U = np.zeros((out_size, in_size))
    np.add.at(U, (np.arange(out_size), i0), l0.astype(np.float64))
    np.add.at(U, (np.arange(out_size), i1), l1.astype(np.float64))
    return U


def up_transposed(d, hs, ws, swap=False):
    """d [n][h][w][C] float64 -> (up^T d, up^T |d|) on [n][hs][ws][C]: out[n, iy, ix] = sum_{oy, ox} Uy[oy, iy] Ux[ox, ix] d[n, oy, ox]."""
    n, h, w, C = d.shape
    Uy, Ux = up_matrix(h, hs, swap), up_matrix(w, ws, swap)

    def apply(a):
        t = np.tensordot(Uy.T, a.transpose(1, 0, 2, 3).reshape(h, -1), axes=1).reshape(hs, n, w, C)      # [iy][n][ox][C]
        t = np.tensordot(Ux.T, t.transpose(2, 0, 1, 3).reshape(w, -1), axes=1).reshape(ws, hs, n, C)     # [ix][iy][n][C]
        return np.ascontiguousarray(t.transpose(2, 1, 0, 3))
    return apply(d), apply(np.abs(d))


# ---------------------------------------------------------------------------------------------------------------- the reference
Ref = collections.namedtuple('Ref', 'd_hid dw db absw absb')   # d_hid [P][nh][512]; per head dw [k][512], db [k], sums of |terms|


def head2_ref(d_out, hid, w2, keep, scale, own_w=None):
    """d_out [P][nh][8] (channels >= k_hd zero), hid [P][512 nh], w2[hd] [k_hd][512], keep [P][512 nh] (bool / bytes) or None.
    own_w [P] (default all ones): how many times a pixel enters the weight-gradient sums -- a half-row split that owns a column twice
    or not at all is modelled by 2 or 0 there (sensitivity probe)."""
    P, nh, _ = d_out.shape
    d_out, hid = d_out.astype(np.float64), hid.astype(np.float64)
    d_hid = np.zeros((P, nh, 512))
    dw, db, absw, absb = [], [], [], []
    wgt = np.ones(P) if own_w is None else np.asarray(own_w, dtype=np.float64)
    for hd in range(nh):
        k = w2[hd].shape[0]
        g = d_out[:, hd, :k]
        assert not d_out[:, hd, k:].any(), 'contract: d_out channels [k, 8) are zero'
        d_hid[:, hd] = scale * (g @ w2[hd].astype(np.float64))
        hh = hid[:, 512 * hd:512 * (hd + 1)]
        gw = g * wgt[:, None]
        dw.append(gw.T @ hh)
        db.append(gw.sum(axis=0))
        absw.append(np.abs(gw).T @ np.abs(hh))
        absb.append(np.abs(gw).sum(axis=0))
    if keep is not None:
        d_hid *= (np.asarray(keep).reshape(P, nh, 512) != 0)
    return Ref(d_hid, dw, db, absw, absb)


def assert_premise(ref, g44=None, g44_abs=None, dyadic=None, geom=None):
    """(a) - (c) of the module docstring."""
    assert np.array_equal(ref.d_hid, np.rint(ref.d_hid)) and float(np.abs(ref.d_hid).max()) <= 64, 'premise (a)'
    for a in ref.absw + ref.absb:
        assert float(a.max()) < 2 ** 24, 'premise (b): a sum of |products| reaches %g' % float(a.max())
    for a in ref.dw + ref.db:
        assert np.array_equal(a, np.rint(a))
    if dyadic:
        n, h, w, hs, ws = geom
        for o, i in ((h, hs), (w, ws)):
            _, _, l0, l1 = bilin_coef(o, i)
            assert set(np.unique(np.concatenate([l0, l1])).tolist()) <= {0.0, 0.5, 1.0}, 'premise (c): a coefficient off {0, 1/2, 1}'
        assert np.array_equal(g44 * 4, np.rint(g44 * 4)) and float(g44_abs.max()) < 2 ** 22, 'premise (c)'


def max_terms(case):
    """The largest number of (destination row, destination column) terms with a nonzero coefficient that one d_g44 output sums."""
    return int((up_matrix(case.h, case.hs) != 0).sum(axis=0).max() * (up_matrix(case.w, case.ws) != 0).sum(axis=0).max())


def interval(g44, g44_abs, dtn, K=16):
    """(d): the closed interval of T values a kernel's d_g44 may take, and the share of outputs where it holds more than one.  K: the
    roundings a term passes through (16 here; tests/aux_ref.py derives its kernels' own)."""
    E = K * 2.0 ** -24 * g44_abs
    lo, hi = round_np(g44 - E, dtn), round_np(g44 + E, dtn)
    return lo, hi, float((lo != hi).mean())


# ---------------------------------------------------------------------------------------------------------------- operands
def int_operands(seed, P, ks, hid_density=0.5):
    """d_out [P][nh][8] in {-2 .. 2} (zero past k), hid [P][512 nh] in {-4 .. 4} with about (1 - hid_density) of it zero, W2[hd] [k][512]
    in {-2 .. 2}, mask [P][512 nh] bytes in {0, 1}."""
    rng = np.random.RandomState(seed)
    nh = len(ks)
    d_out = np.zeros((P, nh, 8), dtype=np.int8)
    for hd, k in enumerate(ks):
        d_out[:, hd, :k] = rng.randint(-2, 3, size=(P, k))
    hid = (rng.randint(1, 5, size=(P, 512 * nh)) * (rng.randint(0, 2, size=(P, 512 * nh)) * 2 - 1) *
           (rng.random_sample((P, 512 * nh)) < hid_density)).astype(np.int8)
    w2 = [rng.randint(-2, 3, size=(k, 512)).astype(np.float64) for k in ks]
    mask = rng.randint(0, 2, size=(P, 512 * nh)).astype(np.uint8)
    return d_out, hid, w2, mask


# ---------------------------------------------------------------------------------------------------------------- cases and plans
Case = collections.namedtuple('Case', 'name n h w hs ws ks dyadic q', defaults=(1.0,))   # q: share of pixels with a nonzero d_out
CASES = collections.OrderedDict((c.name, c) for c in [
    Case('up-one-half', 2, 9, 17, 5, 9, (1, 2, 3, 8), True),
    Case('up-two-halves-ring', 2, 17, 33, 9, 17, (1, 4, 4, 8), True),
    Case('up-stride-2h', 17, 5, 33, 3, 17, (1, 4, 4, 8), True),
    Case('up-stride-1h', 17, 5, 17, 3, 9, (4, 3, 4, 4), True),
    Case('up-reduce-unrolled', 33, 3, 33, 2, 17, (1, 8), True),
    Case('up-workload', 2, 60, 60, 30, 30, (1, 4, 4, 8), False, 0.125),
    Case('up-fallback', 2, 9, 65, 5, 33, (1, 4, 4, 8), True),
    Case('wgrad-cap-3h', 3, 171, 5, None, None, (2, 4, 4), None),
    Case('wgrad-cap-1h', 3, 171, 5, None, None, (8,), None),
])

Half = collections.namedtuple('Half', 'px_lo px_n own_lo own_hi ix_lo ix_n')
Launch = collections.namedtuple('Launch', 'head0 heads kj groups blocks')
Plan = collections.namedtuple('Plan', 'fused halves half launches')
WGS = 512                                                   # workgroups a launch aims at (two per CU)


def half_plan(W, ws):
    """h2u_plan restated: None (no one-pass form) or (halves, [Half, Half]).  One workgroup walks a whole row when it fits 32 pixel and
    16 source columns; otherwise source columns split at S = ws / 2, each half walks every pixel column that interpolates from one of
    its source columns (x0 = trunc(sx ox) in float, or x0 + 1), and the overlap is owned left / right of its middle."""
    if W > 64 or ws > 32 or W < 1 or ws < 1:
        return None
    x0 = bilin_coef(W, ws)[0]
    if W <= 32 and ws <= 16:
        hf = Half(0, W, 0, W, 0, ws)
        return 1, [hf, hf]
    S = ws // 2
    if S < 1 or S > 16 or ws - S > 16:
        return None
    hiL = max(ox for ox in range(W) if x0[ox] <= S - 1)
    loR = min(ox for ox in range(W) if x0[ox] >= S - 1)
    if hiL + 1 > 32 or W - loR > 32 or loR > hiL + 1:
        return None
    Pb = (loR + hiL + 1) // 2
    return 2, [Half(0, hiL + 1, 0, Pb, 0, S), Half(loR, W - loR, Pb, W, S, ws - S)]


def plan_ref(case, dtn):
    """What dbx_head2_backward_up_plan must report (default environment)."""
    none = Plan(0, 0, [Half(*[0] * 6)] * 2, [])
    if case.hs is None or dtn == 'f32':
        return none
    sy = np.float32(case.hs - 1) / np.float32(case.h - 1) if case.h > 1 else np.float32(0)
    sx = np.float32(case.ws - 1) / np.float32(case.w - 1) if case.w > 1 else np.float32(0)
    hp = half_plan(case.w, case.ws)
    if not (0 < sy < 1 and np.float32(0.45) < sx < 1 and case.h >= 2 and hp):
        return none
    halves, half = hp
    kup = [1 if k <= 1 else 2 if k <= 2 else 4 if k <= 4 else 8 for k in case.ks]
    launches, h0 = [], 0
    while h0 < len(kup):
        h1 = h0 + 1
        while h1 < len(kup) and kup[h1] == kup[h0]:
            h1 += 1
        groups = min(max(WGS // ((h1 - h0) * 8 * halves), 1), case.n)
        launches.append(Launch(h0, h1 - h0, kup[h0], groups, groups * halves))
        h0 = h1
    return Plan(1, halves, half, launches)


def wgrad_blocks(case):
    """Workgroups of head2_wgrad_kernel, pixels per workgroup and workgroups with an empty range (the separate passes' split)."""
    rows, npix = case.n * case.h, case.n * case.h * case.w
    blocks = min(rows, 512)
    per = -(-npix // blocks)
    return blocks, per, sum(1 for b in range(blocks) if b * per >= npix)


def impulse_pixels(case, dtn='bf16'):
    """Pixels (image, row, column) for the impulse variant: first and last pixel of the first and last image, both sides of every image
    seam a workgroup crosses (workgroup g walks images g, g + groups, ...: the last pixel of one and the first of the next; every
    consecutive pair of images for the separate passes, whose workgroups own contiguous pixel ranges), both sides of the ownership
    boundary, column W - 1 of a middle row."""
    n, h, w = case.n, case.h, case.w
    px = [(0, 0, 0), (0, h - 1, w - 1), (n - 1, 0, 0), (n - 1, h - 1, w - 1), (0, h // 2, w - 1), (n - 1, 1, w - 1)]
    plan = plan_ref(case, dtn)
    steps = sorted({l.groups for l in plan.launches if l.groups < n}) if plan.fused else [1]
    for g in steps:
        for a in range(n - g):
            if a < 2 or a + g == n - 1:                     # (every seam looks alike: the first two and the last keep the list short)
                px += [(a, h - 1, w - 1), (a, h - 1, 0), (a + g, 0, 0), (a + g, 0, w - 1)]
    if plan.fused and plan.halves == 2:
        b = plan.half[0].own_hi
        px += [(0, 1, b - 1), (0, 1, b), (n - 1, h - 1, b - 1), (n - 1, h - 1, b), (0, 0, plan.half[1].px_lo), (0, 0, plan.half[0].px_n - 1)]
    return sorted(set(px))


# ---------------------------------------------------------------------------------------------------------------- a case's data
SEED = 0xC0DE                                               # hash dropout seed of every case
UNREP = {'bf16': 1 + 2.0 ** -9, 'f16': 1 + 2.0 ** -12}       # a W2 entry the type cannot hold (1 + 2**-9 IS an f16 number: 10 fraction bits)
_CACHE = collections.OrderedDict()


def keep_of(case, drop, mask):
    P, C = case.n * case.h * case.w, 512 * len(case.ks)
    return {'none': None, 'mask': mask, 'hash': drop_keep(SEED, P, C) if drop == 'hash' else None}[drop]


def make(case, drop, content='dense', w2_dtn=None):
    """Operands and reference of a case: dict(d_out, hid, w2, mask, keep, ref, g44, g44_abs).  content 'dense': int_operands, with the
    zeros of d_out at the first and last pixel of every image replaced by ones (the sensitivity probes remove terms there);
    'impulse': d_out zero but for single ones at impulse_pixels(case), in channel (index % k) of every head, under W2 without zeros.
    w2_dtn ('bf16' / 'f16'): the form without a stored d_hid -- W2 gets entries UNREP[w2_dtn] and the reference uses W2 rounded to that
    type; 'w2_raw' is what the call is given, 'ref_raw' the reference with the unrounded W2."""
    key = (case, drop, content, w2_dtn)
    if key in _CACHE:
        _CACHE.move_to_end(key)
        return _CACHE[key]
    n, h, w, ks = case.n, case.h, case.w, case.ks
    P = n * h * w
    d_out, hid, w2, mask = int_operands(1000 + sum(ord(ch) for ch in case.name), P, ks)
    if case.q < 1:
        d_out *= np.random.RandomState(3).random_sample((P, 1, 1)) < case.q
    for img in range(n):
        for p in (img * h * w, (img + 1) * h * w - 1):
            for hd, k in enumerate(ks):
                d_out[p, hd, :k] = np.where(d_out[p, hd, :k] == 0, 1, d_out[p, hd, :k])
    if content == 'impulse':
        d_out[:] = 0
        for i, (img, y, x) in enumerate(impulse_pixels(case)):
            for hd, k in enumerate(ks):
                d_out[(img * h + y) * w + x, hd, i % k] = 1
        w2 = [np.where(a == 0, 1.0, a) for a in w2]
    keep = keep_of(case, drop, mask)
    scale = 1 if drop == 'none' else 2
    out = dict(d_out=d_out, hid=hid, mask=mask, keep=keep, scale=scale)
    if w2_dtn:
        rng = np.random.RandomState(7)
        w2 = [np.where(rng.random_sample(a.shape) < 0.25, UNREP[w2_dtn], a) for a in w2]
        out['w2_raw'] = w2
        out['ref_raw'] = head2_ref(d_out, hid, w2, keep, scale)
        w2 = [round_np(a, w2_dtn) for a in w2]
    out['w2'] = w2
    out['ref'] = head2_ref(d_out, hid, w2, keep, scale)
    if case.hs is not None:
        out['g44'], out['g44_abs'] = up_transposed(out['ref'].d_hid.reshape(n, h, w, -1), case.hs, case.ws)
    _CACHE[key] = out
    while len(_CACHE) > 2:                                  # (the workload case holds ~0.5 GB of float64)
        _CACHE.popitem(last=False)
    return out
