"""Float64 / NumPy CPU reference of the up-sampling, pooling and layout kernels of csrc/aux_ops.hip, written from the operations and not
from the kernels, with the premise under which a result has ZERO tolerance, the derived error bound where it has not, the case table of
tests/test_hip_aux_paths.py and a restatement of the host-side dispatch of dbx_upsample_bilinear_bwd (plan_ref).  The coefficient
arithmetic (bilin_coef: ATen's align_corners rule in float32), up_matrix, up_transposed, round_np and interval are heads_ref's.

Operations
  up_forward    y[n, oy, ox] = ly0 (lx0 a + lx1 b) + ly1 (lx0 c + lx1 d), a .. d the four source pixels, evaluated in float64 with the
                float32 coefficients; also the same sum over |terms|                                       (dbx_upsample_bilinear)
  up_backward   dx = up^T(dy) (heads_ref.up_transposed), zeroed where a gate is not positive                (dbx_upsample_bilinear_bwd)
  up_nchw_f32   the kernel's expression in NumPy float32, one correctly rounded operation after the other: top = lx0 a + lx1 b,
                bot = lx0 c + lx1 d, y = ly0 top + ly1 bot.  The kernel runs under fp contract(off): bit for bit
                                                                                                            (dbx_upsample_bilinear_nchw_f32)
  pool_forward  2x2 / stride 2 floor-mode maximum, the arg-max = the FIRST window element equal to the maximum in (0,0), (0,1), (1,0),
                (1,1) order, the nibble arg | 4 (max > 0), and pool_idx_bytes: channel c in byte c / 2, even channel = low nibble
                (the kernels' IdxWord -- 8 nibbles in a 32-bit word, 4 in a 16-bit word, little-endian -- is that byte order)
  pool_backward dy routed to the arg-max (zero where relu_gate and the maximum is not positive), every other pixel zero, the ragged
                last row / column of an odd map included; accumulate adds what dx held
  u8hwc         ((u8 / 255) - mean) / std in NumPy float32, then ONE rounding to T: three correctly rounded operations and no
                multiply-add that a compiler could contract: exact
  nchw_to_framed, nchw_to_framed_ch, framed_add_ch, framed_to_nchw: element by element.

Zero tolerance (assert_exact_premise).  Operands are small integers (dy, x in {-2 .. 2}; gates in {-1, 0, 1}).  On a geometry whose
coefficients are all multiples of 1/8 every product wy wx d is a multiple of 2**-6, every partial sum of them in any order and grouping
is a multiple of 2**-6 of magnitude below 2**18 -- 24 bits: exact in fp32 -- so every fp32 evaluation yields the float64 value and the
expected output is that value rounded ONCE to T (round_np), bit for bit.

Other geometries: E = K 2**-24 sum |w d|, K the longest chain of fp32 roundings one term passes through (to first order in 2**-24;
the second-order part, K**2 2**-48, is 2**-38 of the sum at K = 39).  Loads convert to fp32 exactly, the store's rounding is the
interval's round_T.  Per kernel, from its code:
  upsample_bwd_kernel, upsample_bwd_rows_kernel (acc += wy * wx * d over at most T = max_terms nonzero terms, the same order in both):
      wy = (y0 == iy ? ly0 : 0) + (y1 == iy ? ly1 : 0) rounds when both match (the reference adds them in float64)      1
      wx likewise                                                                                                        1
      wy * wx                                                                                                            1
      (wy wx) * d                                                                          1, or 0 when contracted into the add
      the adds: the first lands on 0 and is exact, the others round the partial sum that holds the term     T - 1, or T when contracted
      K = T + 3                                                                                      (K_flat = K_rows = max_terms + 3)
  upsample_bwd_walk_kernel (v += wa[r] * d over the R destination rows of a source-row pair, then c += l * v over the C destination
  columns that reach a source column: the l1 parts of the columns with x0 = col - 1 in `n`, rolled into `c`, then the l0 parts):
      wa (as wy above) 1, l (s_l0 = lx0 + lx1 when x1 == x0) 1, wa * d 1, the adds into v R - 1, l * v 1, the adds into c C - 1
      K = R + C + 3, with R the destination rows of a pair that carry weight for either of its rows (walk_rows) and C the largest
      number of destination columns with weight for one source column                                (K_walk = rows per pair + columns + 3)
  upsample_rows_kernel (ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d): the coefficients are the reference's own float32 values):
      lx0 * a 1, the inner add 1, ly0 * (..) 1, the outer add 1: a chain of 4 (fewer when contracted).  The test takes K = 8: all
      seven operations of the expression and the benefit of the doubt, still 2**-21 of sum |terms|.          (K_FWD = 8)
16-bit outputs must lie in [round_T(ref - E), round_T(ref + E)] (heads_ref.interval with that K), fp32 outputs within
E + ulp32(ref) / 2 of the reference (bounds: the float64 pair (lo, hi)).

Share of outputs whose interval holds more than one value of T (tests/test_aux_ref.py asserts <= 2.5 % in bf16, <= 10 % in f16), from
the reference alone, the dense content without a gate (a gate only turns outputs into exact zeros):
  case              K    bf16     f16          case                  K    bf16     f16
  walk-7rows        13   0.84 %   3.82 %       rows-2x-small-c       19   0.63 %   3.71 %
  walk-workload     13   0.59 %   2.65 %       flat-third            28   1.17 %   7.42 %
  rows-widest       39   1.50 %   7.00 %       fwd-2x-1320 (15 -> 30)  8   0.18 %   0.63 %
                                               fwd-5-12               8   0.24 %   0.24 %
(with the gate, which turns two thirds of the outputs into exact zeros, a third of these).

Reference times (NumPy): every case under 0.1 s except walk-rounds2 (2560 channels) at 0.2 s.  A case's data and references are
computed once (make_bwd / make_fwd cache them) and shared by the dtypes: f32 takes the first 4 cg of the 8 cg channels."""
import collections

import numpy as np

from heads_ref import bilin_coef, up_matrix, up_transposed, round_np, interval          # noqa: F401  (re-exported)

F32 = np.float32
VEC = {'bf16': 8, 'f16': 8, 'f32': 4}                       # channels per 16-byte lane
K_FWD = 8


# ---------------------------------------------------------------------------------------------------------------- up-sampling
def up_forward(x, ho, wo):
    """x [n][hi][wi][C] float64 -> (y, sum of |terms|) on [n][ho][wo][C]."""
    _, hi, wi, _ = x.shape
    y0, y1, ly0, ly1 = bilin_coef(ho, hi)
    x0, x1, lx0, lx1 = bilin_coef(wo, wi)
    ly0, ly1 = [a.astype(np.float64)[None, :, None, None] for a in (ly0, ly1)]
    lx0, lx1 = [a.astype(np.float64)[None, None, :, None] for a in (lx0, lx1)]

    def ev(v):
        r0, r1 = v[:, y0], v[:, y1]
        return ly0 * (lx0 * r0[:, :, x0] + lx1 * r0[:, :, x1]) + ly1 * (lx0 * r1[:, :, x0] + lx1 * r1[:, :, x1])
    return ev(np.asarray(x, dtype=np.float64)), ev(np.abs(x).astype(np.float64))


def up_backward(dy, hs, ws, gate=None, swap=False):
    """dy [n][h][w][C] -> (dx, sum of |terms|) on [n][hs][ws][C]; gate [n][hs][ws][C]: dx is zero where it is not positive."""
    dx, ab = up_transposed(np.asarray(dy, dtype=np.float64), hs, ws, swap)
    if gate is not None:
        dx, ab = np.where(gate > 0, dx, 0.0), np.where(gate > 0, ab, 0.0)
    return dx, ab


def up_nchw_f32(x, ho, wo):
    """x [planes][hi][wi] float32 -> [planes][ho][wo] float32, the kernel's operations one by one (NumPy rounds each to float32)."""
    x = np.asarray(x, dtype=F32)
    _, hi, wi = x.shape
    y0, y1, ly0, ly1 = bilin_coef(ho, hi)
    x0, x1, lx0, lx1 = bilin_coef(wo, wi)
    ly0, ly1 = ly0[None, :, None], ly1[None, :, None]
    lx0, lx1 = lx0[None, None, :], lx1[None, None, :]
    r0, r1 = x[:, y0], x[:, y1]
    top = (lx0 * r0[:, :, x0]).astype(F32) + (lx1 * r0[:, :, x1]).astype(F32)
    bot = (lx0 * r1[:, :, x0]).astype(F32) + (lx1 * r1[:, :, x1]).astype(F32)
    out = (ly0 * top).astype(F32) + (ly1 * bot).astype(F32)
    assert out.dtype == F32 and top.dtype == F32
    return out


def nonzero_counts(out_size, in_size):
    """Per source index: how many destination indices carry weight for it."""
    return (up_matrix(out_size, in_size) != 0).sum(axis=0)


def max_terms(h, w, hs, ws):
    return int(nonzero_counts(h, hs).max() * nonzero_counts(w, ws).max())


def walk_rows(h, hs):
    """Destination rows that carry weight for either row of a source-row pair, per pair (the walk kernel's row table)."""
    nz = up_matrix(h, hs) != 0
    return [int((nz[:, i] | nz[:, min(i + 1, hs - 1)]).sum()) for i in range(0, hs, 2)]


def k_bwd(kernel, h, w, hs, ws):
    """K of the module docstring for the backward kernel `kernel` (0 flat, 1 rows, 2 walk)."""
    if kernel == 2:
        return max(walk_rows(h, hs)) + int(nonzero_counts(w, ws).max()) + 3
    return max_terms(h, w, hs, ws) + 3


def ulp32(x):
    _, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(1.0, np.maximum(e - 1, -126) - 23)


def bounds(ref, ref_abs, dtn, K):
    """(lo, hi, share): float64 bounds a kernel's output must lie in, and the share of outputs where lo != hi (16-bit types: the
    interval of T values; fp32: ref -+ (E + ulp32(ref) / 2), share not meaningful and 1)."""
    if dtn == 'f32':
        E = K * 2.0 ** -24 * ref_abs + ulp32(ref) / 2
        return ref - E, ref + E, 1.0
    return interval(ref, ref_abs, dtn, K)


def exact_bounds(ref, dtn):
    r = round_np(ref, dtn)
    return r, r, 0.0


def assert_exact_premise(h, w, hs, ws, ref, ref_abs):
    """The premise of every exact case: coefficients in eighths, sums multiples of 2**-6 below 2**18."""
    for o, i in ((h, hs), (w, ws)):
        _, _, l0, l1 = bilin_coef(o, i)
        c = np.concatenate([l0, l1]).astype(np.float64) * 8
        assert np.array_equal(c, np.rint(c)), 'a coefficient of %d <- %d is no multiple of 1/8' % (i, o)
    assert np.array_equal(ref * 64, np.rint(ref * 64)) and np.array_equal(ref_abs * 64, np.rint(ref_abs * 64))
    assert float(ref_abs.max()) < 2 ** 18


# ---------------------------------------------------------------------------------------------------------------- pooling
def pool_forward(x):
    """x [n][h][w][C] -> (y, nib) on [n][h // 2][w // 2][C]: the maximum and the nibble arg | 4 (max > 0), arg = the first maximum."""
    n, h, w, C = x.shape
    ph, pw = h // 2, w // 2
    win = np.stack([x[:, 0:2 * ph:2, 0:2 * pw:2], x[:, 0:2 * ph:2, 1:2 * pw:2], x[:, 1:2 * ph:2, 0:2 * pw:2], x[:, 1:2 * ph:2, 1:2 * pw:2]])
    y = win.max(axis=0) if ph and pw else np.zeros((n, ph, pw, C))
    arg = np.argmax(win, axis=0) if ph and pw else np.zeros((n, ph, pw, C), dtype=np.int64)     # (np.argmax: the first maximum)
    return y, (arg | (4 * (y > 0))).astype(np.uint8)


def pool_idx_bytes(nib):
    """nib [n][ph][pw][C] -> the dense idx bytes [n][ph][pw][C / 2], flattened."""
    return (nib[..., 0::2] | (nib[..., 1::2] << 4)).astype(np.uint8).reshape(-1)


def pool_backward(nib, dy, h, w, old=None, relu_gate=False):
    """dx [n][h][w][C]: dy at the arg-max of its window (zero under relu_gate where bit 2 is clear), zero elsewhere, + old."""
    n, ph, pw, C = dy.shape
    dx = np.zeros((n, h, w, C))
    v = np.where((nib & 4) != 0, dy, 0.0) if relu_gate else dy
    for k in range(4):
        dx[:, (k >> 1):2 * ph:2, (k & 1):2 * pw:2] = np.where((nib & 3) == k, v, 0.0)
    return dx if old is None else dx + old


# ---------------------------------------------------------------------------------------------------------------- layout
def u8hwc(img, mean, std, dtn):
    """img uint8 [n][h][w][3] -> [n][h][w][3] float64 holding values of T."""
    v = img.astype(F32) / F32(255)
    v = (v - np.asarray(mean, dtype=F32)[None, None, None, :]).astype(F32)
    v = (v / np.asarray(std, dtype=F32)[None, None, None, :]).astype(F32)
    assert v.dtype == F32
    return round_np(v.astype(np.float64), dtn)


def nchw_to_framed(x, c, dtn):
    """x [n][c_src][h][w] float32 -> [n][h][w][c]: channels past c_src zero."""
    n, cs, h, w = x.shape
    out = np.zeros((n, h, w, c))
    for ch in range(cs):
        out[..., ch] = round_np(x[:, ch].astype(np.float64), dtn)
    return out


def nchw_to_framed_ch(frame, x, c_off, dtn):
    """frame [n][h][w][c] with channels [c_off, c_off + c_src) replaced by x [n][c_src][h][w]."""
    out = frame.copy()
    for ch in range(x.shape[1]):
        out[..., c_off + ch] = round_np(x[:, ch].astype(np.float64), dtn)
    return out


def framed_add_ch(dst, src, c_src_off, n_ch, c_dst_off, dtn):
    out = dst.copy()
    for j in range(n_ch):
        out[..., c_dst_off + j] = round_np(dst[..., c_dst_off + j] + src[..., c_src_off + j], dtn)
    return out


def framed_to_nchw(x):
    n, h, w, c = x.shape
    out = np.zeros((n, c, h, w))
    for ch in range(c):
        out[:, ch] = x[..., ch]
    return out


# ---------------------------------------------------------------------------------------------------------------- the dispatch
Geo = collections.namedtuple('Geo', 'n h w pad ld c')
Plan = collections.namedtuple('Plan', 'kernel nseg workgroups lds_bytes')
FLAT, ROWS, WALK = 0, 1, 2


def ac_scale(in_size, out_size):
    return F32(in_size - 1) / F32(out_size - 1) if out_size > 1 else F32(0)


def plan_ref(dtn, dy, dx):
    """What dbx_upsample_bilinear_bwd_plan must report for the views dy (the up-sampled map's gradient) and dx (its source's)."""
    cg = dx.c // VEC[dtn]
    sy, sx = ac_scale(dx.h, dy.h), ac_scale(dx.w, dy.w)
    span = dy.n * (dy.h + 2 * dy.pad) * (dy.w + 2 * dy.pad) * dy.ld
    walk_ok = F32(0.45) < sy < 1 and F32(0.45) < sx < 1 and cg >= 64 and dy.w <= 4096 and span < 2 ** 32
    rows_ok = sy > F32(0.34) and sx > F32(0.34) and dx.w <= 1536
    if walk_ok:
        pairs, rounds = (dx.h + 1) // 2, (cg + 255) // 256
        nseg = max(min(12288 // (dx.n * pairs * 4 * rounds) + 1, dx.w // 8), 1)
        return Plan(WALK, nseg, dx.n * pairs * nseg, dy.w * 12)
    if rows_ok:
        return Plan(ROWS, 0, dx.n * dx.h, dx.w * 36)
    return Plan(FLAT, 0, min(max(-(-(dx.n * dx.h * dx.w * cg) // 256), 1), 8192), 0)


def seams(ws, nseg):
    """The walk kernel's column segments [c_lo, c_hi) of a source row."""
    return [(ws * s // nseg, ws * (s + 1) // nseg) for s in range(nseg)]


# ---------------------------------------------------------------------------------------------------------------- cases
# dx hs x ws <- dy h x w on n images of 8 cg (16-bit) / 4 cg (f32) channels; path / nseg: what the plan must say; exact: zero tolerance
Case = collections.namedtuple('Case', 'name n cg hs ws h w path nseg exact')
BWD = collections.OrderedDict((c.name, c) for c in [
    Case('walk-dyadic-1seg', 2, 64, 9, 9, 17, 17, WALK, 1, True),
    Case('walk-dyadic-segs', 1, 64, 6, 25, 11, 49, WALK, 3, True),
    Case('walk-rounds2', 1, 320, 4, 17, 7, 33, WALK, 2, True),
    Case('walk-7rows', 2, 64, 11, 17, 23, 33, WALK, 2, False),
    Case('walk-workload', 1, 64, 30, 30, 60, 60, WALK, 3, False),
    Case('rows-below-walk', 2, 63, 9, 9, 17, 17, ROWS, 0, True),
    Case('rows-identity', 1, 1, 7, 9, 7, 9, ROWS, 0, True),
    Case('rows-3/8', 2, 3, 4, 7, 9, 17, ROWS, 0, True),
    Case('rows-widest', 1, 2, 5, 5, 12, 12, ROWS, 0, False),
    Case('rows-2x-small-c', 3, 8, 15, 15, 30, 30, ROWS, 0, False),
    Case('flat-quarter', 2, 2, 3, 5, 9, 17, FLAT, 0, True),
    Case('flat-mixed', 1, 2, 9, 3, 17, 9, FLAT, 0, True),
    # down-sampling by 2: both scales are 2 > 0.34 and the dispatcher gives it to the tabulated kernel, not to the flat one; the
    # sources that receive no term (odd rows / columns) must be written 0 all the same
    Case('flat-down', 1, 2, 9, 9, 5, 5, ROWS, 0, True),
    # ... and down-sampling in y with a quarter scale in x: the flat kernel proper on rows that receive no term
    Case('flat-down-y', 1, 2, 9, 3, 5, 9, FLAT, 0, True),
    Case('flat-degenerate-out1', 1, 1, 4, 6, 1, 1, FLAT, 0, True),
    Case('flat-degenerate-in1', 1, 1, 1, 1, 5, 7, FLAT, 0, True),
    Case('flat-third', 1, 2, 4, 4, 10, 10, FLAT, 0, False),
])
VARIANTS = ['walk-dyadic-segs', 'rows-3/8', 'flat-quarter']     # one case per kernel for the view and impulse variants


def geos(case, dtn, dy_pad=0, dx_pad=1):
    c = case.cg * VEC[dtn]
    return Geo(case.n, case.h, case.w, dy_pad, c, c), Geo(case.n, case.hs, case.ws, dx_pad, c, c)


def impulse_pixels(case):
    """(image, row, column) of dy for the impulse variant: the four corners of the first and last image, the destination columns on
    either side of every segment seam (the last whose x0 is left of the seam and the first whose x0 is on it), the last column and
    the last row."""
    n, h, w = case.n, case.h, case.w
    px = [(i, y, x) for i in {0, n - 1} for y in {0, h - 1} for x in {0, w - 1}]
    px += [(0, h // 2, w - 1), (n - 1, h - 1, w // 2)]
    x0 = bilin_coef(w, case.ws)[0]
    for c_lo, _ in seams(case.ws, max(case.nseg, 1))[1:]:
        first = int(np.argmax(x0 >= c_lo))
        px += [(0, 1, first - 1), (0, 1, first), (n - 1, h - 2, first - 1), (n - 1, h - 2, first)]
    return sorted(set(px))


_CACHE = {}


def make_bwd(case, content='dense'):
    """dict(dy, gate, ref, ref_abs): dy [n][h][w][8 cg] in {-2 .. 2}, gate [n][hs][ws][8 cg] in {-1, 0, 1}, the float64 up^T(dy) WITHOUT
    the gate and its sum of |terms| (the gate is applied by the caller: np.where(gate > 0, ., 0)).  content 'impulse': dy zero but for
    single ones at impulse_pixels(case), pixel i in channel i % (4 cg) (so that the f32 slice sees it too)."""
    key = (case.name, content)
    if key not in _CACHE:
        rng = np.random.RandomState(2000 + sum(ord(ch) for ch in case.name))
        C = 8 * case.cg
        dy = rng.randint(-2, 3, size=(case.n, case.h, case.w, C)).astype(np.float64)
        if content == 'impulse':
            dy[:] = 0
            for i, (img, y, x) in enumerate(impulse_pixels(case)):
                dy[img, y, x, i % (4 * case.cg)] = 1
        gate = rng.randint(-1, 2, size=(case.n, case.hs, case.ws, C)).astype(np.float64)
        ref, ref_abs = up_backward(dy, case.hs, case.ws)
        _CACHE[key] = dict(dy=dy, gate=gate, ref=ref, ref_abs=ref_abs)
    return _CACHE[key]


def bwd_bounds(case, m, dtn, gated, kernel=None):
    """(lo, hi, share) of a backward case in dtype dtn: its first 4 cg channels for f32."""
    C = case.cg * VEC[dtn]
    ref, ab = m['ref'][..., :C], m['ref_abs'][..., :C]
    if gated:
        g = m['gate'][..., :C] > 0
        ref, ab = np.where(g, ref, 0.0), np.where(g, ab, 0.0)
    if case.exact:
        return exact_bounds(ref, dtn)
    return bounds(ref, ab, dtn, k_bwd(case.path if kernel is None else kernel, case.h, case.w, case.hs, case.ws))


# forward: x hi x wi -> y ho x wo on n images of cg groups; y.w * cg = 7 (one partial round), 1024 (exactly one trip), 1320 (a second
# loop trip with clamped loads), 1088 (the training call's 512-channel slice of a 768-wide frame)
FCase = collections.namedtuple('FCase', 'name n cg hi wi ho wo exact')
FWD = collections.OrderedDict((c.name, c) for c in [
    FCase('fwd-dyadic', 2, 64, 9, 9, 17, 17, True),
    FCase('fwd-identity-7', 1, 1, 3, 7, 3, 7, True),
    FCase('fwd-identity-1024', 2, 64, 5, 16, 5, 16, True),
    FCase('fwd-3/8', 2, 3, 4, 7, 9, 17, True),
    FCase('fwd-2x-1320', 1, 44, 15, 15, 30, 30, False),
    FCase('fwd-5-12', 2, 2, 5, 5, 12, 12, False),
    FCase('fwd-down', 1, 2, 9, 9, 5, 5, True),
    FCase('fwd-in1', 1, 1, 1, 1, 4, 6, True),
    FCase('fwd-out1', 1, 1, 5, 7, 1, 1, True),
])


def make_fwd(case):
    key = ('fwd', case.name)
    if key not in _CACHE:
        rng = np.random.RandomState(3000 + sum(ord(ch) for ch in case.name))
        x = rng.randint(-2, 3, size=(case.n, case.hi, case.wi, 8 * case.cg)).astype(np.float64)
        ref, ref_abs = up_forward(x, case.ho, case.wo)
        _CACHE[key] = dict(x=x, ref=ref, ref_abs=ref_abs)
    return _CACHE[key]


def fwd_bounds(case, m, dtn):
    C = case.cg * VEC[dtn]
    ref, ab = m['ref'][..., :C], m['ref_abs'][..., :C]
    return exact_bounds(ref, dtn) if case.exact else bounds(ref, ab, dtn, K_FWD)


def halves(seed, shape):
    """A map quantised to halves in [-2, 2] with about a quarter of it zero: ties and all-zero windows occur."""
    rng = np.random.RandomState(seed)
    return np.rint(rng.standard_normal(shape) * 2).clip(-4, 4) / 2 * (rng.random_sample(shape) < 0.75)
