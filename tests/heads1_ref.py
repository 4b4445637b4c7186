"""Float64 CPU reference of the heads' FIRST stage -- the fused forward (dbx_heads_forward_fused / _heads: conv3x3_ws_kernel<T,1,1,2,4>
or conv3x3_p8_kernel<T,1,1> plus heads2_finish_kernel), dbx_heads1_wgrad_gen (wgrad_wide2_kernel<T,true>) and dbx_heads1_dgrad_gen
(heads1_dgrad_gen_kernel<T>), with their fp32 instantiations -- written from the maths and not from the kernels, with the premise under
which a kernel's result has ZERO tolerance, the case tables of tests/test_hip_heads1_paths.py, the impulse pixel lists and a
restatement of the host-side launch plans.  No GPU import.

The operation, for nh <= 4 heads of k_i <= 8 outputs over P = n h w pixels (compact pixel index p row-major over (image, row, column)):
  forward    hid[p, h]   = round_T(2 keep[p, h] (sum_c x[p, c] W1[h, c] + b1[h]))                          h < 512 nh, c < 768
             out_i[p, m] = b2[off_i + m] + sum_c round_T(W2_i)[m, c] hid[p, 512 i + c]                       fp32
  backward   d_hid[p, h] = round_T(scale keep[p, h] sum_{j < k_i} d_out[p, i, j] round_T(W2_i)[j, h - 512 i])   scale 2 with hash, else 1
             dW1[h, c]   = sum_p d_hid[p, h] x[p, c]         db1[h] = sum_p d_hid[p, h]                       fp32
             d_x[p, c]   = (gate[p, c] > 0) round_T(sum_h d_hid[p, h] W1[h, c])                               c: the 256 channels of the slice
keep = heads_ref.drop_keep(seed, P, 512 nh) on the COMPACT pixel index (the ws kernel walks frame positions of a pad-1 x but writes a
pad-0 hid; the weight-gradient generator walks the padded frame of x): a kernel that hashed a frame position fails on the first row.

Operands.  Content 'dense': integers -- x in {-1, 0, 1} (forward: nonzero with density 1/8) or {-3 .. 3} (x of the weight gradient), W1
in {-2 .. 2} (the data gradient: nonzero with Case.q1), b1 / b2 in {-3 .. 3}, d_out and W2 in {-2 .. 2}, gate in {-2 .. 2}; a quarter of
the W2 entries handed to the library are heads_ref.UNREP[T] (1 + 2**-9 / 1 + 2**-12: fp32 numbers T cannot hold, which round to 1): a
generator that multiplied by the unrounded value differs.  Content 'impulse': the same weights without zeros, the pixel operand (x
forward, d_out backward) zero but for single ones at the case's impulse pixels.  Content 'rounding': stored values that need more
bits than T has -- forward: |b1| in [2048, 4096), so the kept hid values are 2 v with v = x W1^T + b1 an integer of magnitude about 2000
to 4150 (hid itself reaches about +-8300); v is a number of T iff 2 v is: above 2048 the odd v are ties in f16 and only multiples
of 16 are bf16 numbers; backward: d_out channel 0 carries 2**11 times its value, so d_hid = scale (2**11 a
+ b) with small integers a, b and needs up to 18 bits; the data gradient: W1 in {-127 .. 127}, so d_x has a standard deviation of
several thousand.  The expected value is the exact one rounded ONCE to nearest-even (heads_ref.round_np).  All densities are fixed
in the tables and never adjusted at run time.

Premise (assert_sum_premise / assert_representable / rounding_stats, from the reference alone, before any launch):
 (a) every operand is an integer (unit 1) and every per-output sum of |products| (+ |bias|) is below 2**24: every partial sum a
     kernel can form, in any order and grouping (MFMA blocks, K tiles, waves, splits, the reduce kernels), is an integer below 2**24
     and exact in fp32.  Where the full |x| |W| product would double a reference's cost the bound is the coarser row sum
     max_p sum_c |x[p, c]| max |W| -- an upper bound of every per-output sum.
 (b) 'dense' / 'impulse': every stored 16-bit value (hid; d_hid, d_x) is a number of T (round_np(v) == v): the store cannot round, an
     error of one unit anywhere is visible.
 (c) 'rounding': at least 10 % of the stored values are not representable before their rounding and at least 16 are exact ties.

Reference times (NumPy float64, measured with 8 CPU threads, operands included; a reference is computed once per (case, content,
dropout) and shared by the dtypes -- a 'rounding' reference once per dtype): forward 0.6 s (f-nh4: 6068 pixels x 768 x 2048) to 1.6 s
(f-roundup: 28809 x 768 x 1024; 0.6 s for x W1^T, 0.9 s for the rounding check and the second convs); weight gradient 0.02 - 0.35 s
(b-empty-split is the largest); data gradient under 0.3 s for the four small cases, 1.9 s for c-two-tiles (76727 pixels x 1024
hidden channels: 0.45 s operands and keep bits, 1.4 s reference) and 2.3 s for c-three-tiles (153454 pixels x 512, nh = 1: 0.8 + 1.5 s;
nh = 1 keeps it there) -- none above 5 s.  keep_bits hashes once per 32-channel block (drop_keep, one hash per element, took 2 s of
c-two-tiles' time); dgrad_ref walks the pixels in chunks of 16384 so that d_hid never exceeds 134 MB."""
import collections

import numpy as np

from heads_ref import round_np, FMT, UNREP

SEED = 0x5EED1
DTN16 = ('bf16', 'f16')


def cdiv(a, b):
    return -(-a // b)


def keep_bits(seed, M, co):
    """heads_ref.drop_keep with one hash per (pixel, 32-channel block) instead of one per element (tests/test_heads1_ref.py pins the two
    to each other): bool [M][co], co a multiple of 32."""
    m64 = np.uint64(0xFFFFFFFF)
    m = np.arange(M, dtype=np.uint64)[:, None]
    c32 = np.arange(co // 32, dtype=np.uint64)[None, :]
    x = (np.uint64(seed) ^ ((m * np.uint64(0x9E3779B1)) & m64) ^ ((c32 * np.uint64(0x85EBCA77)) & m64)) & m64
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m64
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & m64
    x ^= x >> np.uint64(16)
    bits = np.unpackbits(x.astype('<u4').view(np.uint8).reshape(M, co // 32, 4), axis=2, bitorder='little')
    return bits.reshape(M, co).astype(bool)


# ---------------------------------------------------------------------------------------------------------------- premise helpers
def ulp_of(x, dtn):
    """Spacing of T at x (float64 array), as heads_ref.round_np derives it."""
    p, emin = FMT[dtn]
    _, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(1.0, np.maximum(e - 1, emin) - (p - 1))


def assert_integers(*arrays):
    for a in arrays:
        a = np.asarray(a, dtype=np.float64)
        assert np.array_equal(a, np.rint(a)), 'premise (a): an operand is no integer'


def assert_sum_premise(absum_max, what):
    assert float(absum_max) < 2 ** 24, 'premise (a): %s: a sum of |products| reaches %g >= 2**24: fp32 accumulation need not be exact' % (what, absum_max)


def assert_representable(v, dtn, what):
    v = np.asarray(v, dtype=np.float64)
    bad = round_np(v, dtn) != v
    assert not bad.any(), 'premise (b): %s: %d values are no %s numbers (the first: %r)' % (what, int(bad.sum()), dtn, float(v[bad][0]))


def rounding_stats(exact, dtn):
    """(share of values that are not representable before rounding, number of exact ties)."""
    exact = np.asarray(exact, dtype=np.float64)
    r = round_np(exact, dtn)
    off = np.abs(exact - r)
    return float((off != 0).mean()), int((off * 2 == ulp_of(exact, dtn)).sum())


def assert_rounding_premise(exact, dtn, what):
    share, ties = rounding_stats(exact, dtn)
    assert share >= 0.10, 'premise (c): %s: only %.3f of the stored values need rounding in %s' % (what, share, dtn)
    assert ties >= 16, 'premise (c): %s: only %d exact ties in %s' % (what, ties, dtn)
    return share, ties


# ---------------------------------------------------------------------------------------------------------------- cases
Fwd = collections.namedtuple('Fwd', 'name n h w ks premise')
FWD = collections.OrderedDict((c.name, c) for c in [
    Fwd('f-nh4', 2, 41, 74, (1, 4, 4, 8), 'p8 24 tiles of 7 (2) / 8 (22) units, last unit 20 pixels; ws exactly 192 items'),
    Fwd('f-nh1-k5', 2, 101, 121, (5,), 'k > 4 with one head; last unit 26'),
    Fwd('f-nh2', 2, 67, 91, (1, 4), 'the two-head model; last unit 2 pixels'),
    Fwd('f-nh3', 3, 47, 59, (3, 8, 2), 'odd head count, two seams, last unit 31'),
    Fwd('f-roundup', 3, 97, 99, (1, 4), 'p8 round-up branch (512 items)'),
])
# what the restated plan must say at 256 CUs: (p8 mt, base, extra, rounded, items, last-unit pixels, ws items)
FWD_AT_256 = {'f-nh4': (24, 7, 22, False, 192, 20, 192), 'f-nh1-k5': (96, 7, 92, False, 192, 26, 194), 'f-nh2': (48, 7, 46, False, 192, 2, 192),
              'f-nh3': (33, 7, 29, False, 198, 31, 198), 'f-roundup': (128, 7, 5, True, 512, 9, 456)}

Wg = collections.namedtuple('Wg', 'name n h w pad ks slot premise')
WG = collections.OrderedDict((c.name, c) for c in [
    Wg('b-min', 2, 9, 30, 1, (1, 4, 4, 8), 8, 'smallest legal frame: 32 padded columns'),
    Wg('b-ragged-seam', 3, 11, 35, 1, (1, 4, 4, 8), 16, 'h wp = 407 is no multiple of 32; splits cross both seams; the last split is short'),
    Wg('b-empty-split', 10, 11, 35, 1, (1, 4, 4, 8), 8, '130 steps in 15 splits of 9 -> 16 splits, the last one empty'),
    Wg('b-nh1', 3, 11, 35, 1, (8,), 16, 'one head'),
    Wg('b-nh3', 3, 11, 35, 1, (3, 8, 2), 8, 'three heads'),
    Wg('b-pad2', 2, 9, 31, 2, (1, 4, 4, 8), 16, 'a frame of pad 2'),
])
# at 256 CUs: (spi, steps_total, splits, steps_per_split)
WG_AT_256 = {'b-min': (9, 18, 2, 9), 'b-ragged-seam': (13, 39, 4, 10), 'b-empty-split': (13, 130, 16, 9), 'b-nh1': (13, 39, 4, 10),
             'b-nh3': (13, 39, 4, 10), 'b-pad2': (10, 20, 2, 10)}

Dg = collections.namedtuple('Dg', 'name n h w ks slot ypad gpad y_ld y_off q1 premise')
PIX_PER_IMAGE = 97 * 113


def dg_cases(cus):
    """The data-gradient cases; the two multi-tile ones are sized from the CU count (7 and 14 images of 97 x 113 at 256 CUs)."""
    n2 = cdiv(int(1.15 * cus * 256), PIX_PER_IMAGE)
    n3 = cdiv(int(2.30 * cus * 256), PIX_PER_IMAGE)
    return collections.OrderedDict((c.name, c) for c in [
        Dg('c-partial', 1, 9, 11, (8,), 8, 1, 0, 768, 512, 1 / 32, 'one partial tile: 99 pixels, waves 2 and 3 invalid'),
        Dg('c-256', 1, 16, 16, (1, 4), 16, 0, 1, 768, 512, 1 / 16, 'exactly 256 pixels'),
        Dg('c-513', 1, 19, 27, (3, 8, 2), 8, 1, 1, 768, 512, 1 / 32, 'npix % 256 == 1'),
        Dg('c-nh4', 2, 13, 17, (1, 4, 4, 8), 16, 0, 0, 768, 512, 1 / 32, 'four heads, a seam inside tile 0'),
        Dg('c-two-tiles', n2, 97, 113, (1, 4), 8, 1, 0, 320, 64, 1 / 32, 'ntiles in (ncu, 2 ncu), ragged last tile'),
        Dg('c-three-tiles', n3, 97, 113, (8,), 8, 0, 1, 320, 64, 1 / 32, 'ntiles in (2 ncu, 3 ncu), nh = 1'),
    ])


DG_SMALL = ('c-partial', 'c-256', 'c-513', 'c-nh4')


# ---------------------------------------------------------------------------------------------------------------- plans restated
def sched8(M, nt, cus, lo=7, full=8):
    """p8_schedule: tiles of lo .. full units of 32 pixels, their number rounded up to whole rounds of CUs."""
    units = cdiv(M, 32)
    mt = cdiv(units, full)
    rounded = False
    if mt * nt > cus:
        up = cdiv(mt * nt, cus) * cus // nt
        if up > mt and units // up >= lo:
            mt, rounded = up, True
    base, extra = units // mt, units % mt
    ok = extra == 0 if base == full else lo <= base < full
    return dict(ok=ok, mt=mt, base=base, extra=extra, items=mt * nt, rounded=rounded, units=units, last=M - 32 * (units - 1))


def fwd_plan(case, cus, xpad=1):
    """Which kernels take the fused forward of a case (heads_fused_shape_ok + the p8 / ws rules of conv_forward_t for the 1x1 heads GEMM
    768 -> 512 nh with bias + hash dropout, 16-bit): dict(shape_ok, p8, p8_ok, ws_items, ws_ok, fusable, kinds).  fusable: what
    dbx_heads_forward_fusable answers for plain weights (2 where the 8-phase kernel is preferred, else 1 where the ws kernel runs);
    kinds: every kernel a caller can get -- 2 with plain weights, 1 with DBX_CONV_WFRAG wherever the ws kernel can run the problem."""
    n, h, w, ks = case.n, case.h, case.w, case.ks
    nh, M, cin, cout = len(ks), case.n * case.h * case.w, 768, 512 * len(case.ks)
    shape_ok = 1 <= nh <= 4 and all(1 <= k <= 8 for k in ks)
    wp, hp = w + 2 * xpad, h + 2 * xpad
    sizes = M < 1 << 24 and n * hp * wp * cin * 2 < 1 << 32 and 64 * cin * 2 < 1 << 31 and M * cout < 1 << 32
    s = sched8(M, cout // 256, cus)
    p8_ok = bool(shape_ok and sizes and cin % 64 == 0 and (cin // 64) % 2 == 0 and 4 <= cin // 64 < 7000 and s['ok'] and s['items'] >= cus * 3 // 4)
    qtot = n * h * wp
    ws_items = (qtot // 256) * (cout // 256)
    ws_ok = bool(shape_ok and xpad <= 1 and cin % 128 == 0 and h * wp >= 256 + 8 and qtot < 1 << 30 and ws_items >= 192)
    return dict(shape_ok=shape_ok, p8=s, p8_ok=p8_ok, ws_items=ws_items, ws_ok=ws_ok, fusable=2 if p8_ok else (1 if ws_ok else 0),
                kinds=([2] if p8_ok else []) + ([1] if ws_ok else []))


def wgrad_plan_ref(case, cus):
    """wgrad_plan's wide2 branch for dz = 512 nh channels congruent with x (256 channels): 256 x 256 tiles, 32-row steps over the valid
    rows of each image (halo columns included), one round of workgroups."""
    wp = case.w + 2 * case.pad
    ntile = 2 * len(case.ks)
    compact = case.pad >= 1 and wp >= 32
    spi = cdiv(case.h * wp, 32) if compact else 0
    steps = case.n * spi if compact else cdiv(case.n * (case.h + 2 * case.pad) * wp, 32)
    sp = max(cus // ntile, 1)
    if sp > steps // 8:
        sp = max(steps // 8, 1)
    if sp >= 8:
        sp = sp // 8 * 8
    sps = cdiv(steps, sp)
    splits = cdiv(steps, sps)
    if sp >= 8 and splits % 8:
        splits = sp
    return dict(ok=compact, spi=spi, steps_total=steps if compact else 0, splits=splits, steps_per_split=sps if compact else 0, ntile=ntile,
                grid=ntile * splits, scratch=(splits * 512 * len(case.ks) * 256 + splits * 512 * len(case.ks)) * 4 + 256,
                empty=sum(1 for s in range(splits) if s * sps >= steps), short=steps % sps if compact else 0)


def dgrad_plan_ref(npix, cus):
    """heads1_dgrad_gen_kernel: tiles of 256 compact pixels, min(ntiles, CUs) persistent workgroups; workgroup g walks g, g + grid, ..."""
    ntiles = cdiv(npix, 256)
    grid = min(ntiles, cus)
    walks = [len(range(g, ntiles, grid)) for g in range(grid)]
    return dict(ntiles=ntiles, grid=grid, most=max(walks), least=min(walks), with_most=sum(1 for v in walks if v == max(walks)))


# ---------------------------------------------------------------------------------------------------------------- impulse pixels
def common_pixels(n, h, w):
    """Compact indices: corners of the first and last image, both sides of every image seam, column W - 1 | the next row's column 0 in
    a middle row of the first and the last image, the last pixel."""
    hw = h * w
    px = []
    for img in (0, n - 1):
        b = img * hw
        px += [b, b + w - 1, b + hw - w, b + hw - 1]
        r = h // 2
        px += [b + r * w + w - 1, b + (r + 1) * w if r + 1 < h else b + r * w]
    for img in range(1, n):
        px += [img * hw - 1, img * hw]
    px.append(n * hw - 1)
    return px


def frame_neighbours(n, h, w, pad, positions):
    """For frame positions (img, q) -- q row-major over the VALID rows of image img's frame, halo columns included, as the ws kernel and
    the weight-gradient generator walk them -- the nearest valid pixel strictly before q and the nearest at or after q."""
    wp, out = w + 2 * pad, []
    for img, q in positions:
        for qq, step in ((q - 1, -1), (q, 1)):
            while 0 <= qq < h * wp and not pad <= qq % wp < pad + w:
                qq += step
            if 0 <= qq < h * wp:
                out.append(img * h * w + (qq // wp) * w + qq % wp - pad)
    return out


def fwd_impulse_pixels(case, cus):
    """+ both sides of every 128-position ws tile boundary in the first image and of the last one in the last image (tiles over n h wp
    positions of the pad-1 frame rows), of the first three and the last 7|8-unit p8 tile boundaries (either order of the long tiles)."""
    n, h, w = case.n, case.h, case.w
    P, wp = n * h * w, w + 2
    px = common_pixels(n, h, w)
    qtot = n * h * wp
    bounds = [t * 128 for t in range(1, qtot // 128 + 1)]
    near = [b for b in bounds if b < h * wp][:6] + bounds[-2:]
    px += frame_neighbours(n, h, w, 1, [(b // (h * wp), b % (h * wp)) for b in near])
    s = sched8(P, 2 * len(case.ks), cus)
    for long_first in (True, False):
        sizes = ([s['base'] + 1] * s['extra'] + [s['base']] * (s['mt'] - s['extra'])) if long_first else \
                ([s['base']] * (s['mt'] - s['extra']) + [s['base'] + 1] * s['extra'])
        edges = np.cumsum(sizes)[:-1] * 32
        for e in list(edges[:3]) + list(edges[-1:]):
            px += [int(e) - 1, int(e)]
    return sorted({p for p in px if 0 <= p < P})


def wg_impulse_pixels(case, cus):
    """+ both sides of the first 32-row step boundaries of the first image, of every split boundary, of the last step of the last image."""
    n, h, w, pad = case.n, case.h, case.w, case.pad
    px = common_pixels(n, h, w)
    pl = wgrad_plan_ref(case, cus)
    pos = [(0, 32 * j) for j in range(1, min(pl['spi'], 4))] + [(n - 1, 32 * (pl['spi'] - 1))]
    for s in range(1, pl['splits']):
        g = s * pl['steps_per_split']
        if g < pl['steps_total']:
            pos.append((g // pl['spi'], 32 * (g % pl['spi'])))
    px += frame_neighbours(n, h, w, pad, [(i, q) for i, q in pos if q > 0])
    return sorted({p for p in px if 0 <= p < n * h * w})


def dg_impulse_pixels(case, cus):
    """+ both sides of pixel 255 | 256 and of the first tile every workgroup walks SECOND (256 grid - 1 | 256 grid), the wave boundaries
    of tile 0, the first pixel of the last tile."""
    P = case.n * case.h * case.w
    pl = dgrad_plan_ref(P, cus)
    px = common_pixels(case.n, case.h, case.w) + [63, 64, 127, 128, 255, 256, 511, 512, 256 * pl['grid'] - 1, 256 * pl['grid'],
                                                  256 * pl['grid'] + 255, 256 * pl['grid'] + 256, 512 * pl['grid'] - 1, 512 * pl['grid'],
                                                  256 * (pl['ntiles'] - 1) - 1, 256 * (pl['ntiles'] - 1)]
    return sorted({p for p in px if 0 <= p < P})


# ---------------------------------------------------------------------------------------------------------------- operands
def _seed(name):
    return 2000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name))


def w2_operands(rng, ks, content):
    """(W2 rounded: what the reference multiplies by, mask of the entries the library is handed as UNREP[T])."""
    w2 = [rng.randint(-2, 3, size=(k, 512)).astype(np.float64) for k in ks]
    if content == 'impulse':
        w2 = [np.where(a == 0, 1.0, a) for a in w2]
    un = [rng.random_sample(a.shape) < 0.25 for a in w2]
    w2 = [np.where(u, 1.0, a) for a, u in zip(w2, un)]
    return w2, un


def w2_raw(w2, un, dtn):
    """What the library is given: fp32 values; in a 16-bit type the masked entries are numbers T cannot hold that round to 1."""
    return [np.where(u, UNREP[dtn], a) if dtn != 'f32' else a for a, u in zip(w2, un)]


def dout_operands(rng, P, ks, content, pixels):
    d = np.zeros((P, len(ks), 8))
    if content == 'impulse':
        for i, p in enumerate(pixels):
            for hd, k in enumerate(ks):
                d[p, hd, i % k] = 1
        return d
    for hd, k in enumerate(ks):
        d[:, hd, :k] = rng.randint(-2, 3, size=(P, k))
    if content == 'rounding':
        d[:, :, 0] *= 2.0 ** 11
    return d


# ---------------------------------------------------------------------------------------------------------------- references
def fwd_pre(x, w1, b1):
    """(x W1^T + b1 in float64, the row-sum bound max_p sum_c |x[p, c]| max |W1| + max |b1| of every per-output sum of |products| + |bias|)."""
    pre = x.astype(np.float64) @ w1.T.astype(np.float64) + b1
    absum = float(np.abs(x).sum(axis=1, dtype=np.int64).max()) * float(np.abs(w1).max()) + float(np.abs(b1).max())
    return pre, absum


def fwd_ref(pre, keep, w2, b2, ks, dtn):
    """hid [P][512 nh] (rounded to T), the exact value before the rounding, out[i] [P][k_i], the largest sum of |W2 hid| + |b2|."""
    exact = 2.0 * keep * pre
    hid = round_np(exact, dtn)
    out, absum, off = [], 0.0, 0
    for i, k in enumerate(ks):
        hh = hid[:, 512 * i:512 * (i + 1)]
        out.append(hh @ w2[i].T + b2[off:off + k])
        absum = max(absum, float((np.abs(hh) @ np.abs(w2[i]).T).max() + np.abs(b2[off:off + k]).max()))
        off += k
    return hid, exact, out, absum


def dhid_exact(d_out, w2, keep, scale, lo=0, hi=None):
    """scale keep (d_out W2) for pixels [lo, hi): [hi - lo][512 nh] float64, before its rounding to T."""
    hi = d_out.shape[0] if hi is None else hi
    out = np.empty((hi - lo, 512 * len(w2)))
    for hd, a in enumerate(w2):
        k = a.shape[0]
        assert not d_out[lo:hi, hd, k:].any(), 'contract: d_out channels [k, 8) are zero'
        out[:, 512 * hd:512 * (hd + 1)] = d_out[lo:hi, hd, :k] @ a
    out *= scale
    if keep is not None:
        out *= keep[lo:hi]
    return out


WgRef = collections.namedtuple('WgRef', 'd_hid exact dw db absw absb')
DgRef = collections.namedtuple('DgRef', 'd_x exact absum')


def wgrad_ref(d_out, w2, keep, scale, x, dtn):
    """dW1 [512 nh][c], db1 [512 nh] from d_hid rounded to T, and the largest sums of |products|."""
    exact = dhid_exact(d_out, w2, keep, scale)
    d_hid = round_np(exact, dtn)
    xx = x.astype(np.float64)
    return WgRef(d_hid, exact, d_hid.T @ xx, d_hid.sum(axis=0), float((np.abs(d_hid).T @ np.abs(xx)).max()), float(np.abs(d_hid).sum(axis=0).max()))


def dgrad_ref(d_out, w2, keep, scale, w1t, gate, dtn, chunk=16384):
    """d_x [P][256] = (gate > 0) round_T(round_T(d_hid) W1^T), pixels in chunks; `exact`: the gated value before its rounding; absum: the
    row-sum bound max_p sum_h |d_hid[p, h]| max |W1| of every per-output sum of |products|."""
    P = d_out.shape[0]
    d_x, exact = np.empty((P, w1t.shape[1])), np.empty((P, w1t.shape[1]))
    absum, wmax = 0.0, float(np.abs(w1t).max())
    for lo in range(0, P, chunk):
        hi = min(lo + chunk, P)
        e = dhid_exact(d_out, w2, keep, scale, lo, hi)
        dh = e if float(np.abs(e).max()) <= 256 else round_np(e, dtn)     # (integer operands: integers to 256 are numbers of every T)
        absum = max(absum, float(np.abs(dh).sum(axis=1).max()) * wmax)
        g = gate[lo:hi] > 0
        exact[lo:hi] = (dh @ w1t) * g
        d_x[lo:hi] = round_np(exact[lo:hi], dtn)
    return DgRef(d_x, exact, absum)


# ---------------------------------------------------------------------------------------------------------------- a case's data
_CACHE = collections.OrderedDict()


def _cached(key, build, keep_n=2):
    if key in _CACHE:
        _CACHE.move_to_end(key)
        return _CACHE[key]
    _CACHE[key] = build()
    while len(_CACHE) > keep_n:
        _CACHE.popitem(last=False)
    return _CACHE[key]


def make_fwd(case, content, cus=256):
    """Operands and the dtype-independent part of the forward reference: dict(x, w1, b1, w2, un, b2, keep, pre, absum, pixels)."""
    def build():
        rng = np.random.RandomState(_seed(case.name))
        P, nh = case.n * case.h * case.w, len(case.ks)
        x = ((rng.randint(0, 2, size=(P, 768)) * 2 - 1) * (rng.random_sample((P, 768)) < 0.125)).astype(np.int8)
        w1 = rng.randint(-2, 3, size=(512 * nh, 768)).astype(np.int8)
        b1 = rng.randint(-3, 4, size=512 * nh).astype(np.float64)
        b2 = rng.randint(-3, 4, size=sum(case.ks)).astype(np.float64)
        w2, un = w2_operands(rng, case.ks, content)
        pixels = fwd_impulse_pixels(case, cus)
        if content == 'impulse':
            x[:] = 0
            for i, p in enumerate(pixels):
                x[p, (17 * i) % 768] = 1
            w1 = np.where(w1 == 0, 1, w1).astype(np.int8)
        if content == 'rounding':
            b1 = (rng.randint(2048, 4096, size=512 * nh) * (rng.randint(0, 2, size=512 * nh) * 2 - 1)).astype(np.float64)
        pre, absum = fwd_pre(x, w1, b1)
        return dict(x=x, w1=w1, b1=b1, w2=w2, un=un, b2=b2, keep=keep_bits(SEED, P, 512 * nh), pre=pre, absum=absum, pixels=pixels)
    return _cached(('fwd', case, content, cus), build)


def make_wg(case, drop, content, cus=256):
    """dict(d_out, x, w2, un, keep, scale, pixels) of a weight-gradient case (the reference itself depends on the dtype's rounding)."""
    def build():
        rng = np.random.RandomState(_seed(case.name))
        P, nh = case.n * case.h * case.w, len(case.ks)
        pixels = wg_impulse_pixels(case, cus)
        d_out = dout_operands(rng, P, case.ks, content, pixels)
        x = rng.randint(-1, 2, size=(P, 256)) if content == 'rounding' else rng.randint(-3, 4, size=(P, 256))
        w2, un = w2_operands(rng, case.ks, content)
        keep = keep_bits(SEED, P, 512 * nh) if drop == 'hash' else None
        return dict(d_out=d_out, x=x.astype(np.float64), w2=w2, un=un, keep=keep, scale=2 if drop == 'hash' else 1, pixels=pixels, refs={})
    m = _cached(('wg', case, drop, content, cus), build)
    return m


def wg_reference(m, dtn):
    """The reference for a dtype; in 'dense' / 'impulse' content d_hid is representable and one reference serves every dtype."""
    if dtn not in m['refs']:
        r = wgrad_ref(m['d_out'], m['w2'], m['keep'], m['scale'], m['x'], dtn)
        same = [t for t, o in m['refs'].items() if np.array_equal(o.d_hid, r.d_hid)]
        m['refs'][dtn] = m['refs'][same[0]] if same else r
    return m['refs'][dtn]


def make_dg(case, drop, content, cus=256):
    """dict(d_out, w1 [nh][512][768], w1t [512 nh][256], gate, w2, un, keep, scale, pixels, refs)."""
    def build():
        rng = np.random.RandomState(_seed(case.name))
        P, nh = case.n * case.h * case.w, len(case.ks)
        pixels = dg_impulse_pixels(case, cus)
        d_out = dout_operands(rng, P, case.ks, 'dense' if content == 'rounding' else content, pixels)
        w1 = np.full((nh, 512, 768), 3.0)                    # channels [0, 512) belong to other slices of the fusion map: never read
        if content == 'rounding':
            w1[:, :, 512:] = rng.randint(-127, 128, size=(nh, 512, 256))
        else:
            w1[:, :, 512:] = rng.randint(1, 3, size=(nh, 512, 256)) * (rng.randint(0, 2, size=(nh, 512, 256)) * 2 - 1) * \
                (rng.random_sample((nh, 512, 256)) < case.q1)
        gate = rng.randint(-2, 3, size=(P, 256)).astype(np.float64)
        w2, un = w2_operands(rng, case.ks, content)
        keep = keep_bits(SEED, P, 512 * nh) if drop == 'hash' else None
        return dict(d_out=d_out, w1=w1, w1t=np.ascontiguousarray(w1[:, :, 512:].reshape(512 * nh, 256)), gate=gate, w2=w2, un=un, keep=keep,
                    scale=2 if drop == 'hash' else 1, pixels=pixels, refs={})
    return _cached(('dg', case, drop, content, cus), build, keep_n=1)


def dg_reference(m, dtn):
    """The reference for a dtype.  One in which nothing was rounded serves every dtype that holds all of its values."""
    if dtn not in m['refs']:
        unrounded = [r for r in m['refs'].values() if np.array_equal(r.d_x, r.exact)]
        shared = [r for r in unrounded if np.array_equal(round_np(r.exact, dtn), r.exact)]
        m['refs'][dtn] = shared[0] if shared else dgrad_ref(m['d_out'], m['w2'], m['keep'], m['scale'], m['w1t'], m['gate'], dtn)
    return m['refs'][dtn]


# ---------------------------------------------------------------------------------------------------------------- fragment order
def frag_index_1x1(row, k, cin_pad, rows_pad):
    """The element index of (row, input channel k) in a dbx_pack_weight mode 4 / 5 image of a 1x1 layer, as include/densebox_hip.h and
    dbx_frag_index (csrc/common.hpp) define it: 1-KiB blocks [lane = 32 ((k % 16) / 8) + row % 32][k % 8], ordered
    [row / BN][k / 128][(k % 128) / 16][(row % BN) / 32] with BN = 256 where rows_pad is a multiple of 256, else 128.  Arrays broadcast."""
    row, k = np.asarray(row, dtype=np.int64), np.asarray(k, dtype=np.int64)
    bn = 256 if rows_pad % 256 == 0 else 128
    lane = 32 * ((k % 16) // 8) + row % 32
    blk = (((row // bn) * (cin_pad // 128) + k // 128) * 8 + (k % 128) // 16) * (bn // 32) + (row % bn) // 32
    return (blk * 64 + lane) * 8 + k % 8


def frag_image_1x1(matrix):
    """[rows_pad][cin_pad] -> the flat fragment-order image holding it."""
    rows_pad, cin_pad = matrix.shape
    img = np.zeros(rows_pad * cin_pad)
    idx = frag_index_1x1(np.arange(rows_pad)[:, None], np.arange(cin_pad)[None, :], cin_pad, rows_pad)
    assert np.array_equal(np.sort(idx.ravel()), np.arange(rows_pad * cin_pad)), 'the index is a permutation of the image'
    img[idx.ravel()] = matrix.ravel()
    return img


# ---------------------------------------------------------------------------------------------------------------- row recovery
def row_recovery_f32(q, wp):
    """genhid_pixel's frame row of position q in float32 arithmetic: fy = (int)((q + 0.5f) * inv_wp), inv_wp = 1.f / wp."""
    inv = np.float32(1.0) / np.float32(wp)
    return ((np.asarray(q).astype(np.float32) + np.float32(0.5)) * inv).astype(np.int64)
