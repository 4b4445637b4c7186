"""A literal NumPy restatement of the training patch warp (include/densebox_hip.h, "training patch warp"): the sampler's hash and the
device-mode draws, the quad, the 8 x 8 solve, the cofactor inverse, the label rule, the sanitising of a record and the pixels of a whole
240 x 240 patch under both borders.  It imports nothing from the package or from oracle/.  Scalars are Python floats (IEEE float64, one
rounding per operation, no contraction) and Python ints; `>>` on them is arithmetic (a floor)."""
import math

import numpy as np

SIDE = 240
MASK = (1 << 64) - 1
QUAD_MAX = 1 << 20
HALF = 1912                                             # 119.5 pixels in 1/16 pixel
IDENTITY_QUAD = (0, 0, 3824, 0, 3824, 3824, 0, 3824)
SQUARE = (0.0, 0.0, 239.0, 0.0, 239.0, 239.0, 0.0, 239.0)
EYE = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
FIELDS = ('flags', 'border', 'fill', 'rot', 'q0', 'q1', 'q2', 'q3', 'q4', 'q5', 'q6', 'q7', 'scale', 'aspect', 'shear', 'reserved')
# dbx_patch_warp_cfg's fields in layout order (one double, then int32): data.Warp()'s defaults
CFG_DEFAULT = dict(p_warp=0.8, rot_lo=0, rot_hi=30, scale_lo=218, scale_hi=294, aspect_lo=230, aspect_hi=282, shear_lo=-26, shear_hi=26,
                   tx=128, ty=128, jitter=96, margin=8, border=1, fill=0, R=31)


def mix(x):
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def draw_hash(seed, counter, i, j):
    a = mix((seed + 0x9E3779B97F4A7C15 * (counter + 1)) & MASK)
    return mix((a + 0xD1B54A32D192ED03 * (i + 1) + 0x8CB92BA72F3D8DD7 * (j + 1)) & MASK)


def rot_bank(lo, hi):
    """int32 [hi - lo + 1, 2]: (rint(cos * 65536), rint(sin * 65536)) per whole degree."""
    t = np.deg2rad(np.arange(lo, hi + 1, dtype=np.float64))
    return np.stack([np.rint(np.cos(t) * 65536.0), np.rint(np.sin(t) * 65536.0)], axis=1).astype(np.int32)


def record(quad=IDENTITY_QUAD, flags=1, border=0, fill=0, rot=0, scale=256, aspect=256, shear=0, reserved=0):
    r = dict(flags=flags, border=border, fill=fill, rot=rot, scale=scale, aspect=aspect, shear=shear, reserved=reserved)
    for k in range(8):
        r['q%d' % k] = int(quad[k])
    return r


def s32(u):
    return u - (1 << 32) if u >= (1 << 31) else u


def pack_fill(*channels):
    """One byte per channel, channel ch in bits 8 ch .. 8 ch + 7, as the int32 that holds those bits."""
    return s32(sum((int(v) & 255) << (8 * k) for k, v in enumerate(channels)))


def to_row(r):
    return np.array([r[k] for k in FIELDS], dtype=np.int32)


def from_row(row):
    return dict(zip(FIELDS, (int(v) for v in row)))


def quad_of(r):
    return [r['q%d' % k] for k in range(8)]


def clamp(v, lo, hi):
    return max(lo, min(hi, v))


def sanitize(r):
    r = dict(r)
    r['flags'] &= 1
    if r['border'] < 0 or r['border'] > 1:
        r['border'] = 0
    for k in range(8):
        r['q%d' % k] = clamp(r['q%d' % k], -QUAD_MAX, QUAD_MAX)
    r['reserved'] = 0
    return r


def make_quad(cos, sin, scale, aspect, shear, tx=0, ty=0, jitter=(0,) * 8):
    """The eight 1/16-pixel integers of a drawn warp, in Python ints (unbounded, as the kernel's int64 never overflows here)."""
    q = []
    for k, (px, py) in enumerate(((-HALF, -HALF), (HALF, -HALF), (HALF, HALF), (-HALF, HALF))):
        u = (px * scale * aspect) >> 16
        v = (py * scale) >> 8
        u += (shear * v) >> 8
        x = (cos * u - sin * v + 32768) >> 16
        y = (sin * u + cos * v + 32768) >> 16
        q += [clamp(x + HALF + tx + jitter[2 * k], -QUAD_MAX, QUAD_MAX), clamp(y + HALF + ty + jitter[2 * k + 1], -QUAD_MAX, QUAD_MAX)]
    return q


def draw(cfg, bank, seed, counter, s):
    """The device-mode record of slot s."""
    k = lambda j: draw_hash(seed, counter, s, j) >> 11                                         # noqa: E731
    rng = lambda j, lo, hi: lo + k(j) % (hi - lo + 1)                                          # noqa: E731
    on = k(0) * 2.0 ** -53 < cfg['p_warp']
    r = record(flags=1 if on else 0, border=cfg['border'], fill=cfg['fill'], rot=rng(1, cfg['rot_lo'], cfg['rot_hi']),
               scale=rng(2, cfg['scale_lo'], cfg['scale_hi']), aspect=rng(3, cfg['aspect_lo'], cfg['aspect_hi']),
               shear=rng(4, cfg['shear_lo'], cfg['shear_hi']))
    if on:
        q = make_quad(int(bank[r['rot']][0]), int(bank[r['rot']][1]), r['scale'], r['aspect'], r['shear'], rng(5, -cfg['tx'], cfg['tx']),
                      rng(6, -cfg['ty'], cfg['ty']), [rng(7 + i, -cfg['jitter'], cfg['jitter']) for i in range(8)])
        for i in range(8):
            r['q%d' % i] = q[i]
    return r


def solve(src, dst):
    """cv2.getPerspectiveTransform's 8 x 8 system on float64 corner values (LU with partial pivoting): the 9 entries of M, or None
    where a pivot is not above 2^-52."""
    A = [[0.0] * 9 for _ in range(8)]
    for i in range(4):
        sx, sy, dx, dy = float(src[2 * i]), float(src[2 * i + 1]), float(dst[2 * i]), float(dst[2 * i + 1])
        A[i] = [sx, sy, 1.0, 0.0, 0.0, 0.0, -sx * dx, -sy * dx, dx]
        A[i + 4] = [0.0, 0.0, 0.0, sx, sy, 1.0, -sx * dy, -sy * dy, dy]
    for c in range(8):
        piv, best = c, abs(A[c][c])
        for r in range(c + 1, 8):
            if abs(A[r][c]) > best:
                best, piv = abs(A[r][c]), r
        if not best > 2.220446049250313e-16:
            return None
        if piv != c:
            A[c], A[piv] = A[piv], A[c]
        d = -1.0 / A[c][c]
        for r in range(c + 1, 8):
            f = A[r][c] * d
            for j in range(c + 1, 9):
                A[r][j] = A[r][j] + f * A[c][j]
    x = [0.0] * 8
    for r in range(7, -1, -1):
        acc = A[r][8]
        for j in range(r + 1, 8):
            acc = acc - A[r][j] * x[j]
        x[r] = acc / A[r][r]
    return x + [1.0]


def inverse(m):
    """The cofactor inverse, or None where the determinant is zero."""
    det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])
    if det == 0.0:
        return None
    d = 1.0 / det
    return [(m[4] * m[8] - m[5] * m[7]) * d, (m[2] * m[7] - m[1] * m[8]) * d, (m[1] * m[5] - m[2] * m[4]) * d,
            (m[5] * m[6] - m[3] * m[8]) * d, (m[0] * m[8] - m[2] * m[6]) * d, (m[2] * m[3] - m[0] * m[5]) * d,
            (m[3] * m[7] - m[4] * m[6]) * d, (m[1] * m[6] - m[0] * m[7]) * d, (m[0] * m[4] - m[1] * m[3]) * d]


def matrices(quad):
    """(M, inverse) of a quad in 1/16 pixel, or None where the slot is degenerate."""
    with np.errstate(all='ignore'):
        try:
            m = solve(SQUARE, [q / 16.0 for q in quad])
            im = inverse(m) if m is not None else None
        except (ZeroDivisionError, OverflowError):     # Python raises where C gives inf or NaN: not finite either way
            return None
    if m is None or im is None or not all(math.isfinite(v) for v in m + im):
        return None
    return m, im


def warp_labels(m, row, margin):
    """The 12 integers of a positive under M, or None where the label rule refuses."""
    v = []
    for k in range(4):
        vx, vy = int(row[4 + 2 * k]), int(row[5 + 2 * k])
        W = m[6] * vx + m[7] * vy + m[8]
        if not math.isfinite(W) or not W > 0.0:
            return None
        for a in (0, 3):
            f = (m[a] * vx + m[a + 1] * vy + m[a + 2]) / W + 0.5
            if not math.isfinite(f):
                return None
            i = int(f)                                 # truncated toward zero
            if i < margin or i > SIDE - 1 - margin:
                return None
            v.append(i)
    lux, luy, rux, ruy, rdx, rdy, ldx, ldy = v
    bx0, bx1, by0, by1 = min(lux, ldx), max(rux, rdx), min(luy, ruy), max(ldy, rdy)
    if bx1 <= bx0 or by1 <= by0:
        return None
    return [bx0, by0, bx1, by1] + v


def plan(cfg, labels_in, count, params_in=None, bank=None, seed=0, counter=0):
    """dbx_patch_warp_plan for slots 0 .. count - 1: dict of params int32 [count, 16], labels int32 [count, 12], bbox / vertices / label
    float32, fwd / inv float64 [count, 9].  params_in: injected records (rows of 16 or dicts), or None for device mode."""
    params, labels, fwd, inv = [], [], [], []
    for s in range(count):
        r = draw(cfg, bank, seed, counter, s) if params_in is None else (params_in[s] if isinstance(params_in[s], dict) else from_row(params_in[s]))
        r = sanitize(r)
        row = [int(v) for v in labels_in[s]]
        m, im = EYE, EYE
        if r['flags'] & 1:
            mats = matrices(quad_of(r))
            if mats is None:
                r['flags'] = 4
            elif any(v != 0 for v in row):
                w = warp_labels(mats[0], row, cfg['margin'])
                if w is None:
                    r['flags'] = 2
                else:
                    row, (m, im) = w, mats
            else:
                m, im = mats
        params.append(to_row(r))
        labels.append(row)
        fwd.append(list(m))
        inv.append(list(im))
    lab = np.asarray(labels, dtype=np.int32).reshape(-1, 12)
    return dict(params=np.asarray(params, dtype=np.int32).reshape(-1, 16), labels=lab,
                bbox=(lab[:, :4].astype(np.float64) / 4.0).astype(np.float32), vertices=(lab[:, 4:].astype(np.float64) / 4.0).astype(np.float32),
                label=lab.any(axis=1).astype(np.float32).reshape(-1, 1), fwd=np.asarray(fwd, dtype=np.float64).reshape(-1, 9),
                inv=np.asarray(inv, dtype=np.float64).reshape(-1, 9))


def warp(patch, rec, im):
    """patch uint8 [240, 240, c], rec: a record dict (or an int32 row of 16) as the plan wrote it, im: the 9 entries of the slot's inverse
    -> the slot's output patch."""
    if not isinstance(rec, dict):
        rec = from_row(rec)
    r = sanitize(rec)
    if not r['flags'] & 1:
        return patch.copy()
    c = patch.shape[2]
    im = [float(v) for v in im]
    xs = np.arange(SIDE, dtype=np.float64)[None, :]
    ys = np.arange(SIDE, dtype=np.float64)[:, None]
    with np.errstate(all='ignore'):
        X0 = (im[0] * xs + im[1] * ys) + im[2]
        Y0 = (im[3] * xs + im[4] * ys) + im[5]
        W = (im[6] * xs + im[7] * ys) + im[8]
        W = np.where(W != 0.0, 32.0 / W, 0.0)
        fX = np.fmax(-2147483648.0, np.fmin(2147483647.0, X0 * W))      # C's fmin / fmax: a NaN operand is dropped
        fY = np.fmax(-2147483648.0, np.fmin(2147483647.0, Y0 * W))
    X = np.rint(fX).astype(np.int64)                   # nearest, ties to even
    Y = np.rint(fY).astype(np.int64)
    sx, sy, ax, ay = X >> 5, Y >> 5, X & 31, Y & 31
    w00, w01, w10, w11 = (32 - ax) * (32 - ay) * 32, ax * (32 - ay) * 32, (32 - ax) * ay * 32, ax * ay * 32
    fill = np.array([(r['fill'] >> (8 * ch)) & 255 for ch in range(c)], dtype=np.int64)

    def tap(yy, xx):
        v = patch[np.clip(yy, 0, SIDE - 1), np.clip(xx, 0, SIDE - 1)].astype(np.int64)
        if r['border'] == 1:
            return v
        ok = (yy >= 0) & (yy < SIDE) & (xx >= 0) & (xx < SIDE)
        return np.where(ok[..., None], v, fill)
    acc = (tap(sy, sx) * w00[..., None] + tap(sy, sx + 1) * w01[..., None] + tap(sy + 1, sx) * w10[..., None] +
           tap(sy + 1, sx + 1) * w11[..., None] + (1 << 14)) >> 15
    return np.clip(acc, 0, 255).astype(np.uint8)


def shifted(dx16, dy16):
    """The identity quad moved by (dx16, dy16) sixteenths of a pixel."""
    return [IDENTITY_QUAD[k] + (dx16 if k % 2 == 0 else dy16) for k in range(8)]


def _rot(deg, scale=256, aspect=256, shear=0):
    t = math.radians(deg)
    return make_quad(int(round(math.cos(t) * 65536.0)), int(round(math.sin(t) * 65536.0)), scale, aspect, shear)


# The records the suites share (name, quad); the last four are refused or degenerate by construction.
CASES = [
    ('identity', list(IDENTITY_QUAD)),
    ('shift_+3px', shifted(48, 0)), ('shift_-5px_down_2px', shifted(-80, 32)), ('shift_half', shifted(8, 0)), ('shift_frac', shifted(5, -11)),
    ('rot_+15', _rot(15)), ('rot_-15', _rot(-15)),
    ('scale_0.85', _rot(0, scale=218)), ('scale_1.15', _rot(0, scale=294)), ('aspect_shear', _rot(4, aspect=282, shear=-26)),
    ('jitter_keystone', [IDENTITY_QUAD[k] + j for k, j in enumerate((96, -96, -73, 51, 88, 96, -96, -14))]),
    ('strong_keystone', [640, 320, 3184, 0, 3824, 3824, 0, 3504]),
    ('outside', shifted(16 * 600, 16 * 300)),
    ('degenerate_equal_corners', [0, 0, 3824, 0, 3824, 0, 0, 3824]),
    ('degenerate_collinear', [0, 0, 1000, 1000, 2000, 2000, 3000, 3000]),
    ('non_convex', [0, 0, 3824, 0, 1200, 1200, 0, 3824]),
]


def label_rows(n, seed):
    """n label rows as dbx_patch_plan could write them: positives well inside the patch and all-zero negatives."""
    rs = np.random.RandomState(seed)
    rows = np.zeros((n, 12), np.int32)
    for s in range(n):
        if rs.randint(5) == 0:
            continue
        x0, y0 = int(rs.randint(60, 100)), int(rs.randint(70, 100))
        x1, y1 = int(rs.randint(x0 + 30, 180)), int(rs.randint(y0 + 12, 170))
        j = rs.randint(0, 4, size=8)
        lu, ru, rd, ld = (x0 + j[0], y0 + j[1]), (x1 - j[2], y0 + j[3]), (x1, y1 - j[5]), (x0, y1)
        rows[s] = [x0, y0, x1, y1, lu[0], lu[1], ru[0], ru[1], rd[0], rd[1], ld[0], ld[1]]
    return rows
