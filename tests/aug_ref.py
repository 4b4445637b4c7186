"""A literal NumPy restatement of the patch augmentation (include/densebox_hip.h, "training patch augmentation"): the five pixel
steps on a whole 240 x 240 patch, the label rule under a flip, the sanitising of a record and the device-mode parameter draws.
Everything is int64 NumPy or Python ints; `>>` on them is arithmetic (a floor) and `//` is only used on non-negative values.  The
hash is tests/patch_ref.py's (pinned there)."""
import numpy as np

import patch_ref as R

SIDE = 240
MASK = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
FIELDS = ('flags', 'blur', 'box_len', 'sat', 'contrast', 'brightness', 'curve', 'noise_amp', 'key_lo', 'key_hi', 'gain0', 'gain1', 'gain2',
          'res0', 'res1', 'res2')
IDENTITY = dict(flags=0, blur=0, box_len=3, sat=256, contrast=256, brightness=0, curve=-1, noise_amp=0, key_lo=0, key_hi=0,
                gain0=256, gain1=256, gain2=256, res0=0, res1=0, res2=0)
# dbx_patch_aug_cfg's fields in layout order (4 doubles, then int32)
CFG_DEFAULT = dict(p_flip=0.5, p_blur=0.3, p_curve=0.3, p_noise=0.5, kind_w=(1, 1, 1), box_lo=3, box_hi=9, sat_lo=154, sat_hi=358,
                   contrast_lo=179, contrast_hi=333, brightness_lo=-32, brightness_hi=32, gain_lo=230, gain_hi=282, noise_lo=0, noise_hi=12,
                   curve_lo=0, curve_hi=3, G=4)


def record(**kw):
    """A record as a dict, the identity where not given; gain=(a, b, c) and key=<64-bit int> are shorthands."""
    r = dict(IDENTITY)
    if 'gain' in kw:
        r['gain0'], r['gain1'], r['gain2'] = kw.pop('gain')
    if 'key' in kw:
        key = kw.pop('key') & MASK
        r['key_lo'], r['key_hi'] = s32(key & 0xFFFFFFFF), s32(key >> 32)
    assert set(kw) <= set(FIELDS), kw
    r.update(kw)
    return r


def s32(u):
    """The int32 that holds the 32 bits u."""
    return u - (1 << 32) if u >= (1 << 31) else u


def to_row(r):
    return np.array([r[k] for k in FIELDS], dtype=np.int32)


def from_row(row):
    return dict(zip(FIELDS, (int(v) for v in row)))


def clamp(v, lo, hi):
    return max(lo, min(hi, v))


def sanitize(r, G):
    r = dict(r)
    r['flags'] &= 3
    if r['blur'] < 0 or r['blur'] > 3:
        r['blur'] = 0
    if r['blur'] == 3 and (r['box_len'] < 3 or r['box_len'] > 9 or r['box_len'] % 2 == 0):
        r['blur'] = 0
    for k in ('sat', 'contrast', 'noise_amp', 'gain0', 'gain1', 'gain2'):
        r[k] = clamp(r[k], 0, 65535)
    r['brightness'] = clamp(r['brightness'], -255, 255)
    if r['curve'] < 0 or r['curve'] >= G:
        r['curve'] = -1
    r['res0'] = r['res1'] = r['res2'] = 0
    return r


def gamma_bank(gammas):
    """uint8 [G, 256]: round(255 * (v / 255) ** gamma)."""
    v = np.arange(256, dtype=np.float64) / 255.0
    return np.stack([np.rint(255.0 * v ** float(g)) for g in gammas]).astype(np.uint8) if len(gammas) else np.zeros((0, 256), np.uint8)


def _pad(img, r):
    """Edges replicated by r pixels on both axes."""
    return np.pad(img, ((r, r), (r, r), (0, 0)), mode='edge')


def blur(img, kind, L):
    """img int64 [240, 240, c] -> the blurred image."""
    if kind == 0:
        return img
    if kind == 3:
        h = L // 2
        p = _pad(img, h)[h:h + SIDE]
        s = sum(p[:, dx:dx + SIDE] for dx in range(L))
        return (2 * s + L) // (2 * L)
    w = [1, 2, 1] if kind == 1 else [1, 4, 6, 4, 1]
    r = len(w) // 2
    p = _pad(img, r)
    s = np.zeros_like(img)
    for dy in range(len(w)):
        for dx in range(len(w)):
            s = s + w[dy] * w[dx] * p[dy:dy + SIDE, dx:dx + SIDE]
    return (s + 8) >> 4 if kind == 1 else (s + 128) >> 8


def tone_table(r, k, curves):
    v = np.arange(256, dtype=np.int64)
    g = np.clip((v * r['gain%d' % k] + 128) >> 8, 0, 255)
    t = np.clip((((g - 128) * r['contrast'] + 128) >> 8) + 128 + r['brightness'], 0, 255)
    return curves[r['curve']].astype(np.int64)[t] if r['curve'] >= 0 else t


def noise_hash(key):
    """uint64 [240, 240]: mix(key + GOLD * (pixel index + 1)) in wrapping uint64."""
    with np.errstate(over='ignore'):
        x = np.uint64(key) + np.uint64(GOLD) * (np.arange(SIDE * SIDE, dtype=np.uint64) + np.uint64(1))
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x.reshape(SIDE, SIDE)


def noise_term(r, k):
    """int64 [240, 240]: the value step 5 adds to colour channel k before the clamp."""
    key = ((r['key_hi'] & 0xFFFFFFFF) << 32) | (r['key_lo'] & 0xFFFFFFFF)
    h = noise_hash(key)
    b0 = ((h >> np.uint64(16 * k)) & np.uint64(255)).astype(np.int64)
    b1 = ((h >> np.uint64(16 * k + 8)) & np.uint64(255)).astype(np.int64)
    d = (b0 + b1 - 255) * r['noise_amp']
    return np.where(d >= 0, (d + 128) >> 8, -((-d + 128) >> 8))


def augment(patch, rec, curves=None):
    """patch uint8 [240, 240, c], rec: a record dict (or an int32 row of 16) -> the augmented patch."""
    if not isinstance(rec, dict):
        rec = from_row(rec)
    curves = np.zeros((0, 256), np.uint8) if curves is None else np.asarray(curves, dtype=np.uint8).reshape(-1, 256)
    r = sanitize(rec, len(curves))
    c = patch.shape[2]
    K = min(c, 3)
    v = patch.astype(np.int64)
    if r['flags'] & 1:
        v = v[:, ::-1]
    v = blur(v, r['blur'], r['box_len'])
    v = v.copy()
    if c >= 3:
        Y = (v[..., 0] + 2 * v[..., 1] + v[..., 2] + 2) >> 2
        for k in range(K):
            v[..., k] = np.clip(Y + (((v[..., k] - Y) * r['sat'] + 128) >> 8), 0, 255)
    for k in range(K):
        v[..., k] = tone_table(r, k, curves)[v[..., k]]
    if r['noise_amp'] > 0:
        for k in range(K):
            v[..., k] = np.clip(v[..., k] + noise_term(r, k), 0, 255)
    return v.astype(np.uint8)


def flip_labels(row):
    """The 12 integers under a flip, or None where the flip is refused (a positive with an x outside 0..239)."""
    bx0, by0, bx1, by1, lux, luy, rux, ruy, rdx, rdy, ldx, ldy = (int(v) for v in row)
    if any(x < 0 or x > 239 for x in (bx0, bx1, lux, rux, rdx, ldx)):
        return None
    return [239 - bx1, by0, 239 - bx0, by1, 239 - rux, ruy, 239 - lux, luy, 239 - ldx, ldy, 239 - rdx, rdy]


def draw(cfg, seed, counter, s):
    """The device-mode record of slot s."""
    k = lambda j: R.draw_hash(seed, counter, s, j) >> 11                                       # noqa: E731
    on = lambda j, p: k(j) * 2.0 ** -53 < p                                                    # noqa: E731
    rng = lambda j, lo, hi: lo + k(j) % (hi - lo + 1)                                          # noqa: E731
    w0, w1, w2 = cfg['kind_w']
    kind = 0
    if w0 + w1 + w2 > 0:
        w = k(2) % (w0 + w1 + w2)
        kind = 1 if w < w0 else (2 if w < w0 + w1 else 3)
    key = R.draw_hash(seed, counter, s, 11)
    return record(flags=1 if on(0, cfg['p_flip']) else 0, blur=kind if on(1, cfg['p_blur']) else 0,
                  box_len=cfg['box_lo'] + 2 * (k(3) % ((cfg['box_hi'] - cfg['box_lo']) // 2 + 1)),
                  sat=rng(4, cfg['sat_lo'], cfg['sat_hi']), contrast=rng(5, cfg['contrast_lo'], cfg['contrast_hi']),
                  brightness=rng(6, cfg['brightness_lo'], cfg['brightness_hi']),
                  curve=rng(8, cfg['curve_lo'], cfg['curve_hi']) if on(7, cfg['p_curve']) else -1,
                  noise_amp=rng(10, cfg['noise_lo'], cfg['noise_hi']) if on(9, cfg['p_noise']) else 0, key=key,
                  gain=(rng(12, cfg['gain_lo'], cfg['gain_hi']), rng(13, cfg['gain_lo'], cfg['gain_hi']), rng(14, cfg['gain_lo'], cfg['gain_hi'])))


def plan(cfg, labels_in, count, params_in=None, seed=0, counter=0):
    """dbx_patch_aug_plan for slots 0 .. count - 1: dict of params int32 [count, 16], labels int32 [count, 12], bbox / vertices / label
    float32.  params_in: injected records (rows of 16 or dicts), or None for device mode."""
    params, labels = [], []
    for s in range(count):
        r = draw(cfg, seed, counter, s) if params_in is None else (params_in[s] if isinstance(params_in[s], dict) else from_row(params_in[s]))
        r = sanitize(r, cfg['G'])
        r['flags'] &= 1
        row = [int(v) for v in labels_in[s]]
        if r['flags'] & 1 and any(v != 0 for v in row):
            f = flip_labels(row)
            if f is None:
                r['flags'] = 2
            else:
                row = f
        params.append(to_row(r))
        labels.append(row)
    lab = np.asarray(labels, dtype=np.int32).reshape(-1, 12)
    return dict(params=np.asarray(params, dtype=np.int32).reshape(-1, 16), labels=lab,
                bbox=(lab[:, :4].astype(np.float64) / 4.0).astype(np.float32), vertices=(lab[:, 4:].astype(np.float64) / 4.0).astype(np.float32),
                label=lab.any(axis=1).astype(np.float32).reshape(-1, 1))


# The cases the suites share: each op alone at both ends of the default range, then all of them together.
KEY = 0x0123456789ABCDEF
CASES = [
    ('flip', record(flags=1)),
    ('binomial3', record(blur=1)), ('binomial5', record(blur=2)), ('box3', record(blur=3, box_len=3)), ('box9', record(blur=3, box_len=9)),
    ('sat_lo', record(sat=154)), ('sat_hi', record(sat=358)), ('sat_0', record(sat=0)),
    ('contrast_lo', record(contrast=179)), ('contrast_hi', record(contrast=333)),
    ('brightness_lo', record(brightness=-32)), ('brightness_hi', record(brightness=32)), ('brightness_min', record(brightness=-255)),
    ('gain_lo', record(gain=(230, 230, 230))), ('gain_hi', record(gain=(282, 282, 282))),
    ('curve_first', record(curve=0)), ('curve_last', record(curve=3)),
    ('noise_lo', record(noise_amp=1, key=KEY)), ('noise_hi', record(noise_amp=12, key=KEY)),
    ('all_binomial5', record(flags=1, blur=2, sat=358, contrast=333, brightness=-17, curve=1, noise_amp=12, key=KEY + 1, gain=(230, 256, 282))),
    ('all_box7', record(flags=1, blur=3, box_len=7, sat=154, contrast=179, brightness=32, curve=2, noise_amp=7, key=KEY + 2, gain=(282, 240, 230))),
]


def label_rows(n, seed):
    """n label rows as dbx_patch_plan could write them: positives (some with a 240 on the right edge) and all-zero negatives."""
    rs = np.random.RandomState(seed)
    rows = np.zeros((n, 12), np.int32)
    for s in range(n):
        if rs.randint(5) == 0:
            continue
        x0, y0 = int(rs.randint(8, 100)), int(rs.randint(8, 100))
        x1, y1 = (240 if rs.randint(6) == 0 else int(rs.randint(x0 + 20, 240))), int(rs.randint(y0 + 10, 233))
        j = rs.randint(-3, 4, size=8)
        lu, ru, rd, ld = (x0 + abs(j[0]), y0 + abs(j[1])), (x1 - abs(j[2]), y0 + abs(j[3])), (x1, y1 - abs(j[5])), (x0, y1)
        rows[s] = [x0, y0, x1, y1, lu[0], lu[1], ru[0], ru[1], rd[0], rd[1], ld[0], ld[1]]
    return rows
