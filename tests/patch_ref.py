"""A literal Python restatement of the patch sampler's plan (include/densebox_hip.h, "training patch sampling"): the reference's
gen_pos_patch with format_4_vertices and bbox_from_vertices, the negative path of gen_pure_neg_patches with intersect_small, the
counter-based hash, and the slot scan.  Plain Python floats and ints, so the arithmetic is CPython's -- the thing the kernel has to
reproduce bit for bit.  tests/test_patch_ref.py pins this file against results recorded from the reference itself."""
import numpy as np

SIDE = 240
MASK = (1 << 64) - 1
ACCEPTED, RULE, DEGENERATE, EMPTY, OUTSIDE, NO_WINDOW, OVERLAP, CAPACITY = range(8)
SAT = 1000000000


def mix(x):
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def draw_hash(seed, counter, i, j):
    a = mix((seed + 0x9E3779B97F4A7C15 * (counter + 1)) & MASK)
    return mix((a + 0xD1B54A32D192ED03 * (i + 1) + 0x8CB92BA72F3D8DD7 * (j + 1)) & MASK)


def unit(h):
    return (h >> 11) * 2.0 ** -53


def uniform(h):
    return -1.0 + 2.0 * unit(h)


def rnd(x):
    """int(x + 0.5), saturated to +-10^9 as the int32 outputs need."""
    return max(-SAT, min(SAT, int(x + 0.5)))


def sort_vertices(vertices):
    """format_4_vertices; None where it raises IndexError."""
    vertices = [list(v) for v in vertices]
    left = sorted(vertices, key=lambda p: p[0])[:2]
    right = [p for p in vertices if p not in left]
    if len(right) < 2:
        return None
    lu = sorted(left, key=lambda p: p[1])[0]
    ld = [p for p in left if p != lu]
    ru = sorted(right, key=lambda p: p[1])[0]
    rd = [p for p in right if p != ru]
    if not ld or not rd:
        return None
    return [lu, ru, rd[0], ld[0]]


def positive(W, H, verts8, d0, d1, radius=15):
    """(status, (x0, y0, x1, y1), labels[12]) of gen_pos_patch on a W x H frame; window and labels are zeros where the header says so."""
    zero = (0, 0, 0, 0), [0] * 12
    v = [[int(verts8[2 * a]), int(verts8[2 * a + 1])] for a in range(4)]
    if any(x < 0 or x > W - 1 or y < 0 or y > H - 1 for x, y in v):
        return (OUTSIDE,) + zero
    s = sort_vertices(v)
    if s is None or not abs(d0) <= 1e100 or not abs(d1) <= 1e100:
        return (DEGENERATE,) + zero
    bbox = (min(s[0][0], s[3][0]), max(s[1][0], s[2][0]), min(s[0][1], s[1][1]), max(s[3][1], s[2][1]))
    cx = rnd(float(bbox[0] + bbox[1]) * 0.5)
    cy = rnd(float(bbox[2] + bbox[3]) * 0.5)
    bw, bh = float(bbox[1] - bbox[0]), float(bbox[3] - bbox[2])
    off_x, off_y = d0 * radius, d1 * radius
    pw, ph = 4.0 * bw, 4.0 * bh
    org = [cx - pw * 0.5 - off_x, cy - ph * 0.5 - off_y]
    end = [org[0] + pw, org[1] + ph]
    if org[0] < 0 or org[1] < 0:
        org = [org[0] if org[0] >= 0 else 0.0, org[1] if org[1] >= 0 else 0.0]
        pw, ph = end[0] - org[0], end[1] - org[1]
    if end[0] >= W or end[1] >= H:
        end = [end[0] if end[0] < W else float(W - 1), end[1] if end[1] < H else float(H - 1)]
        pw, ph = end[0] - org[0], end[1] - org[1]
    if pw == 0.0 or ph == 0.0:
        return (DEGENERATE,) + zero
    pts = [(bbox[0], bbox[2]), (bbox[1], bbox[3])] + [tuple(p) for p in s]
    labels = []
    for x, y in pts:
        labels += [rnd(((x - org[0]) / pw) * 240.0), rnd(((y - org[1]) / ph) * 240.0)]
    lu, ru, rd, ld = (labels[4 + 2 * a:6 + 2 * a] for a in range(4))
    if lu[0] < 8 or lu[1] < 8 or ru[0] > W - 8 or ru[1] < 8 or rd[0] > W - 8 or rd[1] > H - 8 or ld[0] < 8 or ld[1] > H - 8:
        return (RULE,) + zero
    win = (rnd(org[0]), rnd(org[1]), rnd(end[0]), rnd(end[1]))
    status = EMPTY if win[2] <= win[0] or win[3] <= win[1] else ACCEPTED
    return status, win, labels


def negative(W, H, plates8, d0, d1, th=0):
    """The negative crop centred on (d0, d1): intersect_small over the frame's plates (rows of 8 integers)."""
    zero = (0, 0, 0, 0), [0] * 12
    if W < 241 or H < 241 or not (120 <= d0 < W - 120) or not (120 <= d1 < H - 120) or d0 != int(d0) or d1 != int(d1):
        return (NO_WINDOW,) + zero
    cx, cy = int(d0), int(d1)
    boxes = [sort_vertices([[int(row[2 * a]), int(row[2 * a + 1])] for a in range(4)]) for row in plates8]
    if any(s is None for s in boxes):          # every plate is formatted before intersect_small runs
        return (DEGENERATE,) + zero
    for s in boxes:
        iw = min(s[2][0], cx + 120) - max(s[0][0], cx - 120)
        ih = min(s[2][1], cy + 120) - max(s[0][1], cy - 120)
        if iw < 0 or ih < 0:
            break
        if iw * ih > th:
            return (OVERLAP,) + zero
    return ACCEPTED, (cx - 120, cy - 120, cx + 120, cy + 120), [0] * 12


def plan(sizes, plates, plate0, M, n, cand=None, draws=None, seed=0, counter=0, neg_frac=0.1, radius=15, th=0):
    """dbx_patch_plan.  sizes: [(H, W)] per frame; plates int [P, 9]; cand / draws: the injected tables, or None for device mode.
    Returns a dict of numpy arrays: status, slot, cand, draws, count, tally, labels [count, 12], windows [count, 4], frames [count],
    kinds [count]."""
    plates = np.asarray(plates, dtype=np.int64).reshape(-1, 9)
    P, F = len(plates), len(sizes)
    status, slot = np.zeros(M, np.int32), np.full(M, -1, np.int32)
    cand_out, draws_out = np.zeros((M, 2), np.int32), np.zeros((M, 2), np.float64)
    labels, windows, frames, kinds = [], [], [], []
    accepted = 0
    for i in range(M):
        d0 = d1 = 0.0
        if cand is None:
            kind = 1 if (P == 0 or unit(draw_hash(seed, counter, i, 0)) < neg_frac) else 0
            index = (draw_hash(seed, counter, i, 1) >> 11) % (F if kind else P)
        else:
            kind, index = int(cand[i][0]), int(cand[i][1])
            d0, d1 = float(draws[i][0]), float(draws[i][1])
        frame = -1
        if kind not in (0, 1) or not 0 <= index < (F if kind else P):
            res = (DEGENERATE, (0, 0, 0, 0), [0] * 12)
        else:
            frame = index if kind else int(plates[index][0])
            H, W = sizes[frame]
            if kind == 0:
                if cand is None:
                    d0, d1 = uniform(draw_hash(seed, counter, i, 2)), uniform(draw_hash(seed, counter, i, 3))
                res = positive(W, H, plates[index][1:], d0, d1, radius)
            else:
                if cand is None and W > 240 and H > 240:
                    d0 = float(120 + (draw_hash(seed, counter, i, 2) >> 11) % (W - 240))
                    d1 = float(120 + (draw_hash(seed, counter, i, 3) >> 11) % (H - 240))
                res = negative(W, H, plates[plate0[frame]:plate0[frame + 1], 1:], d0, d1, th)
        st = res[0]
        if st == ACCEPTED:
            slot[i] = accepted
            if accepted < n:
                labels.append(res[2]); windows.append(res[1]); frames.append(frame); kinds.append(kind)
            else:
                st = CAPACITY
            accepted += 1
        status[i] = st
        cand_out[i] = (kind, index)
        draws_out[i] = (d0, d1)
    lab = np.asarray(labels, dtype=np.int32).reshape(-1, 12)
    return dict(status=status, slot=slot, cand=cand_out, draws=draws_out, count=min(accepted, n),
                tally=np.bincount(status, minlength=8).astype(np.int32), labels=lab,
                windows=np.asarray(windows, dtype=np.int32).reshape(-1, 4), frames=np.asarray(frames, dtype=np.int32),
                kinds=np.asarray(kinds, dtype=np.int32),
                bbox=(lab[:, :4].astype(np.float64) / 4.0).astype(np.float32),
                vertices=(lab[:, 4:].astype(np.float64) / 4.0).astype(np.float32),
                label=(1 - np.asarray(kinds, dtype=np.int32)).astype(np.float32).reshape(-1, 1))


def label_name(row):
    """The reference's file name for a label row (process_plate.py:823-825, :747)."""
    return 'frame_label_' + '_'.join(str(int(v)) for v in row) + '.jpg'
