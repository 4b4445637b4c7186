"""NumPy restatement of the score-threshold decode (dbx_detect_thresh_batch) for the tests, and the crafted maps they run on.

thresh_detect adds no arithmetic of its own: for n = min(#{score > t}, max_dets) the rows are the oracle's parse_det(K = n) and the
keep list the oracle's nms on them, so it inherits the oracle's pin to the reference (tests/test_oracle_golden.py).  Not collected."""
import numpy as np

from oracle import densebox_oracle as O


def thresh_detect(score, loc, lm_heat, lm_loc, M, N, t, max_dets, nms_thresh=0.4):
    """(dets float64 [n, 5|13], keep list, pixels above t) of one image's maps; the threshold compares in fp32, strictly"""
    s = np.asarray(score, np.float32).reshape(-1)
    total = int((s > np.float32(t)).sum())
    n = min(total, int(max_dets))
    dc = 5 if (lm_heat is None and lm_loc is None) else 13
    if n == 0:
        return np.zeros((0, dc), np.float64), [], total
    dets = O.parse_det(score, loc, M, N, K=n, lm_heat=lm_heat, lm_loc=lm_loc)
    return dets, O.nms(dets, nms_thresh), total


def score_grid(count, t=0.5):
    """`count` <= 4096 distinct fp32 scores above t = 0.5 and at most 1: t + k / 8192, every one exact in fp32"""
    assert t == 0.5 and 0 <= count <= 4096
    return (np.float32(0.5) + np.arange(1, count + 1, dtype=np.float32) / np.float32(8192.0)).astype(np.float32)


def craft_maps(seed, rows, cols, n_cand, plates, t=0.5):
    """One image's maps with exactly n_cand pixels above t: `plates` rectangles on a grid of cells, each lighting pixels of its centre
    region (round-robin over the plates until n_cand are lit) with scores drawn without repetition from score_grid; background
    scores below 0.4.  Loc maps: the exact offsets to the plate's corners plus an integer jitter in {-1, 0, 1} map pixels, so the
    boxes of one plate overlap far above 0.4 and those of different plates (two map pixels apart at least) do not.  Landmark
    offsets and heat maps are random.  Returns dict(score [1,1,r,c], loc [1,4,r,c], lm_heat [1,4,r,c], lm_loc [1,8,r,c]) fp32."""
    rs = np.random.RandomState(seed)
    gx = int(np.ceil(np.sqrt(plates * cols / rows)))
    gy = int(np.ceil(plates / gx))
    cw, ch = cols // gx, rows // gy
    assert cw >= 8 and ch >= 8, (rows, cols, plates)
    score = (rs.rand(rows, cols) * 0.4).astype(np.float32)
    loc = rs.randint(-6, 7, size=(4, rows, cols)).astype(np.float32)
    lists = []
    for p in range(plates):
        x0, y0 = (p % gx) * cw, (p // gx) * ch
        box = (x0 + 1, y0 + 1, x0 + cw - 2, y0 + ch - 2)
        xs = range(x0 + int(cw * 0.15), x0 + int(np.ceil(cw * 0.85)))
        ys = range(y0 + int(ch * 0.15), y0 + int(np.ceil(ch * 0.85)))
        pix = [(x, y, box) for y in ys for x in xs]
        rs.shuffle(pix)
        lists.append(pix)
    lit = []
    for k in range(max(len(l) for l in lists)):
        for l in lists:
            if k < len(l):
                lit.append(l[k])
    assert len(lit) >= n_cand, (len(lit), n_cand)
    vals = score_grid(n_cand, t)[rs.permutation(n_cand)]
    for (x, y, box), v in zip(lit[:n_cand], vals):
        score[y, x] = v
        j = rs.randint(-1, 2, size=4)
        loc[0, y, x] = x - (box[0] + j[0])
        loc[1, y, x] = y - (box[1] + j[1])
        loc[2, y, x] = x - (box[2] + j[2])
        loc[3, y, x] = y - (box[3] + j[3])
    lm_heat = rs.rand(4, rows, cols).astype(np.float32)
    lm_loc = (rs.randint(-40, 41, size=(8, rows, cols)) / 4.0).astype(np.float32)
    return dict(score=score[None, None], loc=loc[None], lm_heat=lm_heat[None], lm_loc=lm_loc[None])
