"""NumPy restatement of dbx_draw_overlay_batch (include/densebox_hip.h has the contract), written as a literal painter: the kept rows in
list order, per row the outline, the label background, the label text, the four discs and the inset, each assigned over what is there.
It shares nothing with the kernel's back-to-front search, carries its own font table and formats the score with '%.3f'."""
import math

import numpy as np

CHARS = '0123456789.-# '
_ART = {
    '0': '.###. #...# #..## #.#.# ##..# #...# .###.',
    '1': '..#.. .##.. ..#.. ..#.. ..#.. ..#.. .###.',
    '2': '.###. #...# ....# ...#. ..#.. .#... #####',
    '3': '.###. #...# ....# ..##. ....# #...# .###.',
    '4': '...#. ..##. .#.#. #..#. ##### ...#. ...#.',
    '5': '##### #.... ####. ....# ....# #...# .###.',
    '6': '..##. .#... #.... ####. #...# #...# .###.',
    '7': '##### ....# ...#. ..#.. .#... .#... .#...',
    '8': '.###. #...# #...# .###. #...# #...# .###.',
    '9': '.###. #...# #...# .#### ....# ...#. .##..',
    '.': '..... ..... ..... ..... ..... .##.. .##..',
    '-': '..... ..... ..... ##### ..... ..... .....',
    '#': '.#.#. .#.#. ##### .#.#. ##### .#.#. .#.#.',
    ' ': '..... ..... ..... ..... ..... ..... .....',
}


def font():
    """uint8 [14][8]: row j of glyph g, bit i = column i; column 5 and row 7 are empty"""
    out = np.zeros((14, 8), np.uint8)
    for g, ch in enumerate(CHARS):
        for j, row in enumerate(_ART[ch].split()):
            out[g, j] = sum(1 << i for i, c in enumerate(row) if c == '#')
    return out


FONT = font()
STYLE = dict(box_color=(0, 215, 255), text_color=(225, 255, 255), mark_color=(0, 0, 255), thickness=2, radius=5, font_scale=2, inset_scale=1)


def label(score, track_id=None):
    score = float(score)
    head = '#%d ' % track_id if track_id is not None and track_id >= 0 else ''
    return head + ('%.3f' % score if math.isfinite(score) and abs(score) < 1000 else '---')


def usable(v):
    return math.isfinite(v) and abs(v) < 2.0 ** 30


def _rect(h, w, x0, x1, y0, y1):
    """the slices of the inclusive rectangle clipped to the frame (possibly empty)"""
    return slice(max(y0, 0), max(min(y1, h - 1) + 1, 0)), slice(max(x0, 0), max(min(x1, w - 1) + 1, 0))


def draw(img, dets, keep, track_id=None, crops=None, ok=None, style=None, count=None):
    """One frame: img uint8 [h, w, c]; dets float64 [n, 5|13]; keep the list of kept rows (an entry outside 0..n-1 paints nothing);
    track_id / ok / crops by list position, or None.  count: an int array [h, w] that is incremented once per row that paints the pixel.
    A colour of fewer than c entries is padded with zeros, as the style record is.  Returns the annotated copy."""
    st = dict(STYLE)
    st.update(style or {})
    out = np.array(img, copy=True)
    h, w, c = out.shape
    txt = np.array((tuple(st['text_color']) + (0,) * 4)[:c], np.uint8)
    mark = np.array((tuple(st['mark_color']) + (0,) * 4)[:c], np.uint8)
    box = np.array((tuple(st['box_color']) + (0,) * 4)[:c], np.uint8)
    t, r, s, m = st['thickness'], st['radius'], st['font_scale'], st['inset_scale']
    a = t // 2
    b = t - a
    dets = np.asarray(dets, np.float64)
    yy, xx = np.mgrid[:h, :w]
    for j, row_no in enumerate(keep):
        if row_no < 0 or row_no >= dets.shape[0]:
            continue
        row = [float(v) for v in dets[row_no]]
        if not all(usable(v) for v in row[:4]):
            continue
        touched = np.zeros((h, w), bool)
        X1, Y1, X2, Y2 = (int(v + 0.5) for v in row[:4])
        L, R, Tp, Bt = min(X1, X2), max(X1, X2), min(Y1, Y2), max(Y1, Y2)
        # outline
        outer = (xx >= L - a) & (xx <= R + a) & (yy >= Tp - a) & (yy <= Bt + a)
        inner = (xx >= L + b) & (xx <= R - b) & (yy >= Tp + b) & (yy <= Bt - b)
        out[outer & ~inner] = box
        touched |= outer & ~inner
        # label
        if s > 0:
            text = label(row[4], None if track_id is None else int(track_id[j]))
            tw, th = 6 * s * len(text), 8 * s
            sl = _rect(h, w, X1, X1 + tw + 3, Y1 - th - 5, Y1)
            out[sl] = box
            touched[sl] = True
            for k, ch in enumerate(text):
                g = FONT[CHARS.index(ch)]
                for gj in range(8):
                    for gi in range(6):
                        if (g[gj] >> gi) & 1:
                            x, y = X1 + 2 + (6 * k + gi) * s, Y1 - 2 - th + gj * s
                            out[_rect(h, w, x, x + s - 1, y, y + s - 1)] = txt
        # discs
        if dets.shape[1] == 13 and r >= 0:
            for q in range(4):
                vx, vy = row[5 + 2 * q], row[6 + 2 * q]
                if not (usable(vx) and usable(vy)):
                    continue
                cx, cy = int(vx), int(vy)
                disc = (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r
                out[disc] = mark
                touched |= disc
        # inset
        if crops is not None and ok[j]:
            crop = np.asarray(crops[j])
            oh, ow = crop.shape[:2]
            px, py = L - a, Bt + a + 2
            x0, x1, y0, y1 = max(px, 0), min(px + ow * m, w), max(py, 0), min(py + oh * m, h)
            if x0 < x1 and y0 < y1:
                ys = (np.arange(y0, y1) - py) // m
                xs = (np.arange(x0, x1) - px) // m
                out[y0:y1, x0:x1] = crop[ys][:, xs]
                touched[y0:y1, x0:x1] = True
        if count is not None:
            count += touched
    return out
