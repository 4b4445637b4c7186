#!/usr/bin/env python
"""Records what the reference's patch cutters return, as the fixture tests/golden/patch_plan.npz (data only).

    python tools/gen_patch_golden.py --reference DIR [--out tests/golden/patch_plan.npz]

DIR holds the reference's process_plate.py.  The module is imported with stub modules for what it imports but the two functions
under test never need (cv2, torchvision, models, tqdm, PIL), and random.uniform is replaced by an iterator over the stored draws.
The cv2 stub's resize hands the slice back (and raises on an empty one, as OpenCV does; gen_pos_patch catches that and goes on), so
the shape of the returned patch IS the shape of the slice.

Positive cases call gen_pos_patch(img, ['x,y', ...]) and store W, H, the 8 vertex integers in the (permuted) annotation order, the
two draws, and: status 0 + the 12 label integers + the slice shape; status 1 where it returned None; status 2 where it raised
IndexError / ZeroDivisionError; status 3 where the returned slice is empty.  Negative cases run format_4_vertices on every plate and
intersect_small on the result, as gen_pure_neg_patches does, and store status 0 (True) or 6 (False)."""
import argparse
import contextlib
import importlib
import io
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_reference(ref_dir):
    def resize(patch, dsize=None, interpolation=None):
        if 0 in patch.shape:
            raise ValueError('empty source')
        return patch
    cv2 = types.ModuleType('cv2')
    cv2.resize = resize
    for k in ('INTER_LINEAR', 'INTER_CUBIC', 'INTER_AREA', 'INTER_NEAREST', 'INTER_LANCZOS4', 'IMREAD_UNCHANGED'):
        setattr(cv2, k, 0)
    stubs = {'cv2': cv2, 'tqdm': types.ModuleType('tqdm'), 'torchvision': types.ModuleType('torchvision'),
             'torchvision.transforms': types.ModuleType('torchvision.transforms'), 'models': types.ModuleType('models'),
             'PIL': types.ModuleType('PIL'), 'PIL.Image': types.ModuleType('PIL.Image'), 'PIL.ImageDraw': types.ModuleType('PIL.ImageDraw')}
    stubs['tqdm'].tqdm = lambda it, *a, **k: it
    stubs['torchvision'].transforms = stubs['torchvision.transforms']
    stubs['models'].LP_Net = object
    stubs['PIL'].Image, stubs['PIL'].ImageDraw = stubs['PIL.Image'], stubs['PIL.ImageDraw']
    sys.modules.update(stubs)
    sys.path.insert(0, ref_dir)
    with contextlib.redirect_stdout(io.StringIO()):
        return importlib.import_module('process_plate')


def run_positive(ref, W, H, verts8, draws):
    it = iter(draws)
    ref.random.uniform = lambda a, b: float(next(it))
    img = np.broadcast_to(np.uint8(0), (H, W, 3))
    strs = ['%d,%d' % (verts8[2 * a], verts8[2 * a + 1]) for a in range(4)]
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            patch, lu, rd, pts = ref.gen_pos_patch(img, strs)
    except (IndexError, ZeroDivisionError):
        return 2, [0] * 12, (0, 0)
    finally:
        ref.random.uniform = random.uniform
    if patch is None:
        return 1, [0] * 12, (0, 0)
    labels = list(lu) + list(rd) + [v for p in pts for v in p]
    shape = tuple(int(v) for v in patch.shape[:2])
    return (3 if 0 in shape else 0), [int(v) for v in labels], shape


def run_negative(ref, plates, centre, th):
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            boxes = [ref.format_4_vertices([[int(r[2 * a]), int(r[2 * a + 1])] for a in range(4)]) for r in plates]
            ok = ref.intersect_small(boxes, [int(centre[0]), int(centre[1])], th)
    except IndexError:
        return 2
    return 0 if ok else 6


def random_plate(rng, W, H):
    w, h = int(rng.randint(4, min(200, W - 1) + 1)), int(rng.randint(4, min(80, H - 1) + 1))
    x, y = int(rng.randint(0, W - w)), int(rng.randint(0, H - h))
    pts = [(x, y), (x + w, y), (x + w, y + h), (x, y + h)]
    pts = [(min(max(px + int(rng.randint(-4, 5)), 0), W - 1), min(max(py + int(rng.randint(-4, 5)), 0), H - 1)) for px, py in pts]
    return [v for k in rng.permutation(4) for v in pts[k]]


def hand_cases():
    """(W, H, verts8, draws): each clamp, the source-W/H quirk, equal x, equal vertices, a zero side, an empty slice."""
    def box(x0, y0, x1, y1):
        return [x0, y0, x1, y0, x1, y1, x0, y1]
    out = []
    for d in ((0.0, 0.0), (0.9, 0.9), (-0.9, -0.9), (0.999, -0.999)):
        out += [(640, 480, box(0, 200, 60, 230), d), (640, 480, box(300, 0, 380, 24), d), (640, 480, box(579, 200, 639, 230), d),
                (640, 480, box(300, 455, 380, 479), d), (640, 480, box(0, 0, 50, 20), d), (640, 480, box(589, 459, 639, 479), d)]
        out += [(247, 600, box(100, 300, 130, 312), d), (600, 247, box(300, 100, 330, 112), d), (200, 200, box(80, 90, 120, 104), d),
                (100, 1000, box(40, 500, 60, 508), d), (240, 240, box(100, 110, 140, 124), d), (248, 248, box(100, 110, 140, 124), d)]
        out += [(640, 480, [300, 200, 300, 230, 360, 202, 360, 228], d), (640, 480, [300, 200, 360, 200, 300, 230, 361, 231], d),
                (640, 480, [360, 228, 300, 230, 300, 200, 360, 202], d)]
        out += [(640, 480, [300, 200, 300, 200, 360, 230, 300, 230], d), (640, 480, [300, 200, 360, 200, 360, 200, 300, 230], d),
                (640, 480, [300, 200, 360, 230, 300, 230, 300, 200], d), (640, 480, [300, 200, 300, 200, 300, 200, 300, 200], d)]
        out += [(640, 480, [300, 200, 300, 210, 300, 220, 300, 230], d), (640, 480, [300, 200, 310, 200, 320, 200, 330, 200], d),
                (640, 480, [2, 200, 3, 200, 3, 204, 2, 204], d), (640, 480, [636, 200, 639, 200, 639, 204, 636, 204], d),
                (640, 480, [300, 1, 330, 1, 330, 3, 300, 3], d), (640, 480, [300, 476, 330, 476, 330, 479, 300, 479], d)]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='directory with the reference process_plate.py')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'patch_plan.npz'))
    ap.add_argument('--cases', type=int, default=2000)
    ap.add_argument('--seed', type=int, default=20240917)
    args = ap.parse_args()
    ref = load_reference(args.reference)
    rng = np.random.RandomState(args.seed)
    cases = []
    for _ in range(args.cases):
        W, H = int(rng.randint(60, 2001)), int(rng.randint(60, 1201))
        cases.append((W, H, random_plate(rng, W, H), tuple(rng.uniform(-1.0, 1.0, 2))))
    cases += hand_cases()
    rows = [run_positive(ref, W, H, v, d) for W, H, v, d in cases]
    neg = []
    for _ in range(400):
        W, H = int(rng.randint(241, 1401)), int(rng.randint(241, 1001))
        k = int(rng.randint(0, 4))
        plates = [random_plate(rng, W, H) for _ in range(k)]
        if k and rng.randint(0, 12) == 0:
            plates[-1][2:4] = plates[-1][0:2]                      # two equal vertices: format_4_vertices raises
        centre = (int(rng.randint(120, W - 120)), int(rng.randint(120, H - 120)))
        if k and rng.randint(0, 2):                                # half of them near a plate, so that both answers occur
            p = plates[int(rng.randint(0, k))]
            centre = (min(max(p[0] + int(rng.randint(-150, 151)), 120), W - 121), min(max(p[1] + int(rng.randint(-150, 151)), 120), H - 121))
        th = int(rng.choice([0, 0, 0, 50, 400]))
        neg.append((W, H, plates, centre, th, run_negative(ref, plates, centre, th)))
    padded = np.zeros((len(neg), 3, 8), np.int32)
    for i, r in enumerate(neg):
        for j, p in enumerate(r[2]):
            padded[i, j] = p
    status = np.array([r[0] for r in rows], np.int32)
    np.savez_compressed(
        args.out,
        pos_size=np.array([(W, H) for W, H, _, _ in cases], np.int32), pos_verts=np.array([v for _, _, v, _ in cases], np.int32),
        pos_draws=np.array([d for _, _, _, d in cases], np.float64), pos_status=status,
        pos_labels=np.array([r[1] for r in rows], np.int32), pos_shape=np.array([r[2] for r in rows], np.int32),
        pos_random=np.int32(args.cases),
        neg_size=np.array([(r[0], r[1]) for r in neg], np.int32), neg_nplates=np.array([len(r[2]) for r in neg], np.int32),
        neg_plates=padded, neg_centre=np.array([r[3] for r in neg], np.int32), neg_th=np.array([r[4] for r in neg], np.int32),
        neg_status=np.array([r[5] for r in neg], np.int32))
    print('positive: %d cases, status counts %s' % (len(rows), np.bincount(status, minlength=4).tolist()))
    print('negative: %d cases, status counts %s' % (len(neg), np.bincount([r[5] for r in neg], minlength=7).tolist()))
    print('%s: %d bytes' % (args.out, os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
