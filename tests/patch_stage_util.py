"""What tests/test_hip_augment.py and tests/test_hip_warp.py share: byte-offset views inside an arena of sentinel bytes, the scene the
samplers cut from, the augmenter they run, and a snapshot of everything a sampler's stages wrote."""
import numpy as np
import torch

from densebox_amd import data

SENTINEL = 0xA5
GAMMAS = (0.6, 0.8, 1.25, 1.6)
SIZES = [(97, 131), (300, 300), (260, 900), (1080, 1920)]            # (H, W)


def _at_offset(n, c, offset, fill=None):
    """(arena, view): a uint8 [n, 240, 240, c] view that starts `offset` bytes into an arena of sentinel bytes."""
    size = n * 240 * 240 * c
    arena = torch.full((size + 64,), SENTINEL, dtype=torch.uint8, device='cuda')
    view = arena[offset:offset + size].view(n, 240, 240, c)
    if fill is not None:
        view.copy_(torch.from_numpy(fill))
    assert view.data_ptr() % 16 == offset % 16
    return arena, view


def _untouched(arena, offset, size):
    return bool((arena[:offset] == SENTINEL).all()) and bool((arena[offset + size:] == SENTINEL).all())


def _plate(rs, W, H):
    w, h = int(rs.randint(4, min(200, W // 3) + 1)), int(rs.randint(4, min(80, H // 3) + 1))
    x, y = int(rs.randint(0, W - w)), int(rs.randint(0, H - h))
    pts = [(x, y), (x + w, y), (x + w, y + h), (x, y + h)]
    return [v for k in rs.permutation(4) for v in pts[k]]


def _scene(seed=3):
    rs = np.random.RandomState(seed)
    frames = [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in SIZES]
    plates = [[_plate(rs, w, h) for _ in range(k)] for (h, w), k in zip(SIZES, (5, 4, 6, 12))]
    return frames, plates


def _augment():
    return data.Augment(flip=0.5, blur=0.6, curve=0.5, noise_p=0.6, gammas=GAMMAS, seed=23)


def _snap(s):
    """Clones of what the sampler's stages wrote in the last launch, in launch order, then of the cut's patches."""
    out = []
    if s.warp is not None:
        w = s.warp_plan
        out += [s.warped, w.labels_i32, w.bbox, w.vertices, w.labels, w.params, w.fwd, w.inv]
    if s.augment is not None:
        out += [s.aug_patches, s.aug.labels_i32, s.aug.bbox, s.aug.vertices, s.aug.labels, s.aug.params]
    return [t.clone() for t in out + [s.patches]]
