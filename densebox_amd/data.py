"""The input side of the hot path: the reference datasets' file-name labels and image transform.

The reference stores the label of a 240x240 patch in its file name, ``..._label_a_b_..`` (DenseBox.py:784-860, :927-970,
:1038-1052) and divides by 4 into the 60x60 output space; images go through torchvision's ToTensor + ImageNet
Normalize (DenseBox.py:766-772).  Here: the three label parsers (host string work, same results as the dataset
constructors) and the device-side transform, which is fused into the layout kernel -- pass uint8 ``[N,H,W,3]`` tensors to
``net.forward`` (``dbx_u8hwc_to_framed``).  JPEG decoding / directory walking stay out of scope.
"""
import ctypes as C
import re

import numpy as np
import torch

from . import _lib
from .rectify import frame_records, host_images, to_device

IMAGENET_MEAN = (0.485, 0.456, 0.406)   # DenseBox.py:770
IMAGENET_STD = (0.229, 0.224, 0.225)    # DenseBox.py:771

_PAT12 = re.compile('.*_label_' + '_'.join(['([0-9]+)'] * 12) + '.*')     # DenseBox.py:787-789, :928-930
_PAT4 = re.compile('.*_label_([0-9]+)_([0-9]+)_([0-9]+)_([0-9]+)')         # DenseBox.py:1038


def parse_densebox_label(img_name):
    """DenseBoxDataset (DenseBox.py:784-860): 12 integers -> (bbox[4], vertices[8], label[1]) float32 in 60-space;
    an all-zero label marks a negative patch (label 0, zero bbox / vertices)."""
    m = _PAT12.match(img_name)
    if m is None:
        raise ValueError('no 12-integer _label_ field in %r' % img_name)
    d = [float(m.group(i)) for i in range(1, 13)]
    if all(v == 0.0 for v in d):
        return np.zeros(4, np.float32), np.zeros(8, np.float32), np.zeros(1, np.float32)
    q = np.array([v / 4.0 for v in d])          # python float division, then FloatTensor(np.array(...)) -> float32
    return q[:4].astype(np.float32), q[4:].astype(np.float32), np.ones(1, np.float32)


def parse_lm_label(img_name):
    """LPPatchLM_Online (DenseBox.py:927-970): 12 integers -> (bbox[4], vertices[8]); no negative-patch handling."""
    m = _PAT12.match(img_name)
    if m is None:
        raise ValueError('no 12-integer _label_ field in %r' % img_name)
    q = np.array([float(m.group(i)) / 4.0 for i in range(1, 13)])
    return q[:4].astype(np.float32), q[4:].astype(np.float32)


def parse_bbox_label(img_name):
    """LPPatch_Online (DenseBox.py:1038-1052): 4 integers -> bbox[4]."""
    m = _PAT4.match(img_name)
    if m is None:
        raise ValueError('no 4-integer _label_ field in %r' % img_name)
    return np.array([float(m.group(i)) / 4.0 for i in range(1, 5)]).astype(np.float32)


def collate_labels(names):
    """File names -> (bbox[N,4], vertices[N,8], labels[N,1]) float32 tensors, DenseBoxDataset semantics + default collate."""
    b, v, l = zip(*[parse_densebox_label(n) for n in names])
    return torch.from_numpy(np.stack(b)), torch.from_numpy(np.stack(v)), torch.from_numpy(np.stack(l))


# ---------------------------------------------------------------------------------------------------------------------------
# Training patches sampled and cut on the device (dbx_patch_plan + dbx_patch_cut; include/densebox_hip.h, "training patch
# sampling"): the reference's gen_pos_patch and the negative path of gen_pure_neg_patches (process_plate.py:167-352, :711-749).
PATCH_SIDE = 240
MAX_CANDIDATES = 4096
PATCH_STATUS = ('accepted', 'landmark rule', 'degenerate', 'empty slice', 'vertex outside its frame', 'negative: no 240 x 240 window',
                'negative: overlaps a plate', 'accepted beyond the capacity')


def plate_tables(plates, n_frames):
    """plates: one list per frame of plates, a plate being 8 integers (4 (x, y) vertices in annotation order) or 4 pairs; or an int
    [P, 9] array of (frame, 8 integers) rows sorted by frame.  Returns the host tables (plates int32 [P, 9], plate0 int32
    [n_frames + 1]) of dbx_patch_plan, checked by dbx_patch_check_tables."""
    if isinstance(plates, np.ndarray) or torch.is_tensor(plates):
        rows = np.ascontiguousarray(plates.cpu().numpy() if torch.is_tensor(plates) else plates)
        if rows.ndim != 2 or rows.shape[1] != 9 or rows.dtype.kind not in 'iu':
            raise RuntimeError('plate_tables: a plate table must be an integer [P, 9] array, got %s %s' % (rows.dtype, list(rows.shape)))
        rows = rows.astype(np.int32)
    else:
        if len(plates) != n_frames:
            raise RuntimeError('plate_tables: %d lists of plates for %d frames' % (len(plates), n_frames))
        flat = []
        for f, ps in enumerate(plates):
            for p in ps:
                v = np.asarray(p).reshape(-1)
                if v.size != 8 or np.any(v != np.floor(v)):
                    raise RuntimeError('plate_tables: a plate must be 8 integers (4 (x, y) vertices), got %r in frame %d' % (p, f))
                flat.append([f] + [int(x) for x in v])
        rows = np.asarray(flat, dtype=np.int32).reshape(-1, 9)
    frames_of = rows[:, 0].astype(np.int64)
    plate0 = np.searchsorted(frames_of, np.arange(n_frames + 1), side='left').astype(np.int32)
    _lib.check(_lib.lib().dbx_patch_check_tables(rows.ctypes.data_as(C.c_void_p) if len(rows) else None, len(rows),
                                                 plate0.ctypes.data_as(C.c_void_p), n_frames, None, 0))
    return rows, plate0


class _LabelPlan(object):
    """The zeroed label outputs every plan launch writes: labels_i32 int32 [n, 12], bbox float32 [n, 4], vertices [n, 8], labels [n, 1]."""

    def __init__(self, n, device):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)
        self.n = int(n)
        self.labels_i32, self.bbox, self.vertices, self.labels = z((n, 12), torch.int32), z((n, 4), torch.float32), z((n, 8), torch.float32), \
            z((n, 1), torch.float32)


class PatchPlan(_LabelPlan):
    """The device tensors one dbx_patch_plan launch writes: jobs (uint8 [n, 96], dbx_patch_job records), labels_i32 int32 [n, 12],
    bbox float32 [n, 4], vertices [n, 8], labels [n, 1], count int32 [1], tally int32 [8], status / slot int32 [M], cand int32 [M, 2],
    draws float64 [M, 2].  Rows at or past count are not written (the tensors start zeroed)."""

    def __init__(self, M, n, device):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)
        _LabelPlan.__init__(self, n, device)
        self.M, self.jobs = int(M), z((n, 96), torch.uint8)
        self.count, self.tally = z((1,), torch.int32), z((8,), torch.int32)
        self.status, self.slot = z((max(M, 1),), torch.int32)[:M], z((max(M, 1),), torch.int32)[:M]
        self.cand, self.draws = z((max(M, 1), 2), torch.int32)[:M], z((max(M, 1), 2), torch.float64)[:M]


def plan_patches(table, n_frames, c, plates, plate0, M, n, cand=None, draws=None, state=None, neg_frac=0.1, offset_radius=15, th=0,
                 out=None):
    """The dbx_patch_plan launch alone, on the current stream; nothing is copied and nothing waits.  table: rectify.frame_table's
    device table; plates int32 [P, 9] / plate0 int32 [n_frames + 1]: device tensors (plate_tables, uploaded); cand int32 [M, 2] +
    draws float64 [M, 2] (injected mode) or state int64 [2] = (seed, counter) (device mode), device tensors.  Returns the PatchPlan
    (`out`, or a new one)."""
    out = out if out is not None else PatchPlan(M, n, table.device)
    io = _lib.PatchPlanIO()
    io.frames, io.plates, io.plate0 = table.data_ptr(), (plates.data_ptr() if plates.numel() else None), plate0.data_ptr()
    io.cand = cand.data_ptr() if cand is not None else None
    io.draws = draws.data_ptr() if draws is not None else None
    io.state = state.data_ptr() if state is not None else None
    io.jobs, io.labels, io.bbox, io.vertices, io.label = out.jobs.data_ptr(), out.labels_i32.data_ptr(), out.bbox.data_ptr(), \
        out.vertices.data_ptr(), out.labels.data_ptr()
    io.count, io.tally = out.count.data_ptr(), out.tally.data_ptr()
    if M:
        io.status, io.slot, io.cand_out, io.draws_out = out.status.data_ptr(), out.slot.data_ptr(), out.cand.data_ptr(), out.draws.data_ptr()
    _lib.check(_lib.lib().dbx_patch_plan(C.byref(io), int(n_frames), int(plates.numel() // 9), int(c), int(M), int(n), float(neg_frac),
                                         float(offset_radius), int(th), _lib.stream_ptr()))
    return out


def cut_patches(plan, c, patches=None):
    """The dbx_patch_cut launch alone: the plan's first `count` jobs into `patches` (uint8 [n, 240, 240, c], any byte alignment; a new
    zeroed tensor when None).  Slots at or past the count keep what they held."""
    if patches is None:
        patches = torch.zeros((plan.n, PATCH_SIDE, PATCH_SIDE, c), dtype=torch.uint8, device=plan.jobs.device)
    if patches.dtype != torch.uint8 or tuple(patches.shape) != (plan.n, PATCH_SIDE, PATCH_SIDE, c) or not patches.is_contiguous():
        raise RuntimeError('cut_patches: patches must be a contiguous uint8 [%d, 240, 240, %d] tensor, got %s %s'
                           % (plan.n, c, patches.dtype, list(patches.shape)))
    _lib.check(_lib.lib().dbx_patch_cut(C.c_void_p(plan.jobs.data_ptr()), C.c_void_p(plan.count.data_ptr()), plan.n, int(c),
                                        C.c_void_p(patches.data_ptr()), _lib.stream_ptr()))
    return patches


def _upload(*arrays):
    """The int32 / float64 host arrays as views of ONE uploaded buffer (each at an 8-byte boundary)."""
    offs, pos = [], 0
    for a in arrays:
        offs.append(pos)
        pos += (a.nbytes + 7) // 8 * 8
    host = np.zeros(max(pos, 8), np.uint8)
    for a, o in zip(arrays, offs):
        host[o:o + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    dev = torch.from_numpy(host).cuda()
    return [dev[o:o + a.nbytes].view(torch.from_numpy(a).dtype).view(a.shape) for a, o in zip(arrays, offs)]


def sample_patches(frames, plates, n, candidates=None, draws=None, neg_frac=0.1, offset_radius=15, seed=0, counter=0, m=None, th=0):
    """One upload + the two launches.  frames: as for resize.pad_resize_batch (host or device images of any sizes, C = 1..4);
    plates: as for plate_tables; n: the capacity.  Injected mode: candidates int [M, 2] = (kind, index) with draws float64 [M, 2];
    device mode (candidates None): m candidates (default ceil(1.5 n)) from the hash of (seed, counter).  Returns (patches uint8
    [n, 240, 240, C], plan): plan.count patches are valid, plan.bbox / vertices / labels are net.loss's inputs."""
    host, _ = host_images('sample_patches', frames, None)
    dev = to_device(frames, host)
    c = int(dev[0].size(2))
    rows, plate0 = plate_tables(plates, len(dev))
    if (candidates is None) != (draws is None):
        raise RuntimeError('sample_patches: candidates and draws go together (injected mode), or neither (device mode)')
    parts = [np.frombuffer(frame_records(dev), dtype=np.uint8), rows, plate0]
    if candidates is not None:
        cand = np.ascontiguousarray(np.asarray(candidates, dtype=np.int32).reshape(-1, 2))
        dr = np.ascontiguousarray(np.asarray(draws, dtype=np.float64).reshape(-1, 2))
        if len(cand) != len(dr):
            raise RuntimeError('sample_patches: %d candidates but %d rows of draws' % (len(cand), len(dr)))
        M = len(cand)
        _lib.check(_lib.lib().dbx_patch_check_tables(rows.ctypes.data_as(C.c_void_p) if len(rows) else None, len(rows),
                                                     plate0.ctypes.data_as(C.c_void_p), len(dev), cand.ctypes.data_as(C.c_void_p), M))
        parts += [cand, dr]
    else:
        M = int(m) if m is not None else min(MAX_CANDIDATES, (3 * int(n) + 1) // 2)
        parts += [np.array([seed, counter], dtype=np.int64)]
    up = _upload(*parts)
    table, d_rows, d_plate0 = up[0], up[1], up[2]
    if candidates is not None:
        plan = plan_patches(table, len(dev), c, d_rows, d_plate0, M, n, cand=up[3], draws=up[4], neg_frac=neg_frac,
                            offset_radius=offset_radius, th=th)
    else:
        plan = plan_patches(table, len(dev), c, d_rows, d_plate0, M, n, state=up[3], neg_frac=neg_frac, offset_radius=offset_radius, th=th)
    patches = cut_patches(plan, c)
    plan.keep = (dev, up)              # the table holds raw addresses: the frames live as long as the plan
    return patches, plan


# ---------------------------------------------------------------------------------------------------------------------------
# What the stages behind the cut share (the augmenter and the warper below; csrc/patch_stage.hpp is the device half): a plan launch
# that decides a 64-byte record and the label row per slot, and a pixel launch of a workgroup per 16-row band.
class _StagePlan(_LabelPlan):
    def __init__(self, n, device):
        _LabelPlan.__init__(self, n, device)
        self.params = torch.zeros((n, 16), dtype=torch.int32, device=device)


def _plan_stage(entry, io, labels_i32, count, cfg, params, state, out):
    """The io fields every stage's plan has, then the launch `entry` on the current stream; the caller has set the stage's own fields."""
    io.labels_in, io.count = labels_i32.data_ptr(), count.data_ptr()
    io.params_in = params.data_ptr() if params is not None else None
    io.state = state.data_ptr() if state is not None else None
    io.params, io.labels, io.bbox, io.vertices, io.label = out.params.data_ptr(), out.labels_i32.data_ptr(), out.bbox.data_ptr(), \
        out.vertices.data_ptr(), out.labels.data_ptr()
    _lib.check(entry(C.byref(io), C.byref(cfg), int(labels_i32.size(0)), _lib.stream_ptr()))
    return out


def _checked_out(who, patches, out):
    """The patches / out pair of a pixel launch, checked; returns out (a new zeroed tensor when None)."""
    if patches.dtype != torch.uint8 or patches.dim() != 4 or tuple(patches.shape[1:3]) != (PATCH_SIDE, PATCH_SIDE) or not patches.is_contiguous():
        raise RuntimeError('%s: patches must be a contiguous uint8 [n, 240, 240, c] tensor, got %s %s' % (who, patches.dtype, list(patches.shape)))
    if out is None:
        out = torch.zeros_like(patches)
    if out.dtype != torch.uint8 or out.shape != patches.shape or not out.is_contiguous():
        raise RuntimeError('%s: out must be a contiguous uint8 %s tensor, got %s %s' % (who, list(patches.shape), out.dtype, list(out.shape)))
    return out


def _stage_patches(patches, plan_or_labels, config, bank, params, counter, plan, apply, extras):
    """augment_patches and warp_patches: one upload + the two launches.  config: the Augment or Warp (its seed); bank: its host bank,
    flat; plan(labels_in, count, bank, params, state) and apply(patches, plan, count, bank): the stage's launches on the uploaded
    tensors (params None in device mode); extras: the plan's tensors returned after (out, labels_i32, bbox, vertices, labels)."""
    dev = (patches if torch.is_tensor(patches) else torch.from_numpy(np.ascontiguousarray(patches))).cuda()
    n = int(dev.size(0))
    parts = [bank, np.array([config.seed, counter], dtype=np.int64)]
    if params is not None:
        rec = params.cpu().numpy() if torch.is_tensor(params) else np.asarray(params)
        parts.append(np.ascontiguousarray(rec.astype(np.int32).reshape(n, 16)))
    from_plan = isinstance(plan_or_labels, PatchPlan)
    if not from_plan:
        rows = plan_or_labels.cpu().numpy() if torch.is_tensor(plan_or_labels) else np.asarray(plan_or_labels)
        parts += [np.ascontiguousarray(rows.astype(np.int32).reshape(n, 12)), np.array([n], dtype=np.int32)]
    up = _upload(*parts)
    labels_in, count = (plan_or_labels.labels_i32, plan_or_labels.count) if from_plan else (up[-2], up[-1])
    p = plan(labels_in, count, up[0], up[2] if params is not None else None, up[1])
    out = apply(dev, p, count, up[0])
    return (out, p.labels_i32, p.bbox, p.vertices, p.labels) + tuple(getattr(p, k) for k in extras)


# ---------------------------------------------------------------------------------------------------------------------------
# Photometric augmentation and horizontal flip of the cut patches on the device (dbx_patch_aug_plan + dbx_patch_augment;
# include/densebox_hip.h, "training patch augmentation").  The reference has no augmentation: the semantics are this project's own,
# restated in tests/aug_ref.py.
AUG_FIELDS = ('flags', 'blur', 'box_len', 'sat', 'contrast', 'brightness', 'curve', 'noise_amp', 'key_lo', 'key_hi', 'gain0', 'gain1', 'gain2',
              'reserved0', 'reserved1', 'reserved2')


def _q8(v):
    return int(round(float(v) * 256.0))


class Augment(object):
    """A plain config of the augmentation: probabilities and ranges, from which cfg() makes the dbx_patch_aug_cfg struct and curves()
    the uint8 [G, 256] bank of rounded gamma curves.  flip / blur / curve / noise_p: probabilities; saturation, contrast, gain:
    (lo, hi) factors, held in Q8; brightness: (lo, hi) grey levels; noise: (lo, hi) of the record's Q8 amplitude, which is also the peak
    deviation in grey levels; blur_kinds: integer weights of (binomial 3 x 3, binomial 5 x 5, horizontal box); box: (lo, hi) odd box
    lengths.  The defaults are a convention, not tuned: there are no trained weights in this tree to tune them against."""

    def __init__(self, flip=0.5, blur=0.3, saturation=(0.6, 1.4), contrast=(0.7, 1.3), brightness=(-32, 32), gain=(0.9, 1.1),
                 gammas=(0.6, 0.8, 1.25, 1.6), curve=0.3, noise=(0, 12), noise_p=0.5, seed=0, blur_kinds=(1, 1, 1), box=(3, 9)):
        self.flip, self.blur, self.curve, self.noise_p, self.seed = float(flip), float(blur), float(curve), float(noise_p), int(seed)
        self.saturation, self.contrast, self.gain = tuple(saturation), tuple(contrast), tuple(gain)
        self.brightness, self.noise, self.gammas = tuple(brightness), tuple(noise), tuple(float(g) for g in gammas)
        self.blur_kinds, self.box = tuple(int(w) for w in blur_kinds), tuple(int(b) for b in box)
        self._bank = None

    @classmethod
    def identity(cls, seed=0):
        """The no-op: every record it draws is the identity record, and the kernel copies."""
        return cls(flip=0.0, blur=0.0, saturation=(1.0, 1.0), contrast=(1.0, 1.0), brightness=(0, 0), gain=(1.0, 1.0), gammas=(), curve=0.0,
                   noise=(0, 0), noise_p=0.0, seed=seed)

    def cfg(self):
        f = _lib.PatchAugCfg()
        f.p_flip, f.p_blur, f.p_curve, f.p_noise = self.flip, self.blur, self.curve, self.noise_p
        f.kind_w[:] = self.blur_kinds
        f.box_lo, f.box_hi = self.box
        f.sat_lo, f.sat_hi = _q8(self.saturation[0]), _q8(self.saturation[1])
        f.contrast_lo, f.contrast_hi = _q8(self.contrast[0]), _q8(self.contrast[1])
        f.brightness_lo, f.brightness_hi = int(self.brightness[0]), int(self.brightness[1])
        f.gain_lo, f.gain_hi = _q8(self.gain[0]), _q8(self.gain[1])
        f.noise_lo, f.noise_hi = int(self.noise[0]), int(self.noise[1])
        f.G = len(self.gammas)
        f.curve_lo, f.curve_hi = 0, max(f.G - 1, 0)
        return f

    def curves(self):
        """uint8 [G, 256]: round(255 * (v / 255) ** gamma), made once on the host."""
        if self._bank is None:
            v = np.arange(256, dtype=np.float64) / 255.0
            self._bank = (np.stack([np.rint(255.0 * v ** g) for g in self.gammas]).astype(np.uint8) if self.gammas
                          else np.zeros((0, 256), np.uint8))
        return self._bank


class AugPlan(_StagePlan):
    """The device tensors one dbx_patch_aug_plan launch writes: params int32 [n, 16] (dbx_patch_aug records, AUG_FIELDS), labels_i32 int32
    [n, 12], bbox float32 [n, 4], vertices [n, 8], labels [n, 1].  Rows at or past the count are not written (the tensors start zeroed)."""


def plan_augment(labels_i32, count, cfg, params=None, state=None, out=None):
    """The dbx_patch_aug_plan launch alone, on the current stream.  labels_i32 int32 [n, 12] and count int32 [1]: device tensors (a
    PatchPlan's); cfg: Augment.cfg(); params int32 [n, 16] (injected mode) or state int64 [2] = (seed, counter) (device mode), device
    tensors.  Returns the AugPlan (`out`, or a new one)."""
    out = out if out is not None else AugPlan(labels_i32.size(0), labels_i32.device)
    return _plan_stage(_lib.lib().dbx_patch_aug_plan, _lib.PatchAugIO(), labels_i32, count, cfg, params, state, out)


def apply_augment(patches, params, count, curves, out=None):
    """The dbx_patch_augment launch alone: patches uint8 [n, 240, 240, c] (any byte alignment) through the records params int32 [n, 16]
    into `out` (a new zeroed tensor when None; it may not overlap patches).  curves: device uint8 [G, 256].  Slots at or past the count keep
    what they held."""
    out = _checked_out('apply_augment', patches, out)
    G = int(curves.size(0))
    _lib.check(_lib.lib().dbx_patch_augment(C.c_void_p(patches.data_ptr()), C.c_void_p(params.data_ptr()), C.c_void_p(count.data_ptr()),
                                            C.c_void_p(curves.data_ptr()) if G else None, G, int(patches.size(0)), int(patches.size(3)),
                                            C.c_void_p(out.data_ptr()), _lib.stream_ptr()))
    return out


def augment_patches(patches, plan_or_labels, augment=None, params=None, counter=0):
    """One upload + the two launches, for patches a user already has.  patches: uint8 [n, 240, 240, c], host or device; plan_or_labels: a
    PatchPlan (its label rows and count) or the int [n, 12] label rows (then all n slots count); augment: an Augment (None: the
    default one); params: int [n, 16] records (injected mode), else they are drawn from (augment.seed, counter).  Returns (out,
    labels_i32, bbox, vertices, labels, params): the augmented patches, the four label tensors and the records used."""
    augment = augment if augment is not None else Augment()
    G = len(augment.gammas)
    return _stage_patches(patches, plan_or_labels, augment, augment.curves().reshape(-1) if G else np.zeros(256, np.uint8), params, counter,
                          lambda rows, count, bank, rec, state: plan_augment(rows, count, augment.cfg(), params=rec, state=state),
                          lambda dev, plan, count, bank: apply_augment(dev, plan.params, count, bank.view(-1, 256)[:G]), ('params',))


# ---------------------------------------------------------------------------------------------------------------------------
# Geometric augmentation of the cut patches on the device (dbx_patch_warp_plan + dbx_patch_warp; include/densebox_hip.h, "training
# patch warp"): rotation, scale, aspect, shear, translation and keystone as one perspective map per patch, with the labels carried
# through it.  The reference has no augmentation: the semantics are this project's own, restated in tests/warp_aug_ref.py.
WARP_FIELDS = ('flags', 'border', 'fill', 'rot', 'quad0', 'quad1', 'quad2', 'quad3', 'quad4', 'quad5', 'quad6', 'quad7', 'scale', 'aspect',
               'shear', 'reserved')
WARP_IDENTITY_QUAD = (0, 0, 3824, 0, 3824, 3824, 0, 3824)
WARP_BORDERS = {'constant': 0, 'replicate': 1}


def _q4(v):
    return int(round(float(v) * 16.0))


class Warp(object):
    """A plain config of the geometric augmentation, from which cfg() makes the dbx_patch_warp_cfg struct and bank() the int32 [R, 2]
    table of (cos, sin) * 65536, one row per whole degree of `rotate`.  p: the probability that a slot is warped; rotate: (lo, hi) whole
    degrees, positive turning x towards y (clockwise on the screen); scale, aspect: (lo, hi) factors, held in Q8 (aspect multiplies the
    width alone); shear: (lo, hi) of the x-by-y shear, Q8; translate, jitter: pixels, held in 1/16 pixel -- every corner of the quad moves
    by the same translation and by a jitter of its own, which is what makes a keystone; margin: a positive whose warped vertices do not
    all lie in margin .. 239 - margin keeps its un-warped patch and labels (8 is the reference's landmark rule); border: 'replicate' or
    'constant' with fill, one byte per channel.  The defaults are a convention, not tuned: there are no trained weights in this tree to
    tune them against."""

    def __init__(self, p=0.8, rotate=(-15, 15), scale=(0.85, 1.15), aspect=(0.9, 1.1), shear=(-0.1, 0.1), translate=8, jitter=6, margin=8,
                 border='replicate', fill=(0, 0, 0, 0), seed=0):
        if border not in WARP_BORDERS:
            raise RuntimeError("Warp: border=%r must be 'constant' or 'replicate'" % (border,))
        fill = tuple(int(v) for v in (fill if np.ndim(fill) else (fill,) * 4))
        if len(fill) > 4 or any(v < 0 or v > 255 for v in fill):
            raise RuntimeError('Warp: fill=%r must be at most 4 bytes' % (fill,))
        if int(rotate[0]) != rotate[0] or int(rotate[1]) != rotate[1] or rotate[0] > rotate[1]:
            raise RuntimeError('Warp: rotate=%r must be whole degrees, lo <= hi' % (rotate,))
        self.p, self.seed, self.margin, self.border = float(p), int(seed), int(margin), border
        self.rotate, self.scale, self.aspect, self.shear = (int(rotate[0]), int(rotate[1])), tuple(scale), tuple(aspect), tuple(shear)
        self.translate, self.jitter, self.fill = float(translate), float(jitter), fill + (0,) * (4 - len(fill))
        self._bank = None

    @classmethod
    def identity(cls, seed=0):
        """The no-op: no slot is warped, every record carries the identity quad, and the kernel copies."""
        return cls(p=0.0, rotate=(0, 0), scale=(1.0, 1.0), aspect=(1.0, 1.0), shear=(0.0, 0.0), translate=0, jitter=0, seed=seed)

    def cfg(self):
        f = _lib.PatchWarpCfg()
        f.p_warp = self.p
        f.R = self.rotate[1] - self.rotate[0] + 1
        f.rot_lo, f.rot_hi = 0, f.R - 1
        f.scale_lo, f.scale_hi = _q8(self.scale[0]), _q8(self.scale[1])
        f.aspect_lo, f.aspect_hi = _q8(self.aspect[0]), _q8(self.aspect[1])
        f.shear_lo, f.shear_hi = _q8(self.shear[0]), _q8(self.shear[1])
        f.tx = f.ty = _q4(self.translate)
        f.jitter, f.margin, f.border = _q4(self.jitter), self.margin, WARP_BORDERS[self.border]
        f.fill = int(np.array(self.fill, dtype=np.uint8).view('<i4')[0])
        return f

    def bank(self):
        """int32 [R, 2]: (rint(cos * 65536), rint(sin * 65536)) of rotate[0] .. rotate[1] degrees, made once on the host."""
        if self._bank is None:
            t = np.deg2rad(np.arange(self.rotate[0], self.rotate[1] + 1, dtype=np.float64))
            self._bank = np.stack([np.rint(np.cos(t) * 65536.0), np.rint(np.sin(t) * 65536.0)], axis=1).astype(np.int32)
        return self._bank


class WarpPlan(_StagePlan):
    """The device tensors one dbx_patch_warp_plan launch writes: params int32 [n, 16] (dbx_patch_warp_rec records, WARP_FIELDS), labels_i32
    int32 [n, 12], bbox float32 [n, 4], vertices [n, 8], labels [n, 1], fwd / inv float64 [n, 9] (input -> output and output -> input;
    the exact identity for a slot that copies).  Rows at or past the count are not written (the tensors start zeroed)."""

    def __init__(self, n, device):
        _StagePlan.__init__(self, n, device)
        self.fwd, self.inv = torch.zeros((n, 9), dtype=torch.float64, device=device), torch.zeros((n, 9), dtype=torch.float64, device=device)


def plan_warp(labels_i32, count, cfg, bank=None, params=None, state=None, out=None):
    """The dbx_patch_warp_plan launch alone, on the current stream.  labels_i32 int32 [n, 12] and count int32 [1]: device tensors (a
    PatchPlan's); cfg: Warp.cfg(); bank: device int32 [R, 2] (Warp.bank(), uploaded); params int32 [n, 16] (injected mode) or state int64
    [2] = (seed, counter) (device mode), device tensors.  Returns the WarpPlan (`out`, or a new one)."""
    out = out if out is not None else WarpPlan(labels_i32.size(0), labels_i32.device)
    io = _lib.PatchWarpIO()
    io.rot = bank.data_ptr() if bank is not None and bank.numel() else None
    io.fwd, io.inv = out.fwd.data_ptr(), out.inv.data_ptr()
    return _plan_stage(_lib.lib().dbx_patch_warp_plan, io, labels_i32, count, cfg, params, state, out)


def apply_warp(patches, params, inv, count, out=None):
    """The dbx_patch_warp launch alone: patches uint8 [n, 240, 240, c] (any byte alignment) through the records params int32 [n, 16] and
    the matrices inv float64 [n, 9] into `out` (a new zeroed tensor when None; it may not overlap patches).  Slots at or past the count
    keep what they held."""
    out = _checked_out('apply_warp', patches, out)
    n = int(patches.size(0))
    if params.dtype != torch.int32 or params.numel() != 16 * n or inv.dtype != torch.float64 or inv.numel() != 9 * n \
            or not params.is_contiguous() or not inv.is_contiguous():
        raise RuntimeError('apply_warp: params must be int32 [%d, 16] and inv float64 [%d, 9], got %s %s and %s %s'
                           % (n, n, params.dtype, list(params.shape), inv.dtype, list(inv.shape)))
    _lib.check(_lib.lib().dbx_patch_warp(C.c_void_p(patches.data_ptr()), C.c_void_p(params.data_ptr()), C.c_void_p(inv.data_ptr()),
                                         C.c_void_p(count.data_ptr()), n, int(patches.size(3)), C.c_void_p(out.data_ptr()),
                                         _lib.stream_ptr()))
    return out


def warp_patches(patches, plan_or_labels, warp=None, params=None, counter=0):
    """One upload + the two launches, for patches a user already has.  patches: uint8 [n, 240, 240, c], host or device; plan_or_labels: a
    PatchPlan (its label rows and count) or the int [n, 12] label rows (then all n slots count); warp: a Warp (None: the default one);
    params: int [n, 16] records (injected mode), else they are drawn from (warp.seed, counter).  Returns (out, labels_i32, bbox, vertices,
    labels, params, fwd, inv): the warped patches, the four label tensors, the records used and the two matrices of every slot."""
    warp = warp if warp is not None else Warp()
    return _stage_patches(patches, plan_or_labels, warp, warp.bank().reshape(-1), params, counter,
                          lambda rows, count, bank, rec, state: plan_warp(rows, count, warp.cfg(), bank=bank.view(-1, 2), params=rec, state=state),
                          lambda dev, plan, count, bank: apply_warp(dev, plan.params, plan.inv, count), ('params', 'fwd', 'inv'))


class _SamplerStage(object):
    """A stage of a PatchSampler behind the cut: its uploaded bank, its own (seed, counter) state, its cfg struct, its plan and its pixel
    buffer.  NAMES: the sampler's attribute for each of them and for the plan's records.  launch(labels_i32, pixels, count) makes the stage's two launches on the
    stage before it and returns its own (labels_i32, pixels) for the next."""

    def __init__(self, config, bank, plan, like):
        flat, self.state = _upload(bank.reshape(-1) if len(bank) else np.zeros(256, np.uint8), np.array([config.seed, 0], dtype=np.int64))
        self.bank = flat.view(-1, bank.shape[1])[:len(bank)]
        self.cfg, self.plan, self.params, self.pixels = config.cfg(), plan, plan.params, torch.zeros_like(like)


class _WarpStage(_SamplerStage):
    NAMES = dict(bank='rot_bank', state='warp_state', cfg='warp_cfg', plan='warp_plan', params='warp_params', pixels='warped')

    def __init__(self, warp, n, like):
        _SamplerStage.__init__(self, warp, warp.bank(), WarpPlan(n, like.device), like)

    def launch(self, labels_i32, pixels, count):
        plan_warp(labels_i32, count, self.cfg, bank=self.bank, state=self.state, out=self.plan)
        apply_warp(pixels, self.plan.params, self.plan.inv, count, self.pixels)
        return self.plan.labels_i32, self.pixels


class _AugStage(_SamplerStage):
    NAMES = dict(bank='curves', state='aug_state', cfg='aug_cfg', plan='aug', params='aug_params', pixels='aug_patches')

    def __init__(self, augment, n, like):
        _SamplerStage.__init__(self, augment, augment.curves(), AugPlan(n, like.device), like)

    def launch(self, labels_i32, pixels, count):
        plan_augment(labels_i32, count, self.cfg, state=self.state, out=self.plan)
        apply_augment(pixels, self.plan.params, count, self.bank, self.pixels)
        return self.plan.labels_i32, self.pixels


class PatchSampler(object):
    """Fresh training patches every step with frames, tables, state and outputs resident on the device.  frames / plates: as for
    sample_patches; n: patches per batch; every batch decides ceil(oversample * n) candidates (at most 4096), of which a fraction
    neg_frac are pure negatives.  next_batch() is the two launches plus a 4-byte read of the count.  augment: an Augment; then
    launch() adds dbx_patch_aug_plan + dbx_patch_augment after the cut, into a second buffer of the sampler's, and next_batch() returns
    the augmented patches and labels; `raw` and `plan` still hold the un-augmented ones, `aug_params` the records used (int32 [n, 16]).
    The augmenter's state (augment.seed, counter) is its own: the plan's draws do not depend on it.  warp: a Warp; then launch() adds
    dbx_patch_warp_plan + dbx_patch_warp between the cut and the augmenter (cut -> warp -> augment: the augmenter reads the warp's label
    rows and pixels), into a buffer of the sampler's; `warped` holds the warped patches before any photometry, `warp_plan` their labels
    and matrices, `warp_params` the records used.  next_batch() returns the last stage's tensors.  The warper's state (warp.seed,
    counter) is its own as well."""

    def __init__(self, frames, plates, n, oversample=1.5, neg_frac=0.1, seed=0, offset_radius=15, th=0, allow_short=False, augment=None,
                 warp=None):
        if int(n) < 1 or not oversample >= 1.0:
            raise RuntimeError('PatchSampler: n=%r must be positive and oversample=%r at least 1' % (n, oversample))
        host, _ = host_images('PatchSampler', frames, None)
        self.frames = to_device(frames, host)
        self.c, self.n = int(self.frames[0].size(2)), int(n)
        self.M = min(MAX_CANDIDATES, int(np.ceil(float(oversample) * self.n)))
        rows, plate0 = plate_tables(plates, len(self.frames))
        self.table, self.plates, self.plate0, self.state = _upload(np.frombuffer(frame_records(self.frames), dtype=np.uint8), rows, plate0,
                                                                   np.array([seed, 0], dtype=np.int64))
        self.neg_frac, self.offset_radius, self.th, self.allow_short = float(neg_frac), offset_radius, int(th), bool(allow_short)
        self.plan = PatchPlan(self.M, self.n, self.table.device)
        self.patches = torch.zeros((self.n, PATCH_SIDE, PATCH_SIDE, self.c), dtype=torch.uint8, device=self.table.device)
        self.totals = torch.zeros(8, dtype=torch.int64, device=self.table.device)
        self.warp, self.augment = warp, augment
        self.warp_plan = self.warped = self.warp_params = self.aug_params = None
        self.stages = [cls(config, self.n, self.patches) for cls, config in ((_WarpStage, warp), (_AugStage, augment)) if config is not None]
        for stage in self.stages:                       # in launch order; the stage's tensors under the sampler's names for them
            for k, name in stage.NAMES.items():
                setattr(self, name, getattr(stage, k))

    @property
    def raw(self):
        """The un-augmented patches of the last batch (the sampler's own buffer)."""
        return self.patches

    def launch(self):
        """The launches (and the tally's accumulation) on the current stream, without any read: what a graph capture holds."""
        plan_patches(self.table, len(self.frames), self.c, self.plates, self.plate0, self.M, self.n, state=self.state,
                     neg_frac=self.neg_frac, offset_radius=self.offset_radius, th=self.th, out=self.plan)
        cut_patches(self.plan, self.c, self.patches)
        self.totals += self.plan.tally
        labels_i32, pixels = self.plan.labels_i32, self.patches
        for stage in self.stages:
            labels_i32, pixels = stage.launch(labels_i32, pixels, self.plan.count)

    def next_batch(self, allow_short=None):
        """(patches uint8 [n, 240, 240, C], bbox [n, 4], vertices [n, 8], labels [n, 1], count): net.forward's and net.loss's inputs.
        The tensors are the sampler's own and are overwritten by the next call.  Raises when fewer than n candidates were accepted,
        unless allow_short (here or at construction; then the first `count` rows are the batch: slice them)."""
        self.launch()
        count = int(self.plan.count.item())
        if count < self.n and not (self.allow_short if allow_short is None else allow_short):
            raise RuntimeError('PatchSampler: %d of %d candidates were accepted, fewer than n=%d; raise oversample (status tally: %s)'
                               % (count, self.M, self.n, self.plan.tally.tolist()))
        plan, pixels = (self.stages[-1].plan, self.stages[-1].pixels) if self.stages else (self.plan, self.patches)
        return pixels, plan.bbox, plan.vertices, plan.labels, count

    def status_tally(self):
        """{status name: candidates so far}, summed over every batch."""
        return dict(zip(PATCH_STATUS, self.totals.tolist()))
