"""Drop-in ``nn.Module`` front end for the three reference networks.

Same class names, constructor signature, attribute names, aliased ``state_dict``
key set/order and ``forward()`` tuple order as the reference:

  DenseBox       DenseBox.py:31-228    -> (scores[N,1,h,w], locs[N,4,h,w])
  DenseBoxLM     DenseBox.py:232-473   -> (scores, locs, landmarks[N,4], refine_scores[N,1])
  DenseBoxLMLOC  DenseBox.py:477-738   -> (score, rf_score, bbox_loc[N,4], lm_heatmap[N,4], lm_loc[N,8])

The modules only hold the fp32 master parameters (ordinary ``nn.Parameter`` s,
so ``.parameters()``, ``.state_dict()``, ``load_state_dict(strict=True)`` of a
reference checkpoint and ``torch.optim.SGD`` all work).  All compute happens in
the HIP engine (``densebox_amd.engine``) through the C ABI of
``libdensebox_hip.so``: there is NO CPU/PyTorch fallback -- ``forward`` on a
non-GPU tensor, or without the built library, raises.
"""
import copy

import torch
import torch.nn as nn

# (attribute stem, index of the conv in vgg19.features) -- DenseBox.py:49-140.
# conv3_3 is constructed and lives in the state_dict but forward() never runs it
# (DenseBox.py:193-195), so it never receives a gradient.
_VGG_LAYOUT = [
    ('conv1_1', 0), ('conv1_2', 2), ('pool1', 4),
    ('conv2_1', 5), ('conv2_2', 7), ('pool2', 9),
    ('conv3_1', 10), ('conv3_2', 12), ('conv3_3', 14), ('conv3_4', 16), ('pool3', 18),
    ('conv4_1', 19), ('conv4_2', 21), ('conv4_3', 23), ('conv4_4', 25),
]

# (head stem, out channels, name of the nn.Sequential wrapper) per network, in
# registration order (DenseBox.py:149-178, :350-396, :595-658).
_HEADS = {
    'DenseBox': [('det', 1, 'output_score'), ('loc', 4, 'output_loc')],
    'DenseBoxLM': [('det', 1, 'output_score'), ('loc', 4, 'output_loc'),
                   ('landmark', 4, 'output_landmark')],
    'DenseBoxLMLOC': [('det', 1, 'output_score'), ('loc', 4, 'output_bbox_loc'),
                      ('lmloc', 8, 'output_lmloc'), ('landmark', 4, 'output_lm_heatmap')],
}

# forward() tuple order, as names of engine outputs
_OUT_ORDER = {
    'DenseBox': ('det', 'loc'),
    'DenseBoxLM': ('det', 'loc', 'landmark', 'refine'),
    'DenseBoxLMLOC': ('det', 'refine', 'loc', 'landmark', 'lmloc'),
}


class _DenseBoxBase(nn.Module):
    KIND = None

    def __init__(self, vgg19):
        super().__init__()
        feats = vgg19.features._modules
        for stem, idx in _VGG_LAYOUT:
            if stem.startswith('pool'):
                setattr(self, stem, copy.deepcopy(feats[str(idx)]))
                continue
            conv = copy.deepcopy(feats[str(idx)])
            act = copy.deepcopy(feats[str(idx + 1)])
            setattr(self, stem + '_1', conv)
            setattr(self, stem + '_2', act)
            setattr(self, stem, nn.Sequential(conv, act))        # second (aliased) registration
        if self.KIND != 'DenseBox':
            self.pool4 = nn.MaxPool2d(kernel_size=2, stride=2, padding=0, dilation=1, ceil_mode=False)
        for stem, k, wrapper in _HEADS[self.KIND]:
            c1 = nn.Conv2d(768, 512, kernel_size=(1, 1))
            c2 = nn.Conv2d(512, k, kernel_size=(1, 1))
            nn.init.xavier_normal_(c1.weight.data)               # weights only; biases keep Conv2d's default
            nn.init.xavier_normal_(c2.weight.data)
            setattr(self, 'conv5_1_' + stem, c1)
            setattr(self, 'conv5_2_' + stem, c2)
            setattr(self, wrapper, nn.Sequential(c1, nn.Dropout(), c2))
        if self.KIND != 'DenseBox':
            self.conv6_1_det = nn.Conv2d(5, 64, kernel_size=(3, 3))    # no padding (DenseBox.py:399-407)
            self.conv6_2_det = nn.Conv2d(64, 64, kernel_size=(5, 5))
            self.conv6_3_det = nn.Conv2d(64, 1, kernel_size=(1, 1))
            for m in (self.conv6_1_det, self.conv6_2_det, self.conv6_3_det):
                nn.init.xavier_normal_(m.weight.data)
        self._engine = None
        # arithmetic type of the HIP path: 'f16' | 'bf16' | 'f32', or None = 'bf16' for training steps (fp32's range: the
        # reference loss is an unscaled sum, a diverging step could overflow f16's 65504 in the gradient maps) and 'f16'
        # for inference (three more mantissa bits: maps within 2.8e-3 of the reference instead of 2.7e-2)
        self.compute_dtype = None
        self.dropout_masks = None         # optional injected {head: uint8 [N,512,h,w]} (parity tests)

    def resolved_dtype(self, train=None):
        if self.compute_dtype is not None:
            return self.compute_dtype
        train = self.training if train is None else train
        return 'bf16' if train else 'f16'

    # ------------------------------------------------------------------ engine plumbing
    def engine(self):
        if self._engine is None:
            from .engine import Engine
            self._engine = Engine(self)
        return self._engine

    def forward(self, X):
        """Reference forward (DenseBox.py:180-228 / :412-473 / :674-738) on the HIP engine.

        Input NCHW fp32 (or fp16/bf16) on a ROCm device; outputs NCHW-contiguous fp32,
        autograd-connected to the parameters so ``loss.backward()`` + ``optimizer.step()``
        work exactly as in the reference training loops (DenseBox.py:2186-2187).
        """
        if not X.is_cuda:
            raise RuntimeError('densebox_amd has no CPU path: forward() needs a tensor on an MI355X '
                               '(got device %s)' % X.device)
        outs = self.engine().forward(X)
        return tuple(outs[k] for k in _OUT_ORDER[self.KIND])

    # additive API (no reference counterpart; semantics = the inline loss section of the train loops)
    def loss(self, outputs, bbox, vertices=None, labels=None, rand_neg_indices=None,
             lm_rand_neg_indices=None, lambda_loc=3.0, lambda_det=1.0, lambda_lm=0.5, **kw):
        from .loss import densebox_loss
        return densebox_loss(self.KIND, outputs, bbox, vertices, labels, rand_neg_indices,
                             lm_rand_neg_indices, lambda_loc, lambda_det, lambda_lm, **kw)

    def detect(self, image, K=10, nms_thresh=0.4):
        """forward -> top-K decode -> NMS (test drivers, DenseBox.py:3788-3799 etc.)."""
        from .decode import detect
        return detect(self, image, K, nms_thresh)

    def detect_batch(self, images, K=10, nms_thresh=0.4, max_batch=32):
        """detect() over a batch tensor or a list of images: one forward + one decode / NMS launch per chunk of <= max_batch
        same-shape images; a list of (dets, keep) in input order (densebox_amd.decode.detect_batch)."""
        from .decode import detect_batch
        return detect_batch(self, images, K, nms_thresh, max_batch)

    def detect_batch_thresh(self, images, score_thresh, max_dets=1024, nms_thresh=0.4, max_batch=32, with_totals=False):
        """detect_batch() with a score threshold in the place of the fixed top-K: every pixel above score_thresh becomes a row (at most
        max_dets <= 4096 per image), NMS over all of them on the device; a list of (dets[n_b, 5|13], keep) in input order
        (densebox_amd.decode.detect_batch_thresh)."""
        from .decode import detect_batch_thresh
        return detect_batch_thresh(self, images, score_thresh, max_dets, nms_thresh, max_batch, with_totals)

    def detect_plates(self, images, K=10, nms_thresh=0.4, max_batch=32, *, region, score_thresh=None, max_dets=1024):
        """detect_batch() on uint8 frames, then every kept detection's plate rectified in one launch: a list of (dets, keep, plates)
        in input order (densebox_amd.decode.detect_plates)."""
        from .decode import detect_plates
        return detect_plates(self, images, K, nms_thresh, max_batch, region=region, score_thresh=score_thresh, max_dets=max_dets)

    def detect_plate_crops(self, images, *, size, K=10, nms_thresh=0.4, max_batch=32):
        """detect_batch() on uint8 frames, then every kept detection's plate rectified to one crop size on the device, in the same
        hipGraph: a list of (dets, keep, crops [len(keep), oh, ow, 3], ok) in input order (densebox_amd.decode.detect_plate_crops)."""
        from .decode import detect_plate_crops
        return detect_plate_crops(self, images, size=size, K=K, nms_thresh=nms_thresh, max_batch=max_batch)

    def evaluate_batch(self, images, gt_boxes, *, evaluator, K=10, score_thresh=None, max_dets=1024, nms_thresh=0.4, max_batch=32,
                       gt_ignore=None, gt_quads=None):
        """forward -> decode + NMS -> match against ground truth -> append to `evaluator` (an evaluate.Evaluator), all on the device
        and, in eval mode, in one hipGraph per chunk; nothing comes back to the host until evaluator.summary()
        (densebox_amd.evaluate.evaluate_batch)."""
        from .evaluate import evaluate_batch
        return evaluate_batch(self, images, gt_boxes, evaluator=evaluator, K=K, score_thresh=score_thresh, max_dets=max_dets,
                              nms_thresh=nms_thresh, max_batch=max_batch, gt_ignore=gt_ignore, gt_quads=gt_quads)

    def track_batch(self, images, *, tracker, stream0=0, K=10, score_thresh=None, max_dets=1024, nms_thresh=0.4, max_batch=32):
        """forward -> decode + NMS -> association with the tracks of camera streams stream0.. in `tracker` (a track.Tracker), all on
        the device and, in eval mode, in one hipGraph per chunk: a list of (dets, keep, track_id, track_hits) in input order
        (densebox_amd.track.track_batch)."""
        from .track import track_batch
        return track_batch(self, images, tracker=tracker, stream0=stream0, K=K, score_thresh=score_thresh, max_dets=max_dets,
                           nms_thresh=nms_thresh, max_batch=max_batch)

    def watch_batch(self, images, *, tracker, zones, stream0=0, K=10, score_thresh=None, max_dets=1024, nms_thresh=0.4, max_batch=32):
        """track_batch() with zones (a zones.Zones made for `tracker`): the keep lists filtered by the streams' include / exclude
        polygons in front of the tracking update, line crossings and region events counted behind it, all on the device and, in eval
        mode, in one hipGraph per chunk: a list of (dets, filtered keep, track_id, track_hits) in input order
        (densebox_amd.zones.watch_batch)."""
        from .zones import watch_batch
        return watch_batch(self, images, tracker=tracker, zones=zones, stream0=stream0, K=K, score_thresh=score_thresh,
                           max_dets=max_dets, nms_thresh=nms_thresh, max_batch=max_batch)

    def track_plate_crops(self, images, *, tracker, gallery, stream0=0, K=10, nms_thresh=0.4, max_batch=32):
        """track_batch() on uint8 frames with the best plate crop of every track kept on the device in `gallery` (a
        gallery.PlateGallery made for `tracker`), in eval mode in one hipGraph per chunk: a list of (dets, keep, track_id, track_hits) in
        input order (densebox_amd.gallery.track_plate_crops)."""
        from .gallery import track_plate_crops
        return track_plate_crops(self, images, tracker=tracker, gallery=gallery, stream0=stream0, K=K, nms_thresh=nms_thresh,
                                 max_batch=max_batch)

    def annotate_batch(self, frames, *, tracker=None, stream0=0, inset=None, K=10, nms_thresh=0.4, max_batch=32, style=None):
        """detect_batch() (track_batch() with a tracker) on uint8 frames, then the boxes, score labels, landmark discs and -- with
        inset=(width, height) -- the rectified plates painted onto the frames on the device, in eval mode in one hipGraph per chunk: a
        list of (dets, keep, track_id or None, annotated [H,W,3]) in input order (densebox_amd.viz.annotate_batch)."""
        from .viz import annotate_batch
        return annotate_batch(self, frames, tracker=tracker, stream0=stream0, inset=inset, K=K, nms_thresh=nms_thresh,
                              max_batch=max_batch, style=style)

    def redact_batch(self, frames, *, tracker=None, stream0=0, K=10, nms_thresh=0.4, max_batch=32, style=None):
        """detect_batch() (track_batch() with a tracker) on uint8 frames, then every kept row's plate and -- with a tracker -- every
        coasting track's predicted box filled, pixelated or blurred on the device (style: a redact.Redaction), in eval mode in one
        hipGraph per chunk: a list of (dets, keep, track_id or None, redacted [H,W,3]) in input order
        (densebox_amd.redact.net_redact_batch)."""
        from .redact import net_redact_batch
        return net_redact_batch(self, frames, tracker=tracker, stream0=stream0, K=K, nms_thresh=nms_thresh, max_batch=max_batch,
                                style=style)

    def detect_batch_resized(self, images, size=720, K=10, nms_thresh=0.4, max_batch=32, score_thresh=None, max_dets=1024):
        """detect_batch() on uint8 frames of any sizes, each padded to a square and resized to size x size in one launch; a list of
        (dets, keep) in input order, coordinates mapped back to the source frames (densebox_amd.decode.detect_batch_resized)."""
        from .decode import detect_batch_resized
        return detect_batch_resized(self, images, size, K, nms_thresh, max_batch, score_thresh, max_dets)

    def detect_batch_nv12(self, frames, width=None, params=None, K=10, nms_thresh=0.4, max_batch=32):
        """detect_batch() on NV12 frames of one size ([h*3/2, pitch] uint8 each, see densebox_amd.color): one conversion launch, then
        detect_batch's tensor path; a list of (dets, keep) in input order (densebox_amd.color.detect_batch_nv12)."""
        from .color import detect_batch_nv12
        return detect_batch_nv12(self, frames, width, params, K, nms_thresh, max_batch)

    def detect_batch_resized_nv12(self, frames, size=720, width=None, params=None, K=10, nms_thresh=0.4, max_batch=32, score_thresh=None,
                                  max_dets=1024):
        """detect_batch_resized() on NV12 frames of any sizes: pad + bicubic resize read the NV12 surfaces in one fused launch; a list
        of (dets, keep) in input order, coordinates mapped back to the source frames (densebox_amd.color.detect_batch_resized_nv12)."""
        from .color import detect_batch_resized_nv12
        return detect_batch_resized_nv12(self, frames, size, width, params, K, nms_thresh, max_batch, score_thresh, max_dets)

    def redact_batch_nv12(self, frames, *, width=None, tracker=None, stream0=0, K=10, nms_thresh=0.4, max_batch=32, style=None, params=None):
        """redact_batch() with NV12 frames in and redacted NV12 frames out, converted on the device on both sides: a list of
        (dets, keep, track_id or None, nv12 [h*3/2, w]) in input order (densebox_amd.color.redact_batch_nv12)."""
        from .color import redact_batch_nv12
        return redact_batch_nv12(self, frames, width=width, tracker=tracker, stream0=stream0, K=K, nms_thresh=nms_thresh,
                                 max_batch=max_batch, style=style, params=params)

    def detect_pyramid(self, images, sizes=(480, 720, 1080), K=10, nms_thresh=0.4, max_batch=32, score_thresh=None, max_dets=1024,
                       with_levels=False):
        """detect_batch_resized() at every size of `sizes` with one resize launch, the rows of all levels merged in source-frame
        coordinates and ONE NMS per frame over their union on the device; a list of (dets[len(sizes) * K, 5|13], keep) in input
        order.  score_thresh: every pixel of every level above it is a row (at most max_dets per level) in the place of the top K
        (densebox_amd.decode.detect_pyramid)."""
        from .decode import detect_pyramid
        return detect_pyramid(self, images, sizes, K, nms_thresh, max_batch, score_thresh, max_dets, with_levels)

    def detect_tiled(self, frames, tile=512, src=None, overlap=128, K=10, score_thresh=None, max_dets=64, nms_thresh=0.4, max_batch=32,
                     rule='core', roi=None, with_tiles=False):
        """Sliced inference for large frames: every frame cut into overlapping src x src windows resized to tile x tile, the tiles of
        all frames forwarded in chunks of one fixed shape, and the rows stitched per frame on the device -- source-frame coordinates,
        only the rows whose tile owns the box centre, ONE NMS per frame; a list of (dets[m_b, 5|13], keep) in input order
        (densebox_amd.tiles.detect_tiled)."""
        from .tiles import detect_tiled
        return detect_tiled(self, frames, tile, src, overlap, K, score_thresh, max_dets, nms_thresh, max_batch, rule, roi, with_tiles)


class DenseBox(_DenseBoxBase):
    KIND = 'DenseBox'


class DenseBoxLM(_DenseBoxBase):
    KIND = 'DenseBoxLM'


class DenseBoxLMLOC(_DenseBoxBase):
    KIND = 'DenseBoxLMLOC'
