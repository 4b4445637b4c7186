"""Best-shot plate crops per track on the GPU: behind the crop launch and the tracking update of a batch of frames ONE launch
(dbx_track_gallery_update) scores the crop of every track matched or born in its frame -- by an exact integer focus measure
(dbx_crop_sharpness: the squared 5-point Laplacian of an integer luma, summed) or by the detection score -- and keeps the better one in
a per-slot gallery on the device.  When a track ends, its best shot moves into an arena at the index of the track's record in
Tracker.finished().  No pixel leaves the device until the finished tracks are asked for.  include/densebox_hip.h has the contract."""
import ctypes as C

import numpy as np
import torch

from . import _lib, decode as DC, rows as R, track as TR
from ._lib import check, ptr, stream_ptr
from .decode import _integer

MAX_PIXELS = 16384           # oh * ow of a crop: its luma plane is staged in LDS as 16-bit values
POLICIES = {'sharpness': 0, 'score': 1}
SHOT = np.dtype([('key', '<f8'), ('score', '<f8'), ('sharpness', '<i8'), ('id', '<i4'), ('frame', '<i4'), ('shots', '<i4'),
                 ('reserved', '<i4')])                                                                                # dbx_shot
SHOT_RECORD = np.dtype([('stream', '<i4'), ('slot', '<i4'), ('shot', SHOT)])                                          # dbx_shot_record
assert SHOT.itemsize == C.sizeof(_lib.Shot) == 40 and SHOT_RECORD.itemsize == C.sizeof(_lib.ShotRecord) == 48


class PlateGallery:
    """The device side of the best shots of `tracker`'s tracks: per track slot of every stream a dbx_shot (40 bytes) and a crop of
    size = (width, height) x channels, plus an arena of `capacity` dbx_shot_record (48 bytes) with their crops for the tracks that
    ended.  Memory: (streams * max_tracks + capacity) * (oh * ow * c + 48) bytes, e.g. 42 MB for 32 streams of 64 tracks, 4096 finished
    tracks and 94 x 24 x 3 crops.  net.track_plate_crops() and gallery.update_batch() advance it together with the tracker; a tracker
    that is advanced without its gallery (track_batch, track.update_batch) loses the shots of the tracks that end meanwhile (they are
    counted in `lost`, and their entries of finished() are not valid).

    policy: 'sharpness' ranks the crops of a track by dbx_crop_sharpness, 'score' by the detection's score; a later crop replaces the
    kept one only when it ranks strictly higher.  min_score: a crop is only considered when its detection scores at least this.  The
    defaults ('sharpness', every detection) are a convention, NOT tuned values: no trained weights exist in this tree to tune them
    with.  The buffers are allocated on the tracker's device at the first use."""

    def __init__(self, tracker, size=(94, 24), policy='sharpness', min_score=-float('inf'), capacity=4096, channels=3):
        from .rectify import _crop_size
        if not isinstance(tracker, TR.Tracker):
            raise RuntimeError('PlateGallery: tracker must be a track.Tracker, got %s' % type(tracker).__name__)
        ow, oh = _crop_size('PlateGallery', size)
        if oh * ow > MAX_PIXELS:
            raise RuntimeError('PlateGallery: size=%r has more than %d pixels' % (size, MAX_PIXELS))
        if policy not in POLICIES:
            raise RuntimeError("PlateGallery: policy must be 'sharpness' or 'score', got %r" % (policy,))
        if not TR._number(min_score):
            raise RuntimeError('PlateGallery: min_score=%r must be a number' % (min_score,))
        if not _integer(capacity) or capacity < 1:
            raise RuntimeError('PlateGallery: capacity=%r must be a positive integer' % (capacity,))
        if not _integer(channels) or channels not in (1, 3):
            raise RuntimeError('PlateGallery: channels=%r must be 1 or 3' % (channels,))
        self.tracker, self.ow, self.oh, self.channels = tracker, ow, oh, int(channels)
        self.policy, self.min_score, self.capacity = policy, float(min_score), int(capacity)
        self._live = self._arena = self._gstate = None

    def params(self):
        return (self.ow, self.oh, self.channels, POLICIES[self.policy], self.min_score, self.capacity)

    @property
    def crop_bytes(self):
        return self.oh * self.ow * self.channels

    def _initial(self):
        n = self.tracker.streams * self.tracker.max_tracks
        live = np.zeros(n * (SHOT.itemsize + self.crop_bytes), np.uint8)
        live[:n * SHOT.itemsize].view(SHOT)['id'] = -1
        arena = np.zeros(self.capacity * SHOT_RECORD.itemsize, np.uint8)
        arena.view(SHOT_RECORD)['shot']['id'] = -1
        return live, arena

    def _buffers(self, dev):
        """(live uint8: dbx_shot [streams][max_tracks], then their crops; arena uint8: dbx_shot_record [capacity], then their crops;
        gstate int64 [4]) on the tracker's device, allocated once.  Only the records of the arena are initialised: a crop is read
        where its record is valid."""
        if self._live is None:
            dev = self.tracker._buffers(dev)[0].device
            live, arena = self._initial()
            self._live = torch.from_numpy(live).to(dev)
            self._arena = torch.empty(self.capacity * (SHOT_RECORD.itemsize + self.crop_bytes), dtype=torch.uint8, device=dev)
            self._arena[:arena.size].copy_(torch.from_numpy(arena))
            self._gstate = torch.zeros(4, dtype=torch.int64, device=dev)
        return self._live, self._arena, self._gstate

    def _key(self, dev):
        """what a captured graph depends on: the buffers' addresses and the parameters"""
        return tuple(t.data_ptr() for t in self._buffers(dev)) + self.params()

    def reset(self):
        """forget every shot and counter, and every track of the tracker as well, so that the indices of the two arenas stay
        aligned; the buffers (and the graphs captured on them) stay"""
        self.tracker.reset()
        if self._live is not None:
            live, arena = self._initial()
            self._live.copy_(torch.from_numpy(live))
            self._arena[:arena.size].copy_(torch.from_numpy(arena))
            self._gstate.zero_()

    def live(self):
        """one copy of the gallery; per stream (shots, crops): the structured array (SHOT) of the slots with id >= 0, in slot order,
        and their crops uint8 [n, oh, ow, c] (all zeros while shots == 0)"""
        S, T = self.tracker.streams, self.tracker.max_tracks
        host = self._initial()[0] if self._live is None else self._live.cpu().numpy()
        shots = host[:S * T * SHOT.itemsize].view(SHOT).reshape(S, T)
        crops = host[S * T * SHOT.itemsize:].reshape(S, T, self.oh, self.ow, self.channels)
        return [(shots[s][shots[s]['id'] >= 0].copy(), crops[s][shots[s]['id'] >= 0].copy()) for s in range(S)]

    def finished(self):
        """(records SHOT_RECORD [m], crops uint8 [m, oh, ow, c], valid bool [m]) with m = min(the tracker's append cursor, capacity):
        entry i is the best shot of the track of tracker.finished()[i] -- the same stream and shot.id == t.id -- where valid[i], which
        is record.shot.id >= 0; an entry is not valid when its track ended while the tracker was advanced without the gallery.  A
        valid entry with shot.shots == 0 never had a crop that counted, and its pixels are zeros.  One copy of the cursor, then of
        exactly the m records and the m crops."""
        empty = (np.zeros(0, SHOT_RECORD), np.zeros((0, self.oh, self.ow, self.channels), np.uint8), np.zeros(0, bool))
        tr = self.tracker
        if tr._state is None or self._arena is None:
            return empty
        o_app = tr._layout()[1]
        m = min(int(tr._state[o_app:o_app + 8].cpu().numpy().view(np.int64)[0]), self.capacity)
        if m <= 0:
            return empty
        rec = self._arena[:m * SHOT_RECORD.itemsize].cpu().numpy().view(SHOT_RECORD)
        o_crops = self.capacity * SHOT_RECORD.itemsize
        valid = rec['shot']['id'] >= 0
        crops = self._arena[o_crops:o_crops + m * self.crop_bytes].cpu().numpy().reshape(m, self.oh, self.ow, self.channels).copy()
        crops[~valid] = 0                                                   # (never written: whatever the allocation held)
        return rec, crops, valid

    def counters(self):
        """(ended, stored, lost, dropped): the tracks whose slot the gallery saw end; of those, the shots that went to the arena, the
        ones whose retired record was not there (the tracker had been advanced without the gallery) and the ones past `capacity`"""
        return (0, 0, 0, 0) if self._gstate is None else tuple(int(v) for v in self._gstate.cpu().numpy())


def _check_gallery(fn, gallery, tracker):
    if not isinstance(gallery, PlateGallery):
        raise RuntimeError('%s: gallery must be a gallery.PlateGallery, got %s' % (fn, type(gallery).__name__))
    if gallery.tracker is not tracker:
        raise RuntimeError('%s: the gallery was made for another tracker' % fn)


def sharpness(crops):
    """dbx_crop_sharpness alone: int64 [n] for uint8 crops [n, oh, ow, c] (c 1 or 3, oh * ow <= 16384), a numpy array (a numpy array
    comes back) or a tensor on the CPU or the GPU (a tensor on its device comes back)."""
    was_np = isinstance(crops, np.ndarray)
    t = torch.from_numpy(np.ascontiguousarray(crops)) if was_np else crops
    if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 4 or t.size(3) not in (1, 3):
        raise RuntimeError('sharpness: crops must be uint8 [n, oh, ow, 1|3], got %s'
                           % (type(crops).__name__ if not torch.is_tensor(t) else '%s %s' % (t.dtype, list(t.shape))))
    n, oh, ow, c = (int(v) for v in t.shape)
    if oh < 1 or ow < 1 or oh * ow > MAX_PIXELS:
        raise RuntimeError('sharpness: a crop of %d x %d pixels is not 1..%d pixels' % (ow, oh, MAX_PIXELS))
    d = DC._on_device(t)
    out = torch.empty(n, dtype=torch.int64, device=d.device)
    if n:
        check(_lib.lib().dbx_crop_sharpness(ptr(d), n, oh, ow, c, ptr(out), stream_ptr()))
    if was_np:
        return out.cpu().numpy()
    return out if t.is_cuda else out.cpu()


def update_batch(images, dets, keeps, *, tracker, gallery, stream0=0):
    """The host results of any detect_* call with landmarks tracked and their best shots kept: track.update_batch with the crops and the
    gallery in between.  Entry j is the next frame of stream stream0 + j.

    images: the frames the rows were detected in -- a uint8 [B,H,W,C] tensor or a list of uint8 [H,W,C] images of any sizes (numpy or
    torch, CPU or GPU), C the gallery's channels; each is uploaded at most once.  dets, keeps: per image the float64 rows [n, 13] and the
    keep list; at most 1024 rows per image.  Rows of 5 columns have no landmarks to rectify and are refused.

    ONE upload of the rows and lists, then dbx_plate_crops_batch with sel = keep, dbx_track_update_batch, dbx_track_gallery_update,
    dbx_track_append and one copy back of the ids.  Returns what track.update_batch returns: per image (track_id int32 [k], track_hits
    int32 [k]) for the k entries of its keep list."""
    from . import rectify
    fn = 'gallery.update_batch'
    p = R.pack_host(fn, dets, keeps, cols=(13,), max_slots=TR.MAX_SLOTS)
    TR._check_streams(fn, tracker, stream0, p.B)
    _check_gallery(fn, gallery, tracker)
    host_ims, _ = rectify.host_images(fn, images, gallery.channels)
    if len(host_ims) != p.B:
        raise RuntimeError('%s: %d images for %d entries of dets' % (fn, len(host_ims), p.B))
    dev_ims = rectify.to_device(images, host_ims)
    dev = tracker._buffers(dev_ims[0].device)[0].device
    dev_ims = [im.to(dev) for im in dev_ims]
    rows = p.upload(dev)                                                               # the one upload of rows and lists
    table = rectify.frame_table(dev_ims)
    crops, ok = rectify._crops_launch(table, p.B, gallery.channels, rows.dets.data_ptr() + 5 * 8, 13, p.slots * 13, rows.keep, p.slots,
                                      gallery.ow, gallery.oh, dev)
    h = TR._launch(tracker, rows, int(stream0), gallery=(gallery, crops, ok))[0].cpu().numpy()      # the one copy back
    return [(h[0, i, :k.size].copy(), h[1, i, :k.size].copy()) for i, k in enumerate(p.lists)]


# ------------------------------------------------------------------------------------------------------------ net.track_plate_crops
def _eager(tr, gal, K, stream0, nms_thresh, dry_outside_capture):
    """The eager function of track_plate_crops' chunks, for the streams from stream0 on: forward, dbx_detect_batch,
    dbx_plate_crops_batch, then the three launches of track._launch.  The frame table is uploaded on the first call for a tensor (a warm-up
    run, outside the capture) and reused for the same address afterwards, as in detect_plate_crops.  Under _graph_replay the warm-up
    runs are dry.  Returns the tensors that go to the host first, then every other tensor the launches wrote or read: a graph entry
    keeps them all."""
    crops_eager = DC._plate_crops_eager(K, gal.ow, gal.oh, nms_thresh)

    def eager(net, images):
        dets, keep, crops, ok, table = crops_eager(net, images)
        dry = dry_outside_capture and not torch.cuda.is_current_stream_capturing()
        ids, slot, retired, tally = TR._launch(tr, R.Rows(dets, keep, None, int(dets.size(0)), K), stream0, dry, (gal, crops, ok))
        return dets, keep, ids, slot, retired, tally, crops, ok, table
    return eager


_HOST = (True, True, True, False, False, False, False, False, False)


def track_plate_crops(net, images, *, tracker, gallery, stream0=0, K=10, nms_thresh=0.4, max_batch=32):
    """Detection, tracking and the best plate crop of every track in one go: image j is the next frame of camera stream stream0 + j.
    Per chunk of at most `max_batch` frames the forward, dbx_detect_batch, dbx_plate_crops_batch (the kept rows' plates rectified to the
    gallery's size), dbx_track_update_batch, dbx_track_gallery_update and dbx_track_append; chunk c starts at stream stream0 + c *
    max_batch.  Neither the tracker's state nor any crop leaves the device; gallery.live(), gallery.finished() and gallery.counters()
    read them.

    images: uint8 frames only -- a [B,H,W,3] tensor or a list of [H,W,3] tensors of ONE shape; those are the pixels that are cropped.
    net: DenseBoxLM or DenseBoxLMLOC (rows with landmarks); the gallery has 3 channels.  Top-K only, K at most 1024: there is no
    score_thresh here, as detect_plate_crops has none (the threshold decode has up to 4096 rows per image and needs another crop
    layout).

    Returns, per image in input order, (dets, keep, track_id, track_hits), exactly what track_batch returns.

    Eval mode replays ONE hipGraph per chunk from the cache detect() uses, under a tag of its own, keyed by (batch shape, dtype, (K, the
    chunk's first stream, the tracker, its buffers and parameters, the gallery's buffers and parameters), nms_thresh, compute dtype).
    The capture's warm-up runs advance a scratch copy of the tracker's state and run the gallery launch with commit = 0, so only
    replays count.  Train mode and DBX_GRAPH=0 run the same launches eagerly."""
    fn = 'track_plate_crops'
    DC._require_landmarks(fn, net)
    if isinstance(images, (list, tuple)) and any(not torch.is_tensor(im) for im in images):
        raise RuntimeError('%s: a list of images must hold uint8 [H,W,3] tensors' % fn)
    DC._one_shape(fn, images, with_dtype=False)
    n = DC._frame_count(fn, images)
    dtypes = {im.dtype for im in images} if isinstance(images, (list, tuple)) else {images.dtype}
    if dtypes != {torch.uint8} and n:
        raise RuntimeError('%s: images must be uint8 [B,H,W,3] frames (the pixels that are cropped), got %s' % (fn, sorted(map(str, dtypes))))
    TR._check_streams(fn, tracker, stream0, n)
    _check_gallery(fn, gallery, tracker)
    if gallery.channels != 3:
        raise RuntimeError('%s: the gallery has %d channels, the frames 3' % (fn, gallery.channels))
    R._check_K(fn, K, TR.MAX_SLOTS)
    dry = DC._use_graph(net)

    def chunk(x, idx):
        first = int(stream0) + idx[0]
        key = ((int(K),) + tracker._key(x.device, first) + gallery._key(x.device), float(nms_thresh))
        res = DC._run_chunk(net, fn, x, key, _eager(tracker, gallery, int(K), first, nms_thresh, dry), _HOST)
        return TR._unpack('topk', res, 13)
    return DC._detect_many(fn, images, max_batch, chunk, with_index=True)
