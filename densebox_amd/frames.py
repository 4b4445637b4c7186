"""The frame pipeline that the painters -- viz.py (dbx_draw_overlay_batch) and redact.py (dbx_redact_batch) -- share: the table of
dbx_overlay_frame records, the ONE upload / ONE launch / one copy back of the host-level calls (Upload), the net-level runner behind
net.annotate_batch and net.redact_batch (run_net) and the eager chain of its chunks (eager_chain).  A painter supplies its style, the
extra sections of its upload, its launch, and what stands between the decode and that launch.  csrc/frame_tile.hpp is the device's
half of the same sharing."""
import ctypes as C

import numpy as np
import torch

from . import _lib, decode as DC, rows as R
from ._lib import ptr
from .decode import _integer, _keep_list

_ALIGN = 64                  # byte alignment of every frame in an arena (the kernels move 16-byte words where src and dst allow)
assert C.sizeof(_lib.OverlayFrame) == 24


def _up(n, a=_ALIGN):
    return (n + a - 1) // a * a


def _p(t):
    """a device tensor, None, or a raw device address given as an int, as a pointer argument"""
    return C.c_void_p(t) if isinstance(t, int) else ptr(t)


# ------------------------------------------------------------------------------------------------------------ style checks
def _color(cls, name, v):
    try:
        t = tuple(v)
    except TypeError:
        t = ()
    if not 1 <= len(t) <= 4 or not all(_integer(e) and 0 <= e <= 255 for e in t):
        raise RuntimeError('%s: %s=%r must hold 1 to 4 integers in 0..255' % (cls, name, v))
    return tuple(int(e) for e in t) + (0,) * (4 - len(t))


def _bounded(cls, name, v, lo, hi):
    if not _integer(v) or not lo <= v <= hi:
        raise RuntimeError('%s: %s=%r must be an integer in %d..%d' % (cls, name, v, lo, hi))
    return int(v)


def _style(fn, style, cls, name):
    """style, or cls's defaults for None; name: cls as the message shows it"""
    if style is None:
        return cls()
    if not isinstance(style, cls):
        raise RuntimeError('%s: style must be a %s, got %s' % (fn, name, type(style).__name__))
    return style


# ------------------------------------------------------------------------------------------------------------ frame tables
def frame_records(srcs, dsts, hw):
    rec = (_lib.OverlayFrame * len(srcs))()
    for r, s, d, (h, w) in zip(rec, srcs, dsts, hw):
        r.src, r.dst, r.h, r.w = s, d, h, w
    return rec


def overlay_table(src, dst):
    """The device table of dbx_overlay_frame records of contiguous uint8 [H,W,C] CUDA tensors src[b] -> dst[b] (one small upload).  It
    holds raw addresses: keep the tensors alive while the table is in use."""
    rec = frame_records([s.data_ptr() for s in src], [d.data_ptr() for d in dst], [(int(s.size(0)), int(s.size(1))) for s in src])
    return torch.frombuffer(rec, dtype=torch.uint8).to(src[0].device)


# ------------------------------------------------------------------------------------------------------------ the one upload
class Upload:
    """The ONE upload of a host-level call and the arena of its results.  The upload holds the packed rows `pk` (rows.pack_host) and
    their keep lists, the caller's sections `before` the frame table, the table, the frames that are on the host (each 64-aligned; a
    CUDA frame stays where it is) and the caller's sections `after` them.  A section is (name, bytes) or (name, bytes, alignment).
    The arena holds every result frame, 64-aligned, always out of place.

    The caller fills view(name) of its sections, send()s, launches on table / addr(name) / the rows send() returned, and takes
    results(): nothing else crosses the bus."""

    def __init__(self, host, kinds, pk, before=(), after=()):
        self.host, self.kinds, self.pk = host, kinds, pk
        B = len(host)
        self.c = int(host[0].size(2))
        self.max_h, self.max_w = max(int(im.size(0)) for im in host), max(int(im.size(1)) for im in host)
        self._at = {}

        def place(at, sections):
            for name, n, *align in sections:
                at = _up(at, *align) if align else at
                self._at[name] = (at, n)
                at += n
            return at
        self._keep = pk.nd
        at = place(pk.nd + pk.nk, before)
        self._tab = at
        at = _up(at + B * 24)
        self._src = []
        for im, kind in zip(host, kinds):
            self._src.append(None if kind == 'cuda' else at)
            if kind != 'cuda':
                at = _up(at + im.numel())
        total = place(at, after)
        self._dst, out_bytes = [], 0
        for im in host:
            self._dst.append(out_bytes)
            out_bytes = _up(out_bytes + im.numel())
        dev = next((im.device for im in host if im.is_cuda), torch.device('cuda'))
        self.up = torch.empty(total, dtype=torch.uint8, device=dev)
        self.arena = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
        self._src_dev = [im.contiguous() if kind == 'cuda' else None for im, kind in zip(host, kinds)]
        self.h = np.zeros(total, np.uint8)
        self.table = self.up.data_ptr() + self._tab

    def view(self, name):
        """the section's bytes in the host image of the upload"""
        at, n = self._at[name]
        return self.h[at:at + n]

    def addr(self, name):
        """the section's device address"""
        return self.up.data_ptr() + self._at[name][0]

    def send(self):
        """writes the rows, the keep lists, the frame table and the host frames, uploads, and returns the rows on the device"""
        h, host = self.h, self.host
        self.pk.write(h, 0, self._keep)
        srcs = [self.up.data_ptr() + o if s is None else s.data_ptr() for o, s in zip(self._src, self._src_dev)]
        rec = frame_records(srcs, [self.arena.data_ptr() + o for o in self._dst], [(int(im.size(0)), int(im.size(1))) for im in host])
        h[self._tab:self._tab + len(host) * 24] = np.frombuffer(rec, np.uint8)
        for im, o in zip(host, self._src):
            if o is not None:
                h[o:o + im.numel()] = im.contiguous().numpy().reshape(-1)
        self.up.copy_(torch.from_numpy(h))
        return self.pk.on(self.up, 0, self._keep)

    def results(self):
        """the result frames in input order, each of the kind of its input: one copy back when a frame came from the host"""
        arena = self.arena
        down = arena.cpu() if any(k != 'cuda' for k in self.kinds) else None       # (behind the launch on the stream: `up` and the frames are done with)
        out = []
        for im, kind, o in zip(self.host, self.kinds, self._dst):
            v = (arena if kind == 'cuda' else down)[o:o + im.numel()].view(im.shape)
            out.append(v.numpy() if kind == 'numpy' else v)
        return out


# ------------------------------------------------------------------------------------------------------------ the net-level calls
def eager_chain(K, tr, first, nms_thresh, dry_outside_capture, paint, between=None):
    """The eager function of a net-level call's chunks: forward, dbx_detect_batch, what between(images, rows, memo, rest) launches,
    the two tracking launches (tracker given), then the painter's own launch, paint(table, rows, H, W, first, ids, dry, extra) with what
    `between` returned.  The frame table and the output frames are made on the first call for an input tensor (the warm-up, outside
    the capture) and reused for the same address afterwards; `memo` is that input's dict for whatever else `between` has to make
    once, and `rest` the list it appends its tensors to.  Returns (dets, keep[, ids], painted), then every other tensor the launches
    read or wrote: a graph entry keeps them all."""
    from . import track as T
    made = {}

    def eager(net, images):
        s, l, hm, ll = DC._forward_maps(net, images)
        B, H, W = int(images.size(0)), int(images.size(1)), int(images.size(2))
        dets, _, keep = DC._run_batch(s, l, K, lm_heat=hm, lm_loc=ll, nms_thresh=nms_thresh)
        rows = R.Rows(dets, keep, None, B, K)
        key = (images.data_ptr(), tuple(images.shape))
        if key not in made:
            out = torch.empty_like(images)
            made[key] = (out, overlay_table(list(images.unbind(0)), list(out.unbind(0))), {})
        out, table, memo = made[key]
        res, rest = [dets, keep], [table]
        extra = between(images, rows, memo, rest) if between else None
        ids, dry = None, False
        if tr is not None:
            dry = dry_outside_capture and not torch.cuda.is_current_stream_capturing()
            ids, slot, retired, tally = T._launch(tr, rows, first, dry)
            res.append(ids)
            rest += [slot, retired, tally]
        paint(table, rows, H, W, first, ids, dry, extra)
        return tuple(res + [out] + rest)
    return eager


def run_net(fn, tag, net, frames, *, tracker, stream0, K, nms_thresh, max_batch, max_slots, key_parts, n_rest, paint, between=None):
    """Detection, optionally tracking, and the painted frames of net.annotate_batch / net.redact_batch: the argument checks, then per
    chunk of at most max_batch frames one graph entry (or eager run) under `tag`, keyed by ('topk', K) + key_parts + (frames to the
    host,) and, with a tracker, its key for the chunk's first stream.  The chunk's eager function is eager_chain's over paint and
    between, which returns n_rest tensors beyond the results and the tracker's three.  Returns, per frame in input order, (dets,
    keep, track_id or None, painted) with painted of the kind of the frame."""
    from . import rectify, track as T
    host, kinds = rectify.host_images(fn, frames, 3)
    if len({tuple(im.shape) for im in host}) > 1:
        raise RuntimeError('%s: the frames of a list must have one shape (stream j is image j), got %s'
                           % (fn, sorted({str(tuple(im.shape)) for im in host})))
    if tracker is not None:
        T._check_streams(fn, tracker, stream0, len(host))
    R._check_K(fn, K, max_slots)
    if not _integer(max_batch) or max_batch < 1:
        raise RuntimeError('%s: max_batch=%r must be a positive integer' % (fn, max_batch))
    K = int(K)
    to_host = any(k != 'cuda' for k in kinds)
    x = DC._on_device(frames) if torch.is_tensor(frames) else rectify.to_device(frames, host)
    dry = DC._use_graph(net)

    def chunk(x, idx):
        first = int(stream0) + idx[0]
        key = ('topk', K) + key_parts + (to_host,)
        if tracker is not None:
            key += tracker._key(x.device, first)
        n_res = 4 if tracker is not None else 3
        flags = (True,) * (n_res - 1) + (to_host,) + (False,) * (n_rest + (3 if tracker is not None else 0))
        eager = eager_chain(K, tracker, first, nms_thresh, dry, paint, between)
        res = DC._run_chunk(net, tag, x, (key, float(nms_thresh)), eager, flags)
        d, k = res[0].numpy(), res[1].numpy()
        ids = res[2].numpy() if tracker is not None else None
        # the results own their memory (a graph entry's buffers are overwritten by its next replay): the chunk's frames by ONE clone,
        # device to device for CUDA frames
        painted = res[n_res - 1].clone()
        out = []
        for b in range(d.shape[0]):
            keep = _keep_list(k[b])
            out.append((d[b].copy(), keep, None if ids is None else ids[0, b, :len(keep)].copy(), painted[b]))
        return out
    out = []
    for (d, keep, tid, painted), kind in zip(DC._detect_many(fn, x, max_batch, chunk, with_index=True), kinds):
        if kind == 'cuda' and not painted.is_cuda:
            painted = painted.cuda()                                 # (a CUDA frame in a list that also holds host frames)
        out.append((d, keep, tid, painted.numpy() if kind == 'numpy' else painted))
    return out
