"""Rows behind the decodes: the one description of a batch of decoded rows that dbx_match_gt_batch, dbx_eval_append,
dbx_track_update_batch and dbx_draw_overlay_batch take (csrc/det_frame.hpp has the reading rule) -- on the device as the decodes leave
it (Rows, decode_rows), and packed from the host results of any detect_* call (pack_host)."""
import collections

import numpy as np
import torch

from . import decode as DC
from ._lib import ptr
from .decode import _host, _integer


def _check_K(fn, K, limit):
    if not _integer(K) or not 1 <= K <= limit:
        raise RuntimeError('%s: K=%r must be an integer in 1..%d' % (fn, K, limit))


class Rows(collections.namedtuple('Rows', 'dets keep prefix B slots')):
    """Device tensors: dets float64 [..., 5|13], keep int32 and, for the packed layout of dbx_detect_thresh_batch, prefix int32 [B + 1]
    (None: the slot layout of dbx_detect_batch, frame b's rows at b * slots and its list at b * (slots + 1))."""
    __slots__ = ()

    @property
    def dc(self):
        return int(self.dets.size(-1))

    @property
    def det_rows(self):
        return self.dets.numel() // self.dc

    def args(self, batch=True):
        """(dets, det_cols, det_rows, keep, prefix, batch, slots) as the entry points take them; dbx_draw_overlay_batch has its batch
        elsewhere"""
        return (ptr(self.dets), self.dc, self.det_rows, ptr(self.keep), ptr(self.prefix)) + ((self.B,) if batch else ()) + (self.slots,)


def decode_rows(score, loc, lm_heat, lm_loc, B, K, thresh, nms_thresh):
    """The decode (+ NMS) of B frames' maps where the launches behind it read it: dbx_detect_batch of K rows when thresh is None, else
    dbx_detect_thresh_batch with thresh = (score_thresh, max_dets).  Returns (Rows, the other tensors a caller copies: () or (counts,))."""
    if thresh is None:
        dets, _, keep = DC._run_batch(score, loc, K, lm_heat=lm_heat, lm_loc=lm_loc, nms_thresh=nms_thresh)
        return Rows(dets, keep, None, B, K), ()
    dets, keep, counts = DC._run_thresh_batch(score, loc, thresh[0], thresh[1], lm_heat, lm_loc, nms_thresh, lists_behind_rows=False)
    return Rows(dets, keep, counts[2 * B:], B, thresh[1]), (counts,)


class HostRows(collections.namedtuple('HostRows', 'rows lists dc B slots')):
    """pack_host's result: per image the float64 rows [n, dc] and the int64 keep list, and the slot layout that holds them all"""
    __slots__ = ()

    @property
    def nd(self):
        """bytes of the float64 [B, slots, dc] image"""
        return self.B * self.slots * self.dc * 8

    @property
    def nk(self):
        """bytes of the int32 [B, slots + 1] image"""
        return self.B * (self.slots + 1) * 4

    def write(self, host, o_dets, o_keep):
        """the two images into the uint8 array `host` at byte offsets o_dets (a multiple of 8) and o_keep (of 4): every image's rows,
        then zeros; its count, its entries, then zeros"""
        hd = host[o_dets:o_dets + self.nd].view(np.float64).reshape(self.B, self.slots, self.dc)
        hk = host[o_keep:o_keep + self.nk].view(np.int32).reshape(self.B, self.slots + 1)
        for i, (r, k) in enumerate(zip(self.rows, self.lists)):
            hd[i, :r.shape[0]], hd[i, r.shape[0]:] = r, 0.0
            hk[i, 0], hk[i, 1:1 + k.size], hk[i, 1 + k.size:] = k.size, k, 0

    def on(self, buf, o_dets, o_keep):
        """the Rows of the two images where write() put them, in the uint8 device tensor `buf` the array was uploaded to"""
        return Rows(buf[o_dets:o_dets + self.nd].view(torch.float64).view(self.B, self.slots, self.dc),
                    buf[o_keep:o_keep + self.nk].view(torch.int32), None, self.B, self.slots)

    def upload(self, dev):
        """the two images back to back in ONE upload: the Rows on `dev`"""
        host = np.empty(self.nd + self.nk, np.uint8)
        self.write(host, 0, self.nd)
        return self.on(torch.from_numpy(host).to(dev), 0, self.nd)


def pack_host(fn, dets, keeps, cols=(5, 13), max_slots=4096, n=None):
    """The host results of any detect_* call checked for caller `fn`: per image the rows [m, c] with c in `cols` (numpy arrays or
    tensors) and the keep list (a sequence or a tensor); an image may have no rows and an empty list.  n: the number of images the
    lists must match (None: any, but one at least).  slots is the longest of the images' rows and lists, 1 at least and max_slots at
    most.  Returns the HostRows, or raises RuntimeError."""
    lists_ok = isinstance(dets, (list, tuple)) and isinstance(keeps, (list, tuple))
    if n is None and (not lists_ok or len(dets) != len(keeps) or not dets):
        raise RuntimeError('%s: dets and keeps must be non-empty lists with one entry per image' % fn)
    if n is not None and (not lists_ok or len(dets) != n or len(keeps) != n):
        raise RuntimeError('%s: dets and keeps must be lists with one entry per image (%d images)' % (fn, n))
    rows = [_host(d).astype(np.float64) for d in dets]
    dcs = {r.shape[1] for r in rows if r.ndim == 2}
    if any(r.ndim != 2 for r in rows) or len(dcs) != 1 or not dcs <= set(cols):
        what = '[n, 13] (rows with landmarks)' if tuple(cols) == (13,) else '[n, 5] or [n, 13], all alike'
        raise RuntimeError('%s: every dets entry must be %s; got %s' % (fn, what, [list(r.shape) for r in rows]))
    lists = [np.asarray(_host(k), np.int64).reshape(-1) for k in keeps]
    for i, (r, k) in enumerate(zip(rows, lists)):
        if k.size and (k.min() < 0 or k.max() >= r.shape[0]):
            raise RuntimeError('%s: keeps[%d] names a row outside 0..%d' % (fn, i, r.shape[0] - 1))
    slots = max(1, max(max(r.shape[0], k.size) for r, k in zip(rows, lists)))
    if slots > max_slots:
        raise RuntimeError('%s: %d rows in one image exceed %d' % (fn, slots, max_slots))
    return HostRows(rows, lists, dcs.pop(), len(rows), slots)
