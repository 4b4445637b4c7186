"""Tiled detection for large frames: every frame is cut into overlapping fixed-size windows ("tiles", optionally magnified), the tiles
of all frames run through ONE fixed-shape batched forward, and the rows are stitched back per frame on the device
(dbx_tile_rows_batch per forward chunk, dbx_tile_nms_batch once per call; csrc/tile_ops.hip).

A tile OWNS the part of the frame nearer to its centre than to its neighbours' -- its core, bounded by the midpoints of the overlaps --
and a row survives the stitch only in the tile whose core holds the centre of its box: a plate cut by a tile border gives a second,
truncated box in the neighbour that IoU-NMS would not remove, and the ownership rule drops it.  With an overlap at least as wide as
the widest object, the object is whole inside the tile that owns its centre."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from . import decode as DC
from ._lib import check, ptr, stream_ptr
from .decode import _integer

TILE_DTYPE = np.dtype([('frame', '<i4'), ('x0', '<i4'), ('y0', '<i4'), ('side', '<i4'), ('cw', '<i4'), ('ch', '<i4'), ('scale', '<f8'),
                       ('lo2x', '<f8'), ('hi2x', '<f8'), ('lo2y', '<f8'), ('hi2y', '<f8')])
assert TILE_DTYPE.itemsize == C.sizeof(_lib.Tile) == 64
RULES = {'none': _lib.TILE_RULE_NONE, 'core': _lib.TILE_RULE_CORE}
MAX_ROWS = 4096                  # dbx_tile_nms_batch's bound on the tiles of a frame x rows per tile


def _table_ptr(table):
    return C.c_void_p(table.ctypes.data)


def _check_grid(fn, src, overlap):
    if not _integer(src) or src < 1:
        raise RuntimeError('%s: src=%r must be a positive integer (the window side in source pixels)' % (fn, src))
    if not _integer(overlap) or overlap < 0 or 2 * overlap > src:
        raise RuntimeError('%s: overlap=%r must be an integer in 0..src / 2 = %d' % (fn, overlap, src // 2))


def _check_roi(fn, roi, b=None):
    """the integer rectangles (x0, y0, x1, y1) of one frame, x1 > x0 and y1 > y0"""
    where = '' if b is None else ' of frame %d' % b
    if not isinstance(roi, (list, tuple)):
        raise RuntimeError('%s: roi%s must be a list of rectangles (x0, y0, x1, y1), got %r' % (fn, where, roi))
    out = []
    for r in roi:
        ok = isinstance(r, (list, tuple, np.ndarray)) and len(r) == 4 and all(_integer(v) for v in r)
        if not ok or r[2] <= r[0] or r[3] <= r[1]:
            raise RuntimeError('%s: a rectangle%s must be 4 integers (x0, y0, x1, y1) with x1 > x0 and y1 > y0, got %r' % (fn, where, r))
        out.append(tuple(int(v) for v in r))
    return out


def plan(h, w, src, overlap, roi=None, fn='tiles.plan'):
    """The tiles of one h x w frame for window side `src` and `overlap` (source pixels) as a NumPy record array of TILE_DTYPE (the
    layout of dbx_tile), row-major (dbx_tile_grid): along an axis of length L one padded window at 0 when L <= src, otherwise
    ceil((L - src) / (src - overlap)) + 1 windows at min(i * (src - overlap), L - src).  frame is 0 and scale 1; a caller that resizes
    the windows sets scale = src / tile.

    roi: a list of integer rectangles (x0, y0, x1, y1), exclusive at x1 / y1; only the tiles whose core -- the part of the plane they
    own -- meets one of them are returned.  Cores always come from the full grid, so pruning never changes who owns a point."""
    if not (_integer(h) and _integer(w)) or h < 1 or w < 1:
        raise RuntimeError('%s: frame size %r x %r must be positive integers' % (fn, h, w))
    _check_grid(fn, src, overlap)
    L = _lib.lib()
    n = L.dbx_tile_grid(int(h), int(w), int(src), int(overlap), None, 0)
    if n < 0:
        check(n)
    table = np.zeros(n, TILE_DTYPE)
    got = L.dbx_tile_grid(int(h), int(w), int(src), int(overlap), _table_ptr(table), n)
    if got != n:
        check(got if got < 0 else -1)
    if roi is None:
        return table
    rects = _check_roi(fn, roi)
    hit = np.zeros(n, bool)
    for x0, y0, x1, y1 in rects:
        # the core holds the points p with lo2 <= 2 p < hi2; the rectangle the points x0 <= p < x1
        hit |= (2 * x0 < table['hi2x']) & (2 * x1 > table['lo2x']) & (2 * y0 < table['hi2y']) & (2 * y1 > table['lo2y'])
    return table[hit]


def call_table(fn, sizes, tile, src, overlap, roi=None):
    """The table of a call over frames of sizes[b] = (h, w): every frame's plan with frame = b and scale = src / tile, back to back.
    roi: None or one list of rectangles per frame (None for a frame: all its tiles).  A frame may end up with no tile."""
    if roi is not None and (not isinstance(roi, (list, tuple)) or len(roi) != len(sizes)):
        raise RuntimeError('%s: roi must be None or one list of rectangles per frame (%d frames)' % (fn, len(sizes)))
    parts = []
    for b, (h, w) in enumerate(sizes):
        r = None if roi is None or roi[b] is None else _check_roi(fn, roi[b], b)
        p = plan(h, w, src, overlap, r, fn)
        p['frame'] = b
        p['scale'] = int(src) / int(tile)
        parts.append(p)
    return np.concatenate(parts)


def _check_rows(fn, table, frames, rpt):
    per_frame = np.bincount(table['frame'], minlength=frames)
    if table.shape[0] == 0:
        raise RuntimeError('%s: no tile to run (the regions of interest meet no frame)' % fn)
    if int(per_frame.max()) * rpt > MAX_ROWS:
        b = int(per_frame.argmax())
        raise RuntimeError('%s: frame %d has %d tiles x %d rows per tile = %d rows, more than the %d the NMS takes; use fewer rows per '
                           'tile, a larger src or a smaller overlap' % (fn, b, per_frame[b], rpt, per_frame[b] * rpt, MAX_ROWS))
    return per_frame


class _Stitch(object):
    """The device side of one call's stitch: the table (host + device copy), the staging area, and the two entry points."""

    def __init__(self, fn, table, tdev, frames, rpt, dc, rule, dev):
        self.fn, self.table, self.tdev, self.B, self.rpt, self.dc, self.rule, self.dev = fn, table, tdev, frames, rpt, dc, rule, dev
        self.n = int(table.shape[0])
        self.L = _lib.lib()
        nbytes = self.L.dbx_tile_stage_bytes(self.n, rpt, dc)
        if nbytes < 0:
            raise RuntimeError('%s: %d tiles x %d rows per tile are out of range' % (fn, self.n, rpt))
        self.stage = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def rows(self, dets, counts, t0, n):
        """ONE dbx_tile_rows_batch launch: dets [n, rpt, dc] float64 / counts [n, 2] int32 or None (device) of tiles t0 .. t0 + n"""
        check(self.L.dbx_tile_rows_batch(ptr(dets), ptr(counts), _table_ptr(self.table), ptr(self.tdev), self.n, t0, n, self.rpt, self.dc,
                                         self.rule, ptr(self.stage), stream_ptr()))

    def nms(self, nms_thresh):
        """dbx_tile_nms_batch: (arena uint8 -- packed rows, the keep lists right behind them --, tile index int32, counts int32), device"""
        n, B, rpt, dc = self.n, self.B, self.rpt, self.dc
        max_tiles = int(np.bincount(self.table['frame'], minlength=B).max())
        ws = torch.empty(self.L.dbx_tile_nms_batch_workspace_bytes(B, max_tiles, rpt), dtype=torch.uint8, device=self.dev)
        arena = torch.empty(n * rpt * (dc * 8 + 4) + B * 4, dtype=torch.uint8, device=self.dev)
        tile_of = torch.empty(n * rpt, dtype=torch.int32, device=self.dev)
        counts = torch.empty(2 * n + B + 1, dtype=torch.int32, device=self.dev)
        check(self.L.dbx_tile_nms_batch(_table_ptr(self.table), ptr(self.tdev), n, B, rpt, dc, float(nms_thresh), ptr(self.stage), ptr(arena),
                                        ptr(arena), ptr(tile_of), ptr(counts), ptr(ws), stream_ptr()))
        return arena, tile_of, counts

    def fetch(self, net, nms_thresh, with_tiles):
        """The NMS, then the counts to the host (the first wait), then exactly the rows, lists and tile indices they announce (the
        second).  Per frame (dets float64 [m_b, dc], keep list[, tile index per row within the frame's plan, the frame's plan])."""
        arena, tile_of, counts = self.nms(nms_thresh)
        n, B, dc = self.n, self.B, self.dc
        counts = counts.cpu().numpy()
        prefix = counts[2 * n:]
        total = int(prefix[-1])
        nbytes = total * (dc * 8 + 4) + B * 4
        if net is None:
            host = arena[:nbytes].cpu().numpy()
        else:
            pin = DC._pinned(net, nbytes)
            pin[:nbytes].copy_(arena[:nbytes], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            host = pin[:nbytes].numpy().copy()
        out = DC._unpack_packed(prefix, host, None, dc)
        if not with_tiles:
            return out
        t_host = tile_of[:total].cpu().numpy()
        first = np.concatenate([[0], np.cumsum(np.bincount(self.table['frame'], minlength=B))])
        return [r + ((t_host[int(prefix[b]):int(prefix[b + 1])] - first[b]).astype(np.int64), self.table[first[b]:first[b + 1]].copy())
                for b, r in enumerate(out)]


def _check_front(fn, tile, src, overlap, K, max_batch, rule):
    if not _integer(tile) or tile < 4 or tile % 4:
        raise RuntimeError('%s: tile=%r must be a positive multiple of 4 (the maps are tile / 4)' % (fn, tile))
    src = tile if src is None else src
    _check_grid(fn, src, overlap)
    if not _integer(max_batch) or max_batch < 1:
        raise RuntimeError('%s: max_batch=%r must be a positive integer' % (fn, max_batch))
    if not _integer(K) or not 1 <= K <= MAX_ROWS:
        raise RuntimeError('%s: K=%r must be an integer in 1..%d' % (fn, K, MAX_ROWS))
    if rule not in RULES:
        raise RuntimeError("%s: rule=%r must be 'core' or 'none'" % (fn, rule))
    return int(tile), int(src), int(overlap), int(K), int(max_batch), RULES[rule]


def cut(dev, table, tile):
    """ONE dbx_resize_cubic_batch_u8 launch that cuts every tile of `table` out of the device frames dev[b] (uint8 [H,W,3]): window
    (x0, y0, cw, ch) padded on the right / bottom with 128 to side x side and resized to tile x tile; uint8 [n, tile, tile, 3]."""
    from . import resize
    spec = [(int(t['frame']), int(t['x0']), int(t['y0']), int(t['cw']), int(t['ch']), 0, 0, int(t['side'] - t['cw']), int(t['side'] - t['ch']),
             tile, tile) for t in table]
    return resize._resize_jobs(dev, spec, int(dev[0].size(2)))


def detect_tiled(net, frames, tile=512, src=None, overlap=128, K=10, score_thresh=None, max_dets=64, nms_thresh=0.4, max_batch=32,
                 rule='core', roi=None, with_tiles=False):
    """Sliced inference: every frame is cut into overlapping src x src windows (dbx_tile_grid), each resized to tile x tile, the tiles
    of ALL frames are forwarded in plan order in chunks of `max_batch` -- one graph shape plus a tail, whatever the frame sizes -- and
    the rows are stitched per frame on the device: rows in source-frame coordinates, only those whose tile owns the box centre, ONE
    greedy NMS per frame over them.

    frames: a uint8 [B,H,W,3] tensor or a list of [H,W,3] images (numpy arrays or tensors, on the CPU or the GPU) of any sizes; each is
    uploaded at most once.  tile: the network input side, a multiple of 4.  src: the window side in source pixels (default: tile;
    src < tile magnifies).  overlap: in source pixels, at most src / 2; the default 128 covers the 120-pixel widest trained plate, a
    convention and NOT a tuned value (no trained weights exist in this tree).  K: rows per tile of the top-K decode; score_thresh: a
    number runs the threshold decode in its place with at most max_dets rows per tile (a non-default K together with a threshold
    raises).  The tiles of a frame times the rows per tile may not exceed 4096.  rule: 'core' (above) or 'none' (every row is owned).
    roi: per frame a list of integer rectangles (x0, y0, x1, y1), or None; a tile runs only if its core meets one of them.

    The launches: ONE dbx_resize_cubic_batch_u8 cuts every tile of the call; per chunk the forward + dbx_detect_batch (or
    dbx_thresh_rows_batch) -- in eval mode the cached hipGraph detect_pyramid's levels replay -- and one dbx_tile_rows_batch; then one
    dbx_tile_nms_batch.  The host waits twice: for the counts, then for exactly the rows and lists they announce.  Train mode and
    DBX_GRAPH=0 run the same launches eagerly.

    Returns, per frame in input order, (dets float64 [m_b, 5|13] in source-frame coordinates, keep list); m_b may be 0.
    with_tiles=True adds the tile of every row (an index into the frame's plan) and the frame's plan (tiles.TILE_DTYPE records of the
    tiles that ran)."""
    from . import rectify
    fn = 'detect_tiled'
    tile, src, overlap, K, max_batch, rule_id = _check_front(fn, tile, src, overlap, K, max_batch, rule)
    tc = DC._thresh_or_topk(fn, K, score_thresh, max_dets)
    if np.isnan(float(nms_thresh)) or float(nms_thresh) < 0:
        raise RuntimeError('%s: nms_thresh=%r must be a number >= 0' % (fn, nms_thresh))
    host, _ = rectify.host_images(fn, frames, 3)
    B, dc = len(host), DC._det_cols(net)
    rpt = K if tc is None else tc[1]
    table = call_table(fn, [(int(im.size(0)), int(im.size(1))) for im in host], tile, src, overlap, roi)
    _check_rows(fn, table, B, rpt)
    dev = rectify.to_device(frames, host)
    x = cut(dev, table, tile)
    tdev = torch.from_numpy(table.view(np.uint8).copy()).to(x.device)
    st = _Stitch(fn, table, tdev, B, rpt, dc, rule_id, x.device)
    if tc is None:
        eager, tag, key = DC._detect_batch_eager(K, nms_thresh), 'level', (K, float(nms_thresh))
    else:
        eager, tag, key = DC._thresh_rows_eager(tc[0], tc[1]), 'level_thresh', ((tc[1], tc[0]), float(nms_thresh))
    for c0 in range(0, st.n, max_batch):
        c1 = min(st.n, c0 + max_batch)
        # (a graph entry's device rows and counts: overwritten by its next replay, queued behind this chunk's launch)
        d, second = DC._run_chunk(net, tag, x[c0:c1], key, eager, (False, False))
        st.rows(d, None if tc is None else second, c0, c1 - c0)
    return st.fetch(net, nms_thresh, bool(with_tiles))


def merge_host_results(results, table, frames, rule='core', nms_thresh=0.4, with_tiles=False):
    """The stitch alone, for per-tile HOST results of any detect_* call: results[t] the float64 rows [n_t, 5|13] of tile t of `table`
    in TILE coordinates (or a (dets, keep) pair, of which the rows are taken; n_t may differ and be 0), table the call's TILE_DTYPE
    records (tiles.call_table), frames the number of frames.  One upload (table, counts and rows), then dbx_tile_rows_batch over all
    tiles and dbx_tile_nms_batch.  Returns what detect_tiled returns."""
    fn = 'tiles.merge_host_results'
    if rule not in RULES:
        raise RuntimeError("%s: rule=%r must be 'core' or 'none'" % (fn, rule))
    if not isinstance(table, np.ndarray) or table.dtype != TILE_DTYPE or table.ndim != 1 or table.shape[0] < 1:
        raise RuntimeError('%s: table must be a non-empty 1-d array of tiles.TILE_DTYPE records' % fn)
    if not isinstance(results, (list, tuple)) or len(results) != table.shape[0]:
        raise RuntimeError('%s: results must be a list with one entry per tile (%d tiles)' % (fn, table.shape[0]))
    if not _integer(frames) or frames < 1:
        raise RuntimeError('%s: frames=%r must be a positive integer' % (fn, frames))
    rows = [np.asarray(DC._host(r[0] if isinstance(r, tuple) else r), np.float64) for r in results]
    dcs = {r.shape[1] for r in rows if r.ndim == 2}
    if any(r.ndim != 2 for r in rows) or len(dcs) != 1 or not dcs <= {5, 13}:
        raise RuntimeError('%s: every result must be rows [n, 5] or [n, 13], all alike; got %s' % (fn, [list(r.shape) for r in rows]))
    dc, n = dcs.pop(), len(rows)
    rpt = max(1, max(r.shape[0] for r in rows))
    if rpt > MAX_ROWS:
        raise RuntimeError('%s: %d rows in one tile exceed %d' % (fn, rpt, MAX_ROWS))
    table = np.ascontiguousarray(table)
    _check_rows(fn, table, int(frames), rpt)
    nt, nc = n * 64, n * 8
    host = np.zeros(nt + nc + n * rpt * dc * 8, np.uint8)
    host[:nt] = table.view(np.uint8)
    cnt = host[nt:nt + nc].view(np.int32).reshape(n, 2)
    slot = host[nt + nc:].view(np.float64).reshape(n, rpt, dc)
    for t, r in enumerate(rows):
        cnt[t] = r.shape[0]
        slot[t, :r.shape[0]] = r
    buf = torch.from_numpy(host).cuda()
    st = _Stitch(fn, table, buf[:nt], int(frames), rpt, dc, RULES[rule], buf.device)
    st.rows(buf[nt + nc:].view(torch.float64), buf[nt:nt + nc].view(torch.int32), 0, n)
    return st.fetch(None, nms_thresh, bool(with_tiles))
