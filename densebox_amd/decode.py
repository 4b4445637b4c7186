"""Inference tail on the GPU: top-K decode (parse_output / parse_out_MN / parse_DetLM / parse_DetLMLOC,
DenseBox.py:3114-3395) and greedy NMS (DenseBox.py:3398-3443), same names, arguments and results
(float64 ``np.ndarray`` rows in descending-score order, python list of kept row indices)."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr


def _integer(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _keep_list(k):
    """the python list of kept rows in a keep buffer [count, idx...] on the host"""
    return [int(v) for v in k[1:1 + int(k[0])]]


def _det_cols(net):
    return 5 if net.KIND == 'DenseBox' else 13


def _require_landmarks(fn, net, to='rectify'):
    if net.KIND == 'DenseBox':
        raise RuntimeError('%s: DenseBox rows have no landmarks to %s; use DenseBoxLM or DenseBoxLMLOC' % (fn, to))


def _decode_inputs(score, loc, lm_heat, lm_loc, batch=None):
    """The prologue of every decode launcher: shape checks of the [B,C,rows,cols] maps (B == batch where one is given), the device (the
    score map's, or the current CUDA device for host maps) and the fp32-contiguous maps on it.  Returns (score, loc, lm_heat, lm_loc, B,
    rows, cols, row columns 5|13, device)."""
    B, _, rows, cols = score.shape
    assert (batch is None or B == batch) and score.size(1) == 1 and loc.size() == torch.Size([B, 4, rows, cols])
    if lm_heat is not None:
        assert lm_heat.size() == torch.Size([B, 4, rows, cols])
    if lm_loc is not None:
        assert lm_loc.size() == torch.Size([B, 8, rows, cols])
    dev = score.device if score.is_cuda else torch.device('cuda')

    def f(t):
        return None if t is None else t.detach().to(dev, torch.float32).contiguous()
    return f(score), f(loc), f(lm_heat), f(lm_loc), B, rows, cols, 5 if (lm_heat is None and lm_loc is None) else 13, dev


def _run(score_map, loc_map, M, N, K, lm_heat=None, lm_loc=None, nms_thresh=0.4):
    s, l, hm, ll, _, rows, cols, dc, dev = _decode_inputs(score_map, loc_map, lm_heat, lm_loc, batch=1)
    assert (rows, cols) == (M // 4, N // 4)
    dets = torch.empty((K, dc), dtype=torch.float64, device=dev)
    topk = torch.empty(K, dtype=torch.int64, device=dev)
    keep = torch.empty(K + 1, dtype=torch.int32, device=dev)
    L = _lib.lib()
    scratch = torch.empty(L.dbx_detect_scratch_bytes(rows, cols, K), dtype=torch.uint8, device=dev)
    check(L.dbx_detect(ptr(s), ptr(l), ptr(hm), ptr(ll), rows, cols, K, float(nms_thresh), ptr(dets), dc, ptr(topk),
                       ptr(keep), ptr(scratch), stream_ptr()))
    return dets, topk, keep


def parse_out_MN(score_map, loc_map, M, N, K=10):
    return _run(score_map, loc_map, M, N, K)[0].cpu().numpy()


def parse_output(score_map, loc_map, K=10):
    assert score_map.size() == torch.Size([1, 1, 60, 60])
    return parse_out_MN(score_map, loc_map, 240, 240, K)


def parse_DetLM(score_map, loc_map, lm_map, M, N, K=10):
    return _run(score_map, loc_map, M, N, K, lm_heat=lm_map)[0].cpu().numpy()


def parse_DetLMLOC(score_map, bbox_loc_map, lm_heat_map, lm_loc_map, M, N, K=10):
    return _run(score_map, bbox_loc_map, M, N, K, lm_heat=lm_heat_map, lm_loc=lm_loc_map)[0].cpu().numpy()


def NMS(dets, nms_thresh=0.4):
    d = torch.as_tensor(np.ascontiguousarray(dets, dtype=np.float64)).cuda()
    n, dc = d.shape
    keep = torch.empty(n + 1, dtype=torch.int32, device=d.device)
    scratch = torch.empty(5 * n + 16, dtype=torch.uint8, device=d.device)
    check(_lib.lib().dbx_nms(ptr(d), n, dc, float(nms_thresh), ptr(keep), ptr(scratch), stream_ptr()))
    return _keep_list(keep.cpu().numpy())


def _run_batch(score_map, loc_map, K, lm_heat=None, lm_loc=None, nms_thresh=0.4):
    """dbx_detect_batch over [B,C,rows,cols] maps: dets [B,K,5|13] float64, topk [B,K] int64, keep [B,K+1] int32 (device)."""
    s, l, hm, ll, B, rows, cols, dc, dev = _decode_inputs(score_map, loc_map, lm_heat, lm_loc)
    dets = torch.empty((B, K, dc), dtype=torch.float64, device=dev)
    topk = torch.empty((B, K), dtype=torch.int64, device=dev)
    keep = torch.empty((B, K + 1), dtype=torch.int32, device=dev)
    L = _lib.lib()
    scratch = torch.empty(L.dbx_detect_batch_scratch_bytes(B, rows, cols, K), dtype=torch.uint8, device=dev)
    check(L.dbx_detect_batch(ptr(s), ptr(l), ptr(hm), ptr(ll), B, rows, cols, K, float(nms_thresh), ptr(dets), dc, ptr(topk),
                             ptr(keep), ptr(scratch), stream_ptr()))
    return dets, topk, keep


_MAX_GRAPHS = 8


def _maps(kind, outs):
    """(score, loc, lm_heat, lm_loc) the decode ranks and reads per network: the refined score for the landmark nets
    (DenseBox.py:3626-3643, :3709-3726)."""
    if kind == 'DenseBox':
        return outs[0], outs[1], None, None
    if kind == 'DenseBoxLM':
        return outs[3], outs[1], outs[2], None
    return outs[1], outs[2], outs[3], outs[4]


def _forward_maps(net, images):
    with torch.no_grad():
        outs = net(images)
    return _maps(net.KIND, outs)


def _detect_eager(K, nms_thresh):
    def eager(net, image):
        s, l, hm, ll = _forward_maps(net, image)
        dets, _, keep = _run(s, l, image.size(2), image.size(3), K, lm_heat=hm, lm_loc=ll, nms_thresh=nms_thresh)
        return dets, keep
    return eager


def _detect_batch_eager(K, nms_thresh):
    def eager(net, images):
        s, l, hm, ll = _forward_maps(net, images)
        dets, _, keep = _run_batch(s, l, K, lm_heat=hm, lm_loc=ll, nms_thresh=nms_thresh)
        return dets, keep
    return eager


def _use_graph(net):
    """eval mode replays captured hipGraphs; train mode and DBX_GRAPH=0 run the same launches eagerly"""
    import os
    return not net.training and os.environ.get('DBX_GRAPH', '1') != '0'


def _run_chunk(net, tag, x, key, eager, host):
    """eager(net, x) -> a tuple of device tensors, through _graph_replay where _use_graph says so (and x is on the device); either way
    the results whose `host` flag is set come back as host tensors, the others as device tensors."""
    if x.is_cuda and _use_graph(net):
        return _graph_replay(net, tag, x, key, eager, host)
    return tuple(r.cpu() if f else r for r, f in zip(eager(net, x), host))


def _graph_replay(net, tag, x, key, eager, host):
    """Replays (capturing on the first call) one hipGraph of eager(net, x) -> a tuple of device tensors.  One cache per network, shared
    by every inference entry point: keyed by (tag, input shape, input dtype) + key + (compute dtype,), re-captured when the weight
    signature changes, at most _MAX_GRAPHS entries (LRU).

    eager is a closure that holds its own parameters; key is a hashable tuple in which the caller names everything a replay bakes in
    (kernel arguments such as K and the thresholds, buffer addresses, the serial of an evaluator or tracker, the first stream): two calls
    that differ in any of it must differ in key, or the second replays a stale graph.

    host: one bool per result.  A flagged result is copied to pinned memory by the graph and returned as that pinned host tensor, valid
    until the entry's next replay; an unflagged one is returned as the entry's own device tensor (or whatever eager returned in its
    place: the entry keeps it alive), valid in stream order until the entry's next replay -- e.g. detect_batch_thresh's arena, of which
    the counts decide how much to fetch: a copy of a size that depends on device data cannot be a graph node.  The stream is synchronised
    iff a flag is set; with none set nothing is copied and nothing waits (detect_pyramid's levels)."""
    import collections
    cache = net.__dict__.setdefault('_detect_graphs', collections.OrderedDict())
    # weight signature: versions + storage addresses of every parameter (a replay reads the packed copies made at capture).
    # Read straight from the sub-modules' parameter dicts (sees in-place updates, .to()/.half() and replaced Parameter
    # objects; 12 us instead of the 75 us Module.parameters() spends walking the tree); the list of dicts itself is
    # rebuilt every 64 calls in case a whole sub-module was swapped.
    # A replaced sub-module (net.conv6_3_det = nn.Conv2d(...)) changes the DIRECT children's identities: their ids are part
    # of the signature (one dict walk), and the cached list is rebuilt whenever they differ.
    kids = tuple(id(m) for m in net._modules.values())
    pd = net.__dict__.get('_detect_pdicts')
    if pd is None or pd[0] <= 0 or pd[2] != kids:
        pd = [64, [m._parameters for m in net.modules() if m._parameters], kids]
        net.__dict__['_detect_pdicts'] = pd
    pd[0] -= 1
    sig = (kids,) + tuple([(p._version, p.data_ptr()) for d in pd[1] for p in d.values() if p is not None])
    key = (tag, tuple(x.shape), x.dtype) + tuple(key) + (net.resolved_dtype(False),)
    ent = cache.get(key)
    if ent is None or ent[0] != sig:
        static_in = x.clone()
        for _ in range(2):                       # warm: workspace plan, packed weights, scratch buffers, kernel attributes
            warm = eager(net, static_in)
        assert len(host) == len(warm)
        pinned = tuple(torch.empty(w.shape, dtype=w.dtype).pin_memory() if f else None       # (pinned allocation is not capturable)
                       for w, f in zip(warm, host))
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        # No cyclic garbage collection DURING the capture: a dead network (modules sit in reference cycles) takes its cached graphs
        # with it, and destroying a graph while a stream captures is an error that ends the process.  Collect what is dead now, then
        # keep the collector off until the capture has ended (torch.cuda.graph no longer collects on entry).
        import gc
        gc.collect()
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(g):
                outs = tuple(eager(net, static_in))
                # the result copies are graph nodes too (pinned destinations): one replay + one stream sync per call
                # instead of two blocking .cpu() calls with their launch round trips (~60 us of idle GPU per call)
                for h, o in zip(pinned, outs):
                    if h is not None:
                        h.copy_(o, non_blocking=True)
        finally:
            if gc_was_on:
                gc.enable()
        # The captured kernels hold RAW pointers into the engine's workspace plan and packed / folded weight buffers.  The
        # engine keeps one plan and re-creates its weight caches when the dtype or mode flips, so the entry pins every
        # tensor it captured: a later forward at another shape (or a train-mode step) cannot free what a replay reads.
        ent = (sig, g, static_in, outs, net._engine.captured_refs(), pinned)
        cache[key] = ent
        while len(cache) > _MAX_GRAPHS:            # bounded: one graph + private pool + pinned workspace per shape
            cache.popitem(last=False)
    cache.move_to_end(key)
    _, g, static_in, outs, _refs, pinned = ent
    static_in.copy_(x)
    g.replay()
    if not any(host):
        return outs
    torch.cuda.current_stream().synchronize()
    return tuple(o if h is None else h for o, h in zip(outs, pinned))


def detect(net, image, K=10, nms_thresh=0.4):
    """Whole-image forward -> top-K -> decode -> NMS in one go (test / test_lm / test_lmloc drivers,
    DenseBox.py:3788-3799, :3626-3643, :3709-3726): ranks by the refined score for the landmark nets.
    Returns (dets[K, 5|13] float64 ndarray, keep list).

    In eval mode the ~25 launches of one image are captured into a hipGraph per (shape, K, dtype, weight version) and
    replayed (the single-image path is launch-bound: 0.8 ms eager vs the kernels' own time); DBX_GRAPH=0 keeps it eager."""
    assert image.dim() == 4 and image.size(0) == 1
    h_dets, h_keep = _run_chunk(net, 'detect', image, (K, float(nms_thresh)), _detect_eager(K, nms_thresh), (True, True))
    return h_dets.numpy().copy(), _keep_list(h_keep.numpy())


def _batch_of(x, what, fn='detect_batch'):
    """A 4-d network input from one tensor of `what`: float [B,3,H,W] or uint8 [B,H,W,3]."""
    if not torch.is_tensor(x):
        raise RuntimeError('%s: %s must be a tensor, got %s' % (fn, what, type(x).__name__))
    if x.dtype == torch.uint8:
        if x.dim() != 4 or x.size(3) != 3:
            raise RuntimeError('%s: uint8 %s must be [B,H,W,3] (HWC, RGB), got %s' % (fn, what, list(x.shape)))
    elif not x.is_floating_point() or x.dim() != 4 or x.size(1) != 3:
        raise RuntimeError('%s: %s must be float [B,3,H,W] or uint8 [B,H,W,3], got %s %s' % (fn, what, x.dtype, list(x.shape)))
    return x


def _on_device(x):
    return (x if x.is_cuda else x.cuda()).contiguous()


def _frame_count(fn, images):
    return len(images) if isinstance(images, (list, tuple)) else int(_batch_of(images, 'images', fn).size(0))


def _one_shape(fn, images, with_dtype):
    """RuntimeError when the tensors of a list of frames differ in shape (with_dtype: or in dtype): stream j is image j, so a list
    cannot be regrouped by shape as detect_batch does"""
    if isinstance(images, (list, tuple)):
        shapes = {(tuple(im.shape[-3:]), im.dtype if with_dtype else None) for im in images if torch.is_tensor(im)}
        if len(shapes) > 1:
            raise RuntimeError('%s: the frames of a list must have one shape%s (stream j is image j), got %s'
                               % (fn, ' and dtype' if with_dtype else '', sorted(str(s[0]) for s in shapes)))


def _detect_chunk(net, x, K, nms_thresh):
    h_dets, h_keep = _run_chunk(net, 'batch', x, (K, float(nms_thresh)), _detect_batch_eager(K, nms_thresh), (True, True))
    d, k = h_dets.numpy(), h_keep.numpy()
    return [(d[b].copy(), _keep_list(k[b])) for b in range(d.shape[0])]


def detect_batch(net, images, K=10, nms_thresh=0.4, max_batch=32):
    """detect() over many images: one forward and ONE decode + NMS launch (a workgroup per image, dbx_detect_batch) per chunk
    of at most `max_batch` images.  Returns a list with detect()'s (dets[K, 5|13] float64 ndarray, keep list) per image, in
    input order.

    images: a float [B,3,H,W] or uint8 [B,H,W,3] (RGB, normalised on the device) tensor on the CPU or the GPU, or a list /
    tuple of single images -- float [3,H,W] or [1,3,H,W], uint8 [H,W,3] or [1,H,W,3] -- of any sizes (the reference test()
    loop's directory walk).  List images are grouped by (shape, dtype) and never padded into one forward: padding would change
    the border activations after the first pooling and the bilinear up-sampling.  Eval mode replays a hipGraph per (batch
    shape, dtype, K, threshold, compute dtype) from the cache detect() uses; train mode and DBX_GRAPH=0 run eagerly."""
    return _detect_many('detect_batch', images, max_batch, lambda x: _detect_chunk(net, x, K, nms_thresh))


def _detect_many(fn, images, max_batch, chunk, with_index=False):
    """detect_batch's walk over a batch tensor or a list of single images: chunk(x) -> list of per-image results for every chunk of at
    most max_batch same-shape images (x a contiguous device tensor), results in input order.  Every check runs before the first chunk.  with_index: chunk(x, idx) also
    gets the input positions of the chunk's images (evaluate_batch finds their ground truth by them)."""
    if max_batch < 1:
        raise RuntimeError('%s: max_batch=%d must be positive' % (fn, max_batch))
    if not isinstance(images, (list, tuple)):
        x = _batch_of(images, 'images', fn)
        if x.size(0) == 0:
            raise RuntimeError('%s: empty batch' % fn)
        out = []
        for i in range(0, x.size(0), max_batch):
            part = x[i:i + max_batch]
            part = _on_device(part)
            out += chunk(part, list(range(i, i + part.size(0)))) if with_index else chunk(part)
        return out
    if len(images) == 0:
        raise RuntimeError('%s: empty list of images' % fn)
    one = []
    for i, im in enumerate(images):
        if torch.is_tensor(im) and im.dim() == 3:
            im = im.unsqueeze(0)
        one.append(_batch_of(im, 'images[%d]' % i, fn))
        if one[-1].size(0) != 1:
            raise RuntimeError('%s: images[%d] holds %d images; a list takes single images' % (fn, i, one[-1].size(0)))
    if len({im.dtype == torch.uint8 for im in one}) > 1:
        raise RuntimeError('%s: the list mixes uint8 [H,W,3] and float [3,H,W] images' % fn)
    groups = {}
    for i, im in enumerate(one):
        groups.setdefault((tuple(im.shape), im.dtype), []).append(i)
    out = [None] * len(one)
    for idx in groups.values():
        for c in range(0, len(idx), max_batch):
            part = idx[c:c + max_batch]
            dev = next((one[i].device for i in part if one[i].is_cuda), torch.device('cuda'))
            x = torch.cat([one[i].to(dev) for i in part])
            res = chunk(x, part) if with_index else chunk(x)
            for i, r in zip(part, res):
                out[i] = r
    return out


# ---------------------------------------------------------------------------------------------- score-threshold detection
_THRESH_MAX_DETS = 4096          # dbx_detect_thresh_batch's bound on max_dets (one wave holds the removed set: 64 lanes x 64 bits)


def _check_thresh(fn, score_thresh, max_dets):
    """(float threshold, int cap) or RuntimeError: a finite real number (no bool), an integer in 1..4096 (no bool)."""
    ok = isinstance(score_thresh, (int, float, np.integer, np.floating)) and not isinstance(score_thresh, (bool, np.bool_))
    if not ok or not np.isfinite(float(score_thresh)):
        raise RuntimeError('%s: score_thresh=%r must be a finite number' % (fn, score_thresh))
    if not _integer(max_dets) or not 1 <= max_dets <= _THRESH_MAX_DETS:
        raise RuntimeError('%s: max_dets=%r must be an integer in 1..%d' % (fn, max_dets, _THRESH_MAX_DETS))
    return float(np.float32(score_thresh)), int(max_dets)


def _run_thresh_batch(score_map, loc_map, score_thresh, max_dets, lm_heat=None, lm_loc=None, nms_thresh=0.4, lists_behind_rows=True):
    """dbx_detect_thresh_batch over [B,C,rows,cols] maps: (rows buffer, keep buffer, counts int32 [3 B + 1]) device tensors, packed.
    lists_behind_rows: both buffers are ONE uint8 arena with the keep lists right behind the packed rows, which _unpack_thresh reads;
    otherwise the rows are float64 [B * max_dets, 5|13] and the lists int32 [B * (max_dets + 1)], tensors of their own."""
    s, l, hm, ll, B, rows, cols, dc, dev = _decode_inputs(score_map, loc_map, lm_heat, lm_loc)
    if lists_behind_rows:
        dets = keep = torch.empty(B * max_dets * dc * 8 + B * (max_dets + 1) * 4, dtype=torch.uint8, device=dev)
    else:
        dets = torch.empty((B * max_dets, dc), dtype=torch.float64, device=dev)
        keep = torch.empty(B * (max_dets + 1), dtype=torch.int32, device=dev)
    topk = torch.empty(B * max_dets, dtype=torch.int64, device=dev)
    counts = torch.empty(3 * B + 1, dtype=torch.int32, device=dev)
    L = _lib.lib()
    scratch = torch.empty(L.dbx_detect_thresh_batch_scratch_bytes(B, rows, cols, max_dets), dtype=torch.uint8, device=dev)
    check(L.dbx_detect_thresh_batch(ptr(s), ptr(l), ptr(hm), ptr(ll), B, rows, cols, float(score_thresh), max_dets, float(nms_thresh),
                                    ptr(dets), dc, ptr(topk), ptr(keep), ptr(counts), ptr(scratch), stream_ptr()))
    return dets, keep, counts


def _thresh_fetch_bytes(counts, dc):
    """bytes of the arena that hold the call's rows and keep lists, from the host copy of the counts"""
    B = (counts.shape[0] - 1) // 3
    return int(counts[3 * B]) * (dc * 8 + 4) + B * 4


def _unpack_packed(prefix, rows, lists, dc):
    """Per image (dets [n_b, dc] float64, keep list) from host arrays in the packed layout of dbx_detect_thresh_batch and
    dbx_merge_nms_thresh_batch: with P = prefix, the [B + 1] running sum of the row counts, image b owns rows P[b] .. P[b + 1] - 1
    (n_b = P[b + 1] - P[b]) and the list [count, idx...] at word P[b] + b.  rows: the uint8 arena or a float64 array of at least
    P[B] rows; lists: an int32 array, or None for the lists right behind the rows in the arena."""
    B, total = prefix.shape[0] - 1, int(prefix[-1])
    if lists is None:
        lists = rows[total * dc * 8:total * dc * 8 + (total + B) * 4].view(np.int32)
    if rows.dtype == np.uint8:
        rows = rows[:total * dc * 8].view(np.float64)
    rows = rows.reshape(-1)[:total * dc].reshape(total, dc)
    out = []
    for b in range(B):
        p, n = int(prefix[b]), int(prefix[b + 1] - prefix[b])
        out.append((rows[p:p + n].copy(), _keep_list(lists[p + b:p + b + n + 1])))
    return out


def _unpack_thresh(counts, arena, dc, with_totals):
    """per image (dets [n_b, dc] float64, keep list[, pixels above the threshold]) from host arrays: the counts and the fetched arena"""
    B = (counts.shape[0] - 1) // 3
    out = _unpack_packed(counts[2 * B:], arena, None, dc)
    return [r + (int(counts[2 * b + 1]),) for b, r in enumerate(out)] if with_totals else out


def _thresh_batch_eager(score_thresh, max_dets, nms_thresh):
    def eager(net, images):
        s, l, hm, ll = _forward_maps(net, images)
        arena, _, counts = _run_thresh_batch(s, l, score_thresh, max_dets, lm_heat=hm, lm_loc=ll, nms_thresh=nms_thresh)
        return arena, counts
    return eager


def _pinned(net, nbytes):
    """the network's grow-only pinned staging buffer, at least nbytes long: it grows to the largest fetch seen, never to an arena's
    capacity"""
    pin = net.__dict__.get('_thresh_pinned')
    if pin is None or pin.numel() < nbytes:
        pin = net.__dict__['_thresh_pinned'] = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8).pin_memory()
    return pin


def _thresh_chunk(net, x, score_thresh, max_dets, nms_thresh, with_totals):
    dc = _det_cols(net)
    arena, counts = _run_chunk(net, 'thresh', x, ((max_dets, score_thresh), float(nms_thresh)),
                               _thresh_batch_eager(score_thresh, max_dets, nms_thresh), (False, True))
    counts = counts.numpy().copy()
    nbytes = _thresh_fetch_bytes(counts, dc)
    pin = _pinned(net, nbytes)
    pin[:nbytes].copy_(arena[:nbytes], non_blocking=True)        # the ONE copy whose size the counts decide, behind the replay
    torch.cuda.current_stream().synchronize()
    return _unpack_thresh(counts, pin[:nbytes].numpy().copy(), dc, with_totals)


def detect_batch_thresh(net, images, score_thresh, max_dets=1024, nms_thresh=0.4, max_batch=32, with_totals=False):
    """detect_batch with a score threshold in the place of the fixed top-K: per image EVERY pixel whose (refined) score is above
    `score_thresh` becomes a row -- at most `max_dets` of them, the best ones when more pass -- and the reference's greedy NMS runs
    over all of them on the device (dbx_detect_thresh_batch; the NMS handles up to 4096 rows on many CUs).  For
    n_b = min(#{score > score_thresh}, max_dets) image b's result is bit for bit detect_batch(K = n_b)'s.

    images, max_batch, chunking and list grouping: detect_batch's.  score_thresh: a finite number, compared in fp32, strictly (a score
    equal to it is out; NaN scores never pass).  max_dets: an integer in 1..4096.

    Returns, per image in input order, (dets float64 [n_b, 5|13], keep list of int); n_b may be 0 (dets.shape == (0, 5|13),
    keep == []).  with_totals=True: 3-tuples whose last item is the number of pixels above the threshold (> n_b when the cap cut).

    Eval mode replays ONE hipGraph per chunk from the cache detect() uses, under a tag of its own, keyed by (batch shape, dtype,
    (max_dets, score_thresh), nms_thresh, compute dtype): the forward, the three decode launches and the copy of the per-image counts
    to pinned memory; the rows and keep lists then come with ONE copy of exactly their size (one replay, two stream synchronises per
    chunk).  Both thresholds are kernel arguments baked in at capture, as K is: SWEEPING score_thresh RE-CAPTURES at every new value,
    and the cache holds _MAX_GRAPHS = 8 entries per network.  Train mode and DBX_GRAPH=0 run the same launches eagerly."""
    t, cap = _check_thresh('detect_batch_thresh', score_thresh, max_dets)
    return _detect_many('detect_batch_thresh', images, max_batch,
                        lambda x: _thresh_chunk(net, x, t, cap, nms_thresh, bool(with_totals)))


def _thresh_or_topk(fn, K, score_thresh, max_dets):
    """None for the top-K path; (threshold, cap) for the threshold path, where a non-default K is a contradiction"""
    if score_thresh is None:
        return None
    if K != 10:
        raise RuntimeError('%s: K=%r and score_thresh=%r are both given; the threshold decode takes max_dets, not K' % (fn, K, score_thresh))
    return _check_thresh(fn, score_thresh, max_dets)


def detect_plates(net, images, K=10, nms_thresh=0.4, max_batch=32, *, region, score_thresh=None, max_dets=1024):
    """detect_batch, then perspective_transform (DenseBox.py:3446-3481, as viz_result calls it at :3546-3553) on every kept
    detection: the frames go to the device once, and ONE dbx_warp_perspective_batch_u8 launch rectifies the plates of all chunks.

    images: uint8 frames only -- a [B,H,W,3] tensor or a list of [H,W,3] images (numpy arrays or tensors) of any sizes; those are
    the pixels the reference warps.  net: DenseBoxLM or DenseBoxLMLOC (rows with landmarks).  region: 'canvas' (the reference's
    whole 1.5x image) or 'plate' (its window over the plate rectangle), as for rectify.perspective_transform_batch.

    Returns, per image in input order, (dets, keep, plates): detect_batch's (dets, keep) unchanged, and plates[j] the uint8
    [oh, ow, 3] rectification of row keep[j], whose quad is (det[5:7], det[7:9], det[9:11], det[11:13]) = (left-up, right-up,
    right-down, left-down), or None where rectify.perspective_transform_batch gives None.  Plates are of the kind of their frame
    (CUDA tensors are views into one device arena).  detect_batch replays its cached hipGraphs in eval mode; the rectification
    launch is NOT captured, because its size depends on the detections.

    score_thresh: None runs the top-K decode above; a number runs detect_batch_thresh(score_thresh, max_dets) in its place (K is then
    ignored; a non-default K together with a threshold raises), and dets has n_b rows."""
    from . import rectify
    rectify.check_region('detect_plates', region)
    tc = _thresh_or_topk('detect_plates', K, score_thresh, max_dets)
    _require_landmarks('detect_plates', net)
    host, kinds = rectify.host_images('detect_plates', images, 3)
    if torch.is_tensor(images):                    # one upload of the batch; the forward and the warp read the same device copy
        x = _on_device(images)
        dev = list(x.unbind(0))
    else:
        x = dev = rectify.to_device(images, host)
    res = detect_batch(net, x, K, nms_thresh, max_batch) if tc is None else detect_batch_thresh(net, x, tc[0], tc[1], nms_thresh, max_batch)
    quads = [[[[d[k, 5], d[k, 6]], [d[k, 7], d[k, 8]], [d[k, 9], d[k, 10]], [d[k, 11], d[k, 12]]] for k in keep] for d, keep in res]
    plates = rectify._warp_batch(dev, kinds, quads, region)
    return [(d, keep, p) for (d, keep), p in zip(res, plates)]


def _plate_crops_eager(K, ow, oh, nms_thresh):
    """The eager function of detect_plate_crops' chunks: forward, dbx_detect_batch, dbx_plate_crops_batch -> (dets, keep, crops, ok,
    frame table) device tensors.  The crop launch reads the pixels of `images` (the graph's static input under capture), the quads at
    dets + 5 and the kept rows in keep.  The frame table is the one thing that comes from the host: it is uploaded on the first call for
    a tensor (the warm-up, outside the capture) and reused for the same address afterwards; the graph entry keeps it with the results."""
    from . import rectify
    detect, tables = _detect_batch_eager(K, nms_thresh), {}

    def eager(net, images):
        dets, keep = detect(net, images)
        B, dc = int(dets.size(0)), int(dets.size(2))
        key = (images.data_ptr(), tuple(images.shape))
        table = tables.get(key)
        if table is None:
            table = tables[key] = rectify.frame_table(list(images.unbind(0)))
        crops, ok = rectify._crops_launch(table, B, 3, dets.data_ptr() + 5 * 8, dc, K * dc, keep, K, ow, oh, images.device)
        return dets, keep, crops, ok, table
    return eager


def _plate_crops_chunk(net, x, K, ow, oh, nms_thresh, host_crops):
    d, k, crops, ok, _ = _run_chunk(net, 'plate_crops', x, ((K, ow, oh, host_crops), float(nms_thresh)),
                                    _plate_crops_eager(K, ow, oh, nms_thresh), (True, True, host_crops, True, False))
    d, k, ok = d.numpy(), k.numpy(), ok.numpy()
    out = []
    for b in range(d.shape[0]):
        keep = _keep_list(k[b])
        # every result owns its memory (a graph entry's buffers are overwritten by its next replay): crops by a clone, device to device
        # for CUDA frames
        out.append((d[b].copy(), keep, crops[b, :len(keep)].clone(), ok[b, :len(keep)] != 0))
    return out


def detect_plate_crops(net, images, *, size, K=10, nms_thresh=0.4, max_batch=32):
    """detect_batch, then every kept detection's plate rectified to ONE crop size on the device -- the input of a plate recogniser --
    with no host work between the decode and the warp: per chunk of at most `max_batch` same-shape frames the forward, dbx_detect_batch
    and ONE dbx_plate_crops_batch launch, which reads the frames' pixels, the quads in columns 5..12 of the rows and the kept rows in
    `keep` where the decode left them and solves the homographies itself (rectify.plate_crops_batch has the semantics).

    images: uint8 frames only -- a [B,H,W,3] tensor or a list of [H,W,3] images (numpy arrays or tensors) of any sizes, as for
    detect_plates; each is uploaded at most once.  net: DenseBoxLM or DenseBoxLMLOC.  size: (width, height) of a crop, e.g. (94, 24),
    or one integer for both.  K, nms_thresh, max_batch, chunking and list grouping: detect_batch's.

    Returns, per image in input order, (dets, keep, crops, ok): detect_batch's (dets, keep) bit for bit; crops uint8
    [len(keep), oh, ow, 3] of the kind of the frame (numpy array, CPU tensor or CUDA tensor), crop j the rectification of row keep[j]
    onto rectify.plate_rectangle(size); ok a numpy bool [len(keep)], False (and the crop all zeros) where the quad is degenerate or not
    finite -- where detect_plates gives None.  Every result owns its memory.

    Eval mode replays ONE hipGraph per chunk from the cache detect() uses, under a tag of its own, keyed by (batch shape, dtype,
    (K, ow, oh, crops to the host), nms_thresh, compute dtype): the forward, the decode, the crop launch and the copies of dets, keep,
    ok -- and of the crops, when the frames came from the host -- to pinned memory; one replay and one stream synchronise per chunk.
    Train mode and DBX_GRAPH=0 run the same three steps eagerly.

    There is no score_thresh here: the threshold decode has up to 4096 rows per image, and fixed slots for that many are a different
    design (most of them empty, or a compaction pass); use detect_batch_thresh and rectify.plate_crops_batch for it."""
    from . import rectify
    ow, oh = rectify._crop_size('detect_plate_crops', size)
    _require_landmarks('detect_plate_crops', net)
    host, kinds = rectify.host_images('detect_plate_crops', images, 3)
    host_crops = any(k != 'cuda' for k in kinds)
    if torch.is_tensor(images):                    # one upload of the batch; the forward and the warp read the same device copy
        x = _on_device(images)
    else:
        x = rectify.to_device(images, host)
    res = _detect_many('detect_plate_crops', x, max_batch, lambda c: _plate_crops_chunk(net, c, K, ow, oh, nms_thresh, host_crops))
    out = []
    for (d, keep, crops, ok), kind in zip(res, kinds):
        if kind == 'cuda':
            crops = crops if crops.is_cuda else crops.cuda()         # (a CUDA frame in a list that also holds host frames)
        out.append((d, keep, crops.numpy() if kind == 'numpy' else crops, ok))
    return out


def detect_batch_resized(net, images, size=720, K=10, nms_thresh=0.4, max_batch=32, score_thresh=None, max_dets=1024):
    """detect_batch on frames of ANY sizes through the reference's own answer to mixed sizes: every frame is padded to a square with
    grey 128 and resized to size x size with INTER_CUBIC (pad_img + cv2.resize, batch_pad_resize, DenseBox.py:1282-1340) in ONE
    dbx_resize_cubic_batch_u8 launch, and the resulting uint8 [B, size, size, 3] tensor takes detect_batch's tensor path: a
    mixed-size list runs in ceil(B / max_batch) forwards and replays ONE cached hipGraph shape.  The resize launch is NOT captured
    (its job list depends on the call).

    images: uint8 frames only -- a [B,H,W,3] tensor or a list of [H,W,3] images (numpy arrays or tensors); each is uploaded once.
    size: a positive multiple of 4.

    Returns, per image in input order, (dets, keep).  keep is detect_batch's for the resized frame, unchanged.  dets is its float64
    row array with every coordinate column (0..3, and 5..12 for the landmark nets; column 4, the score, stays) mapped back to the
    source frame in float64: x_src = x * (side / size) - pad_x, y_src = y * (side / size) - pad_y with
    (side, pad_x, pad_y) = resize.pad_geometry(H, W).  So plates are rectified from the full-resolution frames by

        res = net.detect_batch_resized(frames)
        quads = [[[d[k, 5:7], d[k, 7:9], d[k, 9:11], d[k, 11:13]] for k in keep] for d, keep in res]
        plates = rectify.perspective_transform_batch(frames, quads, region='plate')

    score_thresh: None runs the top-K decode above; a number runs detect_batch_thresh(score_thresh, max_dets) on the resized frames
    in its place (K is then ignored; a non-default K together with a threshold raises), and dets has n_b rows."""
    from . import rectify, resize
    tc = _thresh_or_topk('detect_batch_resized', K, score_thresh, max_dets)
    if not _integer(size) or size < 4 or size % 4:
        raise RuntimeError('detect_batch_resized: size=%r must be a positive multiple of 4 (the maps are size / 4)' % (size,))
    host, _ = rectify.host_images('detect_batch_resized', images, 3)
    x = resize._pad_resize_device(rectify.to_device(images, host), int(size))
    res = detect_batch(net, x, K, nms_thresh, max_batch) if tc is None else detect_batch_thresh(net, x, tc[0], tc[1], nms_thresh, max_batch)
    return _map_back([(im.size(0), im.size(1)) for im in host], res, size)


def _map_back(hw, res, size):
    """detect_batch_resized's rows in source-frame coordinates: hw[b] = (H, W) of frame b, res[b] = (dets, keep) on its resized frame"""
    from . import resize
    out = []
    for (h, w), (d, keep) in zip(hw, res):
        side, pad_x, pad_y = resize.pad_geometry(h, w)
        s = side / int(size)
        d = d.copy()
        xs = [0, 2] + list(range(5, d.shape[1], 2))
        ys = [1, 3] + list(range(6, d.shape[1], 2))
        d[:, xs] = d[:, xs] * s - pad_x
        d[:, ys] = d[:, ys] * s - pad_y
        out.append((d, keep))
    return out


_PYRAMID_MAX_LEVELS = 4          # each level (and possibly its tail chunk) owns a cached graph shape, and _MAX_GRAPHS is 8
_MERGE_MAX_ROWS = 4096           # dbx_merge_nms_batch's bound on levels * K


def _check_pyramid_sizes(sizes):
    ok = isinstance(sizes, (list, tuple)) and 1 <= len(sizes) <= _PYRAMID_MAX_LEVELS
    ok = ok and all(_integer(s) and s >= 4 and s % 4 == 0 for s in sizes)
    if not ok or len({int(s) for s in sizes}) != len(sizes):
        raise RuntimeError('detect_pyramid: sizes=%r must be 1 to %d distinct positive multiples of 4 (the maps are size / 4; every '
                           'level owns a cached graph shape)' % (sizes, _PYRAMID_MAX_LEVELS))
    return [int(s) for s in sizes]


def _xform_table(xform, levels, b):
    """the host array of dbx_merge_xform [levels][b] from xform [levels][b] (scale, off_x, off_y) triples"""
    xf = (_lib.MergeXform * (levels * b))()
    for l in range(levels):
        for i in range(b):
            xf[l * b + i].scale, xf[l * b + i].off_x, xf[l * b + i].off_y = xform[l][i]
    return xf


def _merge_nms(level_dets, xform, nms_thresh, out_dets, out_keep):
    """ONE dbx_merge_nms_batch launch: level_dets a list of L device [b, K, dc] float64 tensors, xform [L][b] (scale, off_x, off_y)
    triples, out_dets [b, L * K, dc] / out_keep [b, L * K + 1] device tensors (views of larger ones are fine: both are dense)."""
    levels, (b, K, dc) = len(level_dets), level_dets[0].shape
    ptrs = (C.c_void_p * levels)(*[t.data_ptr() for t in level_dets])
    xf = _xform_table(xform, levels, b)
    L = _lib.lib()
    nbytes = L.dbx_merge_nms_batch_workspace_bytes(levels, b, K)
    if nbytes < 0:
        raise RuntimeError('detect_pyramid: %d levels x K=%d rows per frame exceed %d' % (levels, K, _MERGE_MAX_ROWS))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=out_dets.device)
    check(L.dbx_merge_nms_batch(ptrs, xf, levels, b, K, dc, float(nms_thresh), ptr(out_dets), ptr(out_keep), ptr(ws), stream_ptr()))


def _run_thresh_rows(score_map, loc_map, score_thresh, max_dets, lm_heat=None, lm_loc=None):
    """dbx_thresh_rows_batch over [B,C,rows,cols] maps: (dets float64 [B, max_dets, 5|13], topk int64 [B, max_dets], counts int32 [B, 2])
    device tensors in slot layout; only the first counts[b, 0] rows of image b are written."""
    s, l, hm, ll, B, rows, cols, dc, dev = _decode_inputs(score_map, loc_map, lm_heat, lm_loc)
    dets = torch.empty((B, max_dets, dc), dtype=torch.float64, device=dev)
    topk = torch.empty((B, max_dets), dtype=torch.int64, device=dev)
    counts = torch.empty((B, 2), dtype=torch.int32, device=dev)
    L = _lib.lib()
    scratch = torch.empty(L.dbx_thresh_rows_batch_scratch_bytes(B, rows, cols, max_dets), dtype=torch.uint8, device=dev)
    check(L.dbx_thresh_rows_batch(ptr(s), ptr(l), ptr(hm), ptr(ll), B, rows, cols, float(score_thresh), max_dets, ptr(dets), dc,
                                  ptr(topk), ptr(counts), ptr(scratch), stream_ptr()))
    return dets, topk, counts


def _thresh_rows_eager(score_thresh, max_dets):
    def eager(net, images):
        s, l, hm, ll = _forward_maps(net, images)
        dets, _, counts = _run_thresh_rows(s, l, score_thresh, max_dets, lm_heat=hm, lm_loc=ll)
        return dets, counts
    return eager


def _merge_nms_thresh(level_dets, level_counts, xform, nms_thresh, arena, out_counts):
    """ONE dbx_merge_nms_thresh_batch call: level_dets / level_counts lists of L device [b, max_dets, dc] float64 / [b, 2] int32 tensors
    (_run_thresh_rows), xform [L][b] triples; arena uint8 (packed rows, the keep lists right behind them), out_counts int32
    [2 * b * L + b + 1], both on the device."""
    levels, (b, cap, dc) = len(level_dets), level_dets[0].shape
    dp = (C.c_void_p * levels)(*[t.data_ptr() for t in level_dets])
    cp = (C.c_void_p * levels)(*[t.data_ptr() for t in level_counts])
    xf = _xform_table(xform, levels, b)
    L = _lib.lib()
    ws = torch.empty(L.dbx_merge_nms_thresh_batch_workspace_bytes(levels, b, cap), dtype=torch.uint8, device=arena.device)
    check(L.dbx_merge_nms_thresh_batch(dp, cp, xf, levels, b, cap, dc, float(nms_thresh), ptr(arena), ptr(arena), ptr(out_counts), ptr(ws),
                                       stream_ptr()))


def _pyramid_counts_words(b, levels):
    return 2 * b * levels + b + 1


def _pyramid_thresh_fetch_bytes(counts, levels, dc):
    """bytes of a chunk's arena that hold its rows and keep lists, from the host copy of the chunk's merge counts
    ([b][levels][2] pairs, then the [b + 1] prefix of the union sizes)"""
    b = (counts.shape[0] - 1) // (2 * levels + 1)
    return int(counts[-1]) * (dc * 8 + 4) + b * 4


def _unpack_pyramid_thresh(counts, arena, levels, dc, with_levels):
    """per frame (dets [m_b, dc] float64, keep list[, rows per level]) from host arrays: a chunk's merge counts and its fetched arena"""
    b = (counts.shape[0] - 1) // (2 * levels + 1)
    out = _unpack_packed(counts[2 * b * levels:], arena, None, dc)
    if with_levels:
        pairs = counts[:2 * b * levels].reshape(b, levels, 2)
        out = [r + (pairs[i, :, 0].astype(np.int64),) for i, r in enumerate(out)]
    return out


def _pyramid_thresh(net, levels, xform, B, t, cap, nms_thresh, max_batch, with_levels):
    """detect_pyramid's threshold path over the resized levels: everything is queued first, then the counts come to the host, then
    exactly the rows and lists"""
    nl, dc, dev = len(levels), _det_cols(net), levels[0].device
    eager = _thresh_rows_eager(t, cap)
    spans = [(c0, min(B, c0 + max_batch)) for c0 in range(0, B, max_batch)]
    offs = np.cumsum([0] + [_pyramid_counts_words(c1 - c0, nl) for c0, c1 in spans])
    counts_dev = torch.empty(int(offs[-1]), dtype=torch.int32, device=dev)
    arenas = []
    for (c0, c1), o0, o1 in zip(spans, offs[:-1], offs[1:]):
        rows, cnts = [], []
        for lv in levels:
            # (a graph entry's device rows and counts: overwritten by its next replay, queued behind this chunk's merge)
            d, c = _run_chunk(net, 'level_thresh', lv[c0:c1], ((cap, t), float(nms_thresh)), eager, (False, False))
            rows.append(d)
            cnts.append(c)
        b = c1 - c0
        arena = torch.empty(b * nl * cap * (dc * 8 + 4) + b * 4, dtype=torch.uint8, device=dev)
        _merge_nms_thresh(rows, cnts, [xf[c0:c1] for xf in xform], nms_thresh, arena, counts_dev[int(o0):int(o1)])
        arenas.append(arena)
    counts = counts_dev.cpu().numpy()                                # the first wait of the call
    parts = [counts[int(o0):int(o1)] for o0, o1 in zip(offs[:-1], offs[1:])]
    nbytes = [_pyramid_thresh_fetch_bytes(c, nl, dc) for c in parts]
    pin = _pinned(net, sum(nbytes))
    at = np.cumsum([0] + nbytes)
    for arena, a0, nb in zip(arenas, at[:-1], nbytes):
        pin[int(a0):int(a0) + nb].copy_(arena[:nb], non_blocking=True)
    torch.cuda.current_stream().synchronize()                        # the second and last
    host = pin[:int(at[-1])].numpy().copy()
    out = []
    for c, a0, nb in zip(parts, at[:-1], nbytes):
        out += _unpack_pyramid_thresh(c, host[int(a0):int(a0) + nb], nl, dc, with_levels)
    return out


def detect_pyramid(net, images, sizes=(480, 720, 1080), K=10, nms_thresh=0.4, max_batch=32, score_thresh=None, max_dets=1024,
                   with_levels=False):
    """Multi-scale detection, the test-time image pyramid of the DenseBox paper: every frame is padded to a square and resized to
    EVERY size of `sizes` (what detect_batch_resized does for one size) in ONE dbx_resize_cubic_batch_u8 launch; per chunk of at most
    `max_batch` frames each level runs one forward + one dbx_detect_batch (in eval mode a cached hipGraph per level shape whose rows
    stay on the device), and ONE dbx_merge_nms_batch launch maps the rows of all levels back to the source frames and runs the
    reference's greedy NMS over their union, a workgroup per frame.  One copy brings the results of the call to the host.  The resize
    and the merge launches are not captured; train mode and DBX_GRAPH=0 run the same launches eagerly.

    images: uint8 frames only -- a [B,H,W,3] tensor or a list of [H,W,3] images (numpy arrays or tensors, on the CPU or the GPU) of
    any sizes; each is uploaded at most once.  sizes: 1 to 4 distinct positive multiples of 4.  The default is the reference's single
    720 (batch_pad_resize) with 2/3 and 3/2 of it: a convention, NOT a tuned value -- no trained weights exist in this tree to tune
    it with.  K: rows per level (len(sizes) * K <= 4096).

    Returns, per frame in input order, (dets, keep): dets the float64 [len(sizes) * K, 5|13] rows in SOURCE-frame coordinates, level
    by level in the order of `sizes` (row l * K + r is row r of detect_batch_resized(..., size=sizes[l]); x_src = x * (side / size) -
    pad_x, y_src = y * (side / size) - pad_y with (side, pad_x, pad_y) = resize.pad_geometry(H, W)), and keep the row indices the NMS
    over all of them keeps, in the reference's order (the level of a kept row is index // K).  So plates are rectified from the
    full-resolution frames by

        res = net.detect_pyramid(frames)
        quads = [[[d[k, 5:7], d[k, 7:9], d[k, 9:11], d[k, 11:13]] for k in keep] for d, keep in res]
        plates = rectify.perspective_transform_batch(frames, quads, region='plate')

    score_thresh: None runs the top-K decode above.  A number (max_dets an integer with len(sizes) * max_dets <= 4096; K is then ignored,
    and a non-default K together with a threshold raises) makes every level decode every pixel above the threshold, as
    detect_batch_thresh does: per chunk and level one forward + one dbx_thresh_rows_batch (a cached hipGraph per level shape under a
    tag of its own, keyed by (max_dets, score_thresh); rows and counts stay on the device), then ONE dbx_merge_nms_thresh_batch per
    chunk reads the counts on the device, packs the mapped rows of each frame and runs the NMS over its union of m_b rows.  The host
    waits twice per call: for the counts of all chunks, then for exactly the rows and lists they announce.  Returns, per frame in input
    order, (dets float64 [m_b, 5|13], keep); m_b may be 0.  with_levels=True adds a third item, the int array [len(sizes)] of the rows
    each level gave (the level of row i follows from its cumulative sum).  The result is bit for bit detect_batch_resized(frames,
    size=s, score_thresh=..., max_dets=..., max_batch=...) per size, the rows of each frame concatenated in the order of `sizes`, and
    decode.NMS over them."""
    from . import rectify, resize
    sizes = _check_pyramid_sizes(sizes)
    tc = _thresh_or_topk('detect_pyramid', K, score_thresh, max_dets)
    if tc is not None and len(sizes) * tc[1] > _MERGE_MAX_ROWS:
        raise RuntimeError('detect_pyramid: len(sizes)=%d levels x max_dets=%d rows exceed %d rows per frame'
                           % (len(sizes), tc[1], _MERGE_MAX_ROWS))
    if not _integer(max_batch) or max_batch < 1:
        raise RuntimeError('detect_pyramid: max_batch=%r must be a positive integer' % (max_batch,))
    if not _integer(K) or K < 1 or len(sizes) * K > _MERGE_MAX_ROWS:
        raise RuntimeError('detect_pyramid: K=%r must be a positive integer with len(sizes) * K <= %d' % (K, _MERGE_MAX_ROWS))
    host, _ = rectify.host_images('detect_pyramid', images, 3)
    K, max_batch, B, nl = int(K), int(max_batch), len(host), len(sizes)
    dev = rectify.to_device(images, host)
    levels = resize._pad_resize_levels(dev, sizes)
    xform = [[resize.level_xform(im.size(0), im.size(1), s) for im in host] for s in sizes]
    if tc is not None:
        return _pyramid_thresh(net, levels, xform, B, tc[0], tc[1], nms_thresh, max_batch, bool(with_levels))
    dc, n, eager = _det_cols(net), nl * K, _detect_batch_eager(K, nms_thresh)
    # one device buffer for the whole call: [B][n][dc] float64 rows, then [B][n + 1] int32 keep lists -- a single copy to the host
    nd = B * n * dc * 8
    buf = torch.empty(nd + B * (n + 1) * 4, dtype=torch.uint8, device=dev[0].device)
    out_dets, out_keep = buf[:nd].view(torch.float64).view(B, n, dc), buf[nd:].view(torch.int32).view(B, n + 1)
    for c0 in range(0, B, max_batch):
        c1 = min(B, c0 + max_batch)
        rows = []
        for lv in levels:
            # (a graph entry's device rows: overwritten by its next replay, which is queued behind this chunk's merge)
            rows.append(_run_chunk(net, 'level', lv[c0:c1], (K, float(nms_thresh)), eager, (False, False))[0])
        _merge_nms(rows, [xf[c0:c1] for xf in xform], nms_thresh, out_dets[c0:c1], out_keep[c0:c1])
    h = buf.cpu()
    d = h[:nd].view(torch.float64).view(B, n, dc).numpy()
    k = h[nd:].view(torch.int32).view(B, n + 1).numpy()
    return [(d[b].copy(), _keep_list(k[b])) for b in range(B)]
