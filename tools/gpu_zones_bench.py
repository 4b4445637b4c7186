"""Zones on the device next to what a user could write before them, at 512x512 B=32 (32 camera streams, one frame each per call) on a
synthetic DenseBoxLMLOC (f16), top-K mode, K=10; every stream has 2 lines, 2 count regions and 1 include polygon:
  (a) watch_batch: forward, decode + NMS, dbx_zone_filter_keep, dbx_track_update_batch, dbx_zone_update_batch, dbx_track_append and
      dbx_zone_append in one hipGraph replay;
  (b) track_batch alone, on a tracker of its own (what the zones add to a call is (a) - (b));
  (c) track_batch + one copy of the tracker's state to the host (what Tracker.live() costs) + the restated zone update of
      tests/zones_ref.py on the host, per stream;
  (d) the three zone launches alone on rows decoded once, between two device events, 200 triples per timing.
The box head of the stand-in network is set so that every pixel's box is 17 x 13 pixels around it, and the calls of each path see
two CUDA tensors of frames in turn, two calls each, with max_age = 0: rows are filtered out and kept, tracks are matched in one call
and retired and born in the next, so every other call has ended-inside and enter events.  (a)-(c) are timed in turn, R rounds of a >= 0.2 s window each with a host clock, every call ending in a device synchronise;
(d) once per round.  The figures are medians over the rounds, with min and max.  --kernels-only runs 20 watch_batch calls and nothing
else, for a `rocprofv3 --kernel-trace --stats` run of its own (the kernels are zone_filter_kernel, zone_update_kernel and
zone_append_kernel).
usage: python tools/gpu_zones_bench.py [--rounds R] [--kernels-only]"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import densebox_amd as D
import zones_ref
from densebox_amd import _lib, decode as DC, rows as R, synth, track, zones
from densebox_amd._lib import check, ptr, stream_ptr

H, W, B, K, T = 512, 512, 32, 10, 64
# the stand-in network's best pixels lie anywhere, the frame's border included: the polygons reach beyond the frame, and the include
# polygon is its left three quarters
SCENE = dict(lines=[((256, -32), (256, 544)), ((-32, 200), (544, 312))],
             regions=[[(-32, -32), (256, -32), (256, 256), (-32, 256)], [(280, 120), (544, 100), (340, 260), (544, 544), (270, 400)]],
             include=[[(-32, -32), (384, -32), (384, 544), (-32, 544)]])


def window(fn, seconds=0.2):
    it, t0 = 0, time.perf_counter()
    while True:
        fn()
        torch.cuda.synchronize()
        it += 1
        dt = time.perf_counter() - t0
        if dt >= seconds and it >= 3:
            return dt / it * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--kernels-only', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'gpu_zones_bench needs the MI355X'
    assert a.rounds >= 7, 'the median is taken over at least 7 alternating rounds'
    net = D.DenseBoxLMLOC(synth.vgg19_standin(0))
    synth.fill_params_(net, 11)
    with torch.no_grad():                 # every pixel's box is 17 x 13 pixels around it, as in tests/test_hip_zones.py: anchors in the image
        net.conv5_2_loc.weight.zero_()
        net.conv5_2_loc.bias.copy_(torch.tensor([2.0, 1.5, -2.0, -1.5]))
    net = net.cuda().eval()
    net.compute_dtype = 'f16'
    rs = np.random.RandomState(H + B)
    xs = [torch.from_numpy(rs.randint(0, 256, size=(B, H, W, 3)).astype(np.uint8)).cuda() for _ in range(2)]
    x, turn = xs[0], {}

    def frames(who):
        turn[who] = turn.get(who, 0) + 1
        return xs[turn[who] // 2 % 2]
    tag = '%4dx%-4d B=%-2d K=%d' % (W, H, B, K)
    tr_w, tr_t, tr_c = (track.Tracker(B, max_tracks=T, max_age=0) for _ in range(3))
    zn = zones.Zones(tr_w)
    for s in range(B):
        zn.set_stream(s, **SCENE)
    cfgs = [zones_ref.from_pixels(**SCENE)] * B
    zs = zones_ref.new_state(B, T)

    def watch():
        return net.watch_batch(frames('a'), tracker=tr_w, zones=zn, K=K, max_batch=B)

    def alone():
        return net.track_batch(frames('b'), tracker=tr_t, K=K, max_batch=B)

    def composed():
        res = net.track_batch(frames('c'), tracker=tr_c, K=K, max_batch=B)
        return res, zones_ref.update_batch(cfgs, zs, tr_c._host_state(), B)

    if a.kernels_only:
        for _ in range(20):
            watch()
        torch.cuda.synchronize()
        print('%s watch_batch calls: 20' % tag, flush=True)
        return

    # (d): rows decoded once, a tracker table as a few calls left it, and the three launches as zones._launch makes them
    with torch.no_grad():
        s, l, hm, ll = DC._forward_maps(net, x.clone())
        rows, _ = R.decode_rows(s, l, hm, ll, B, K, None, 0.4)
    tr_d = track.Tracker(B, max_tracks=T, max_age=0)
    zn_d = zones.Zones(tr_d)
    for st in range(B):
        zn_d.set_stream(st, **SCENE)
    for _ in range(3):
        zones._launch(zn_d, rows, 0)
    cfg, state, events = zn_d._buffers(x.device)
    o_lines, o_regions, o_app, _ = zn_d._layout()
    o_tab = tr_d._layout()[0]
    tb, zb = tr_d._state.data_ptr(), state.data_ptr()
    staged = torch.empty(B * T * zones.EVENTS_PER_SLOT * 32, dtype=torch.uint8, device=x.device)
    count = torch.empty(B, dtype=torch.int32, device=x.device)
    L = _lib.lib()

    def triple():
        zones._filter(zn_d, rows, 0)
        check(L.dbx_zone_update_batch(C.c_void_p(tb + o_tab), C.c_void_p(tb), ptr(cfg), C.c_void_p(zb), C.c_void_p(zb + o_lines),
                                      C.c_void_p(zb + o_regions), B, B, 0, T, 1, 0, ptr(staged), ptr(count), 1, stream_ptr()))
        check(L.dbx_zone_append(ptr(staged), ptr(count), B, T, ptr(events), zn_d.capacity, C.c_void_p(zb + o_app), stream_ptr()))

    def launches(n=200):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        triple()
        e0.record()
        for _ in range(n):
            triple()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    got = watch()
    d = np.concatenate([g[0][:, :4] for g in got])
    print('%s first call: %d rows kept of %d on the lists' % (tag, sum(len(g[1]) for g in got), sum(len(k) for _, k in net.detect_batch(xs[0], K=K, max_batch=B))),
          'box x %.1f..%.1f y %.1f..%.1f' % (d[:, [0, 2]].min(), d[:, [0, 2]].max(), d[:, [1, 3]].min(), d[:, [1, 3]].max()), flush=True)
    fns = [('(a) watch_batch (one graph replay)', watch), ('(b) track_batch alone', alone),
           ('(c) track_batch + state to the host + restated zones', composed)]
    for _, fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    per = {name: [] for name, _ in fns}
    three = []
    for _ in range(a.rounds):
        for name, fn in fns:
            per[name].append(window(fn))
        three.append(launches())
    med = {}
    for name, _ in fns:
        v = sorted(per[name])
        med[name] = v[len(v) // 2]
        print('%s %-54s %9.3f ms/call (min %.3f, max %.3f over %d alternating rounds)' % (tag, name, med[name], v[0], v[-1], a.rounds), flush=True)
    v = sorted(three)
    print('%s %-54s %9.4f ms (min %.4f, max %.4f; 200 triples between two events, host launches included)'
          % (tag, '(d) filter + zone update + zone append alone', v[len(v) // 2], v[0], v[-1]), flush=True)
    ma, mb, mc = (med[name] for name, _ in fns)
    vb = sorted(per[fns[1][0]])
    lines_, regions_ = zn.counts()
    print('%s (a) - (b) = %+.3f ms (the range of (b) is %.3f ms); (c) / (a) = %.2fx; %d events, crossings %s, region counters %s, %d live tracks'
          % (tag, ma - mb, vb[-1] - vb[0], mc / ma, int(zn._host_state()[3][2]), lines_.sum(axis=(0, 1)).tolist(),
             regions_.sum(axis=(0, 1)).tolist(), sum(len(q) for q in tr_w.live())), flush=True)


if __name__ == '__main__':
    main()
