"""The best-shot gallery next to what a user could write before it, at 512x512 B=32 (32 camera streams, one frame each per call) on a
synthetic DenseBoxLMLOC (f16), K=10, crops of 94 x 24:
  (a) track_plate_crops: forward, decode + NMS, dbx_plate_crops_batch, dbx_track_update_batch, dbx_track_gallery_update and
      dbx_track_append in one hipGraph replay; dets, keep and two int32 per list position come back, no crop does;
  (b) track_batch alone (what the crops and the gallery add to a call is (a) - (b));
  (c) the composition a user can write today: detect_plate_crops with every crop of every frame copied to the host, track.update_batch
      on the host results, and a Python dictionary of the best crop per (stream, track id), ranked by the NumPy focus measure of
      tests/gallery_ref.py.
The frames are one CUDA tensor for (a) and (b) and the same frames as one host tensor for (c)'s crops to come back to the host; they
are the same for every call.  Most boxes of the seeded stand-in network are inverted (x2 < x1) and overlap nothing, themselves included,
so in the steady state nearly every kept row starts a track and as many tracks retire per call: adoption, the first shot and the move
into the arena run in every call; replacements are rare.  The three are timed in turn, R rounds of a >= 0.2 s window each with a host
clock; every call ends in a device synchronise.  The figure is the median over the rounds, with min and max.  --kernels-only runs 20
track_plate_crops calls and nothing else, for a kernel trace of its own (the kernel is track_gallery_update_kernel).
usage: python tools/gpu_gallery_bench.py [--rounds R] [--kernels-only]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import densebox_amd as D
import gallery_ref
from densebox_amd import gallery, synth, track

H, W, B, K, SIZE = 512, 512, 32, 10, (94, 24)


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
    assert torch.cuda.is_available(), 'gpu_gallery_bench needs the MI355X'
    assert a.rounds >= 7, 'the median is taken over at least 7 alternating rounds'
    net = D.DenseBoxLMLOC(synth.vgg19_standin(0))
    synth.fill_params_(net, 11)
    net = net.cuda().eval()
    net.compute_dtype = 'f16'
    rs = np.random.RandomState(H + B)
    host = torch.from_numpy(rs.randint(0, 256, size=(B, H, W, 3)).astype(np.uint8))
    x = host.cuda()
    tag = '%4dx%-4d B=%-2d K=%d %dx%d' % (W, H, B, K, SIZE[0], SIZE[1])
    tr_a = track.Tracker(B, max_tracks=64)
    gal = gallery.PlateGallery(tr_a, size=SIZE, capacity=1 << 16)
    tr_b = track.Tracker(B, max_tracks=64)
    tr_c = track.Tracker(B, max_tracks=64)
    best = {}

    def on_device():
        return net.track_plate_crops(x, tracker=tr_a, gallery=gal, K=K, max_batch=B)

    def alone():
        return net.track_batch(x, tracker=tr_b, K=K, max_batch=B)

    def composed():
        res = net.detect_plate_crops(host, size=SIZE, K=K, max_batch=B)                # crops come back as CPU tensors
        ids = track.update_batch([d for d, _, _, _ in res], [k for _, k, _, _ in res], tracker=tr_c)
        for s, ((_, keep, crops, ok), (tid, _)) in enumerate(zip(res, ids)):
            crops = crops.numpy()
            sharp = gallery_ref.sharpness(crops) if len(keep) else ()
            for j in range(len(keep)):
                if tid[j] >= 0 and ok[j]:
                    was = best.get((s, int(tid[j])))
                    if was is None or sharp[j] > was[0]:
                        best[(s, int(tid[j]))] = (int(sharp[j]), crops[j].copy())
        return res, ids

    if a.kernels_only:
        for _ in range(20):
            on_device()
        torch.cuda.synchronize()
        print('%s track_plate_crops calls: 20' % tag, flush=True)
        return
    got = on_device()
    res, ids = composed()
    assert all(g[2].tolist() == i[0].tolist() and g[3].tolist() == i[1].tolist() for g, i in zip(got, ids)), 'the two paths disagree'
    live = {(s, int(g['id'])): (int(g['sharpness']), c) for s, (shots, crops) in enumerate(gal.live()) for g, c in zip(shots, crops)
            if g['shots'] > 0}
    assert live.keys() == best.keys() and all(live[k][0] == best[k][0] and np.array_equal(live[k][1], best[k][1]) for k in live), \
        'the gallery and the host dictionary disagree'
    kept = sum(len(k) for _, k, _, _ in res)
    fns = [('(a) track_plate_crops (one graph replay)', on_device), ('(b) track_batch alone', alone),
           ('(c) detect_plate_crops to the host + update_batch + dict', composed)]
    for _, fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    per = {name: [] for name, _ in fns}
    for _ in range(a.rounds):
        for name, fn in fns:
            per[name].append(window(fn))
    med = {}
    for name, _ in fns:
        v = sorted(per[name])
        med[name] = v[len(v) // 2]
        print('%s %-58s %9.3f ms/call (min %.3f, max %.3f over %d alternating rounds)' % (tag, name, med[name], v[0], v[-1], a.rounds), flush=True)
    ma, mb, mc = (med[name] for name, _ in fns)
    print('%s (a) - (b) = %+.3f ms; (c) / (a) = %.2fx; %d kept rows per call, %d live shots, counters (ended, stored, lost, dropped) = %s'
          % (tag, ma - mb, mc / ma, kept, len(live), gal.counters()), flush=True)


if __name__ == '__main__':
    main()
