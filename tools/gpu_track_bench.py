"""On-device tracking next to what a user could write before it, at 512x512 B=32 (32 camera streams, one frame each per call) on a
synthetic DenseBoxLMLOC (f16), top-K mode, K=10:
  (a) track_batch: forward, decode + NMS, dbx_track_update_batch and dbx_track_append in one hipGraph replay; dets, keep and two int32
      per list position come back;
  (b) detect_batch alone (what the tracking adds to a call is (a) - (b));
  (c) detect_batch + the NumPy restatement of tests/track_ref.py on the host, per stream.
The frames are one CUDA tensor, the same for every call.  Most boxes of the seeded stand-in network are inverted (x2 < x1) and overlap
nothing, themselves included, so in the steady state nearly every kept row starts a track and as many tracks retire per call: the
association walk, births, retirements and the append all run in every call.  The three are timed in turn, R rounds of a >= 0.2 s window
each with a host clock; every call ends in a device synchronise.  The figure is the median over the rounds, with min and max.  --kernels-only runs 20 track_batch calls and nothing else, for a `rocprofv3 --kernel-trace --stats` run of its own (the
kernels are track_update_batch_kernel and track_append_kernel).
usage: python tools/gpu_track_bench.py [--rounds R] [--kernels-only]"""
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
import track_ref
from densebox_amd import synth, track

H, W, B, K = 512, 512, 32, 10


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
    assert torch.cuda.is_available(), 'gpu_track_bench needs the MI355X'
    assert a.rounds >= 7, 'the median is taken over at least 7 alternating rounds'
    net = D.DenseBoxLMLOC(synth.vgg19_standin(0))
    synth.fill_params_(net, 11)
    net = net.cuda().eval()
    net.compute_dtype = 'f16'
    rs = np.random.RandomState(H + B)
    x = torch.from_numpy(rs.randint(0, 256, size=(B, H, W, 3)).astype(np.uint8)).cuda()
    tag = '%4dx%-4d B=%-2d K=%d' % (W, H, B, K)
    tr = track.Tracker(B, max_tracks=64)
    state = track_ref.new_state(B, 64)

    def on_device():
        return net.track_batch(x, tracker=tr, K=K, max_batch=B)

    def alone():
        return net.detect_batch(x, K=K, max_batch=B)

    def composed():
        res = net.detect_batch(x, K=K, max_batch=B)
        return res, track_ref.update_batch(state, res)

    if a.kernels_only:
        for _ in range(20):
            on_device()
        torch.cuda.synchronize()
        print('%s track_batch calls: 20' % tag, flush=True)
        return
    got = on_device()
    res, want = composed()
    assert all(g[2].tolist() == w[0].tolist() and g[3].tolist() == w[2].tolist() for g, w in zip(got, want)), 'the two paths disagree'
    kept = sum(len(k) for _, k in res)
    fns = [('(a) track_batch (one graph replay)', on_device), ('(b) detect_batch alone', alone),
           ('(c) detect_batch + NumPy tracking on the host', composed)]
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
        print('%s %-48s %9.3f ms/call (min %.3f, max %.3f over %d alternating rounds)' % (tag, name, med[name], v[0], v[-1], a.rounds), flush=True)
    ma, mb, mc = (med[name] for name, _ in fns)
    print('%s (a) - (b) = %+.3f ms; (c) / (a) = %.2fx; %d kept rows per call, %d live tracks'
          % (tag, ma - mb, mc / ma, kept, sum(len(l) for l in tr.live())), flush=True)


if __name__ == '__main__':
    main()
