"""Batched pad + bicubic resize throughput and what it buys detect on mixed-size frames.

Default: (a) resize.pad_resize_batch of 32 frames 1080 x 1920 -> 720 and -> 512 and resize.crop_resize_batch of 320 windows -> 240 x 240,
each ONE launch, timed with a host clock around a device synchronise; (b) the whole call: detect_batch_resized on 32 frames of four
interleaved sizes next to detect_batch on the same list (grouped by shape: one forward and one graph per size), alternating within
this process, median of R.  The two do different work (one resizes, one does not): the pair is reported, not compared as a speed-up.
--kernels-only: 20 calls of each resize workload and nothing else, for a `rocprofv3 --kernel-trace --stats` run; the bytes per call
(source crop bytes + destination bytes, from the shapes) are printed so kernel time turns into bytes / s.
--trace-call: warm-up plus 5 detect_batch_resized calls on the mixed list, for a kernel trace that shows the resize launch next to the
forward's convolution kernels.
usage: python tools/gpu_resize_bench.py [--repeats R] [--kernels-only | --trace-call]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import densebox_amd as D
from densebox_amd import resize, synth

MIXED = [(480, 640), (608, 800), (720, 1280), (1088, 1920)]        # four interleaved frame sizes (multiples of 16: detect_batch takes them as they are)


def timed_once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def resize_workloads():
    rs = np.random.RandomState(8)
    frames = list(torch.from_numpy(rs.randint(0, 256, size=(32, 1080, 1920, 3)).astype(np.uint8)).cuda().unbind(0))
    windows = []
    for _ in frames:                                       # 10 windows per frame, 150..600 pixels wide, 4:3 .. 1:1
        ws = []
        for _ in range(10):
            w = int(rs.randint(150, 600))
            h = int(w * rs.uniform(0.75, 1.0))
            x0, y0 = int(rs.randint(0, 1920 - w)), int(rs.randint(0, 1080 - h))
            ws.append((x0, y0, x0 + w, y0 + h))
        windows.append(ws)
    full = 32 * 1080 * 1920 * 3
    crop = sum((x1 - x0) * (y1 - y0) * 3 for ws in windows for (x0, y0, x1, y1) in ws)
    return [('pad_resize 32 x 1080x1920 -> 720', lambda: resize.pad_resize_batch(frames, 720), full + 32 * 720 * 720 * 3),
            ('pad_resize 32 x 1080x1920 -> 512', lambda: resize.pad_resize_batch(frames, 512), full + 32 * 512 * 512 * 3),
            ('crop_resize 320 windows -> 240x240', lambda: resize.crop_resize_batch(frames, windows, (240, 240)), crop + 320 * 240 * 240 * 3)]


def mixed_frames():
    rs = np.random.RandomState(9)
    return [torch.from_numpy(rs.randint(0, 256, size=MIXED[i % 4] + (3,)).astype(np.uint8)).cuda() for i in range(32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--trace-call', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'gpu_resize_bench needs the MI355X'
    if not a.trace_call:
        for name, fn, nbytes in resize_workloads():
            if a.kernels_only:
                for _ in range(20):
                    fn()
                torch.cuda.synchronize()
                print('%-36s calls: 20, %d bytes per call (source crops + destination)' % (name, nbytes), flush=True)
                continue
            for _ in range(3):
                fn()
            per = [timed_once(fn) for _ in range(max(a.repeats, 5) * 4)]
            print('%-36s %8.3f ms/call (min %.3f, max %.3f over %d calls)  %d bytes/call'
                  % (name, median(per), min(per), max(per), len(per), nbytes), flush=True)
        torch.cuda.empty_cache()
        if a.kernels_only:
            return
    net = D.DenseBoxLMLOC(synth.vgg19_standin(0))
    synth.fill_params_(net, 11)
    net = net.cuda().eval()
    net.compute_dtype = 'f16'
    frames = mixed_frames()

    def resized():
        return net.detect_batch_resized(frames, size=720, K=10)

    def grouped():
        return net.detect_batch(frames, K=10)
    if a.trace_call:
        for _ in range(3 + 5):
            resized()
        torch.cuda.synchronize()
        print('detect_batch_resized: 3 warm-up + 5 calls on 32 frames of sizes %s -> 720' % (MIXED,), flush=True)
        return
    for _ in range(2):                                     # warm both: plans, graphs (one for resized, four for grouped)
        resized()
        grouped()
    tr, tg = [], []
    for _ in range(a.repeats):                             # alternating within one process
        tr.append(timed_once(resized))
        tg.append(timed_once(grouped))
    print('32 frames of sizes %s, DenseBoxLMLOC f16, K=10' % (MIXED,))
    print('detect_batch_resized (one resize launch + one 32 x 720 x 720 forward, 1 graph)  %8.3f ms/call (min %.3f, max %.3f over %d)'
          % (median(tr), min(tr), max(tr), len(tr)))
    print('detect_batch grouped by shape (four 8-frame forwards at full size, 4 graphs)     %8.3f ms/call (min %.3f, max %.3f over %d)'
          % (median(tg), min(tg), max(tg), len(tg)), flush=True)


if __name__ == '__main__':
    main()
