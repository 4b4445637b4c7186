"""Fixed-size plate crops next to their yardsticks, at 512x512 B=32 K=10 on a synthetic DenseBoxLMLOC (f16), crop size (94, 24):
  (a) detect_plate_crops: forward, decode and the crop launch in one hipGraph replay;
  (b) detect_batch alone;
  (c) the composition without it: detect_batch, then per kept row get_perspective_matrix(q, plate_rectangle(size)) on the host and one
      warp_perspective(frame, M, size) launch, stacked per frame.
The frames are one CUDA tensor.  The three are timed in turn, R rounds of a >= 0.2 s window each with a host clock; every call ends
in a device synchronise.  The figure is the median over the rounds, with min and max.  --kernels-only runs 20 detect_plate_crops calls
and nothing else, for a `rocprofv3 --kernel-trace --stats` run of its own (the crop kernel is plate_crops_batch_u8_kernel<3>).
usage: python tools/gpu_plate_crops_bench.py [--rounds R] [--kernels-only]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import densebox_amd as D
from densebox_amd import rectify, synth

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
    assert torch.cuda.is_available(), 'gpu_plate_crops_bench needs the MI355X'
    assert a.rounds >= 7, 'the median is taken over at least 7 alternating rounds'
    net = D.DenseBoxLMLOC(synth.vgg19_standin(0))
    synth.fill_params_(net, 11)
    net = net.cuda().eval()
    net.compute_dtype = 'f16'
    rs = np.random.RandomState(H + B)
    x = torch.from_numpy(rs.randint(0, 256, size=(B, H, W, 3)).astype(np.uint8)).cuda()
    frames = list(x.unbind(0))
    rect = rectify.plate_rectangle(SIZE)
    tag = '%4dx%-4d B=%-2d K=%d size=%dx%d' % (W, H, B, K, SIZE[0], SIZE[1])

    def crops():
        return net.detect_plate_crops(x, size=SIZE, K=K, max_batch=B)

    def det():
        return net.detect_batch(x, K=K, max_batch=B)

    def composed():
        out = []
        for f, (d, keep) in zip(frames, det()):
            plates = []
            for k in keep:
                try:
                    M = rectify.get_perspective_matrix(d[k, 5:13].reshape(4, 2), rect)
                    plates.append(rectify.warp_perspective(f, M, SIZE))
                except RuntimeError:                           # degenerate corners / singular map: no crop for this row
                    pass
            out.append(torch.stack(plates) if plates else None)
        return out

    if a.kernels_only:
        for _ in range(20):
            crops()
        torch.cuda.synchronize()
        print('%s detect_plate_crops calls: 20, %d slots and %d output bytes per call' % (tag, B * K, B * K * SIZE[0] * SIZE[1] * 3), flush=True)
        return
    got = crops()
    rows, ok = sum(len(keep) for _, keep, _, _ in got), sum(int(o.sum()) for _, _, _, o in got)
    del got
    fns = [('(a) detect_plate_crops (one graph replay)', crops), ('(b) detect_batch alone', det),
           ('(c) detect_batch + host solve + warp_perspective per row', composed)]
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
    print('%s (a) - (b) = %+.3f ms (%+.1f%%); (c) / (a) = %.2fx; %d kept rows per call, %d of them ok'
          % (tag, ma - mb, (ma - mb) / mb * 100, mc / ma, rows, ok), flush=True)


if __name__ == '__main__':
    main()
