"""Pyramid detection against the composition a user could write before it existed.

DenseBoxLMLOC, f16, K = 10, sizes (480, 720, 1080), three workloads of 32 frames: (a) device-resident 1080 x 1920 frames, (b) the same
frames as host numpy arrays, (c) the list of four interleaved frame sizes of tools/gpu_resize_bench.py (device-resident).  For each,
after warm-up, net.detect_pyramid(...) and the composition -- one detect_batch_resized call per size, a host concatenate, decode.NMS per
frame -- alternate within this process; median, min and max of R timings each (host clock around a device synchronise).  A pair whose
min-max ranges overlap is reported as "no difference shown".  Writes the lines to --out as well (default profiles/r09_pyramid.txt).
--trace-call: warm-up plus 5 detect_pyramid calls of workload (a) and nothing else, for a `rocprofv3 --kernel-trace --stats` run that
shows the resize and the merge launches next to the forwards' convolution kernels.
usage: python tools/gpu_pyramid_bench.py [--repeats R] [--out FILE] [--trace-call]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import densebox_amd as D
from densebox_amd import decode, synth

SIZES = (480, 720, 1080)
MIXED = [(480, 640), (608, 800), (720, 1280), (1088, 1920)]


def timed_once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def composition(net, frames):
    per = [net.detect_batch_resized(frames, size=s, K=10) for s in SIZES]
    out = []
    for i in range(len(per[0])):
        d = np.concatenate([p[i][0] for p in per], axis=0)
        out.append((d, decode.NMS(d, 0.4)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r09_pyramid.txt'))
    ap.add_argument('--trace-call', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'gpu_pyramid_bench needs the MI355X'
    net = D.DenseBoxLMLOC(synth.vgg19_standin(0))
    synth.fill_params_(net, 11)
    net = net.cuda().eval()
    net.compute_dtype = 'f16'
    rs = np.random.RandomState(8)
    host = [rs.randint(0, 256, size=(1080, 1920, 3)).astype(np.uint8) for _ in range(32)]
    dev = [torch.from_numpy(f).cuda() for f in host]
    if a.trace_call:
        for _ in range(3 + 5):
            net.detect_pyramid(dev, sizes=SIZES, K=10)
        torch.cuda.synchronize()
        print('detect_pyramid: 3 warm-up + 5 calls on 32 device-resident 1080 x 1920 frames, sizes %s' % (SIZES,), flush=True)
        return
    rs = np.random.RandomState(9)
    mixed = [torch.from_numpy(rs.randint(0, 256, size=MIXED[i % 4] + (3,)).astype(np.uint8)).cuda() for i in range(32)]
    lines = ['DenseBoxLMLOC f16, K=10, sizes %s, 32 frames per call; one MI355X, median (min .. max) of %d alternating timings, ms per call'
             % (SIZES, max(a.repeats, 5))]
    for name, frames in (('(a) 32 device-resident 1080x1920 frames', dev), ('(b) the same frames as host numpy arrays', host),
                         ('(c) 32 device-resident frames of sizes %s' % (MIXED,), mixed)):
        for _ in range(2):                                   # warm both: plans, three 'level' graphs and three 'batch' graphs
            got = net.detect_pyramid(frames, sizes=SIZES, K=10)
            ref = composition(net, frames)
        same = all(np.array_equal(g[0], r[0]) and g[1] == r[1] for g, r in zip(got, ref))
        tp, tc = [], []
        for _ in range(max(a.repeats, 5)):                   # alternating within one process
            tp.append(timed_once(lambda: net.detect_pyramid(frames, sizes=SIZES, K=10)))
            tc.append(timed_once(lambda: composition(net, frames)))
        overlap = min(tc) <= max(tp) and min(tp) <= max(tc)
        verdict = 'no difference shown (the ranges overlap)' if overlap else ('detect_pyramid %.1f %% %s' % (
            abs(1.0 - median(tp) / median(tc)) * 100.0, 'less' if median(tp) < median(tc) else 'MORE'))
        lines += [name,
                  '    detect_pyramid                                             %9.3f (%.3f .. %.3f)' % (median(tp), min(tp), max(tp)),
                  '    3 x detect_batch_resized + concatenate + 32 x decode.NMS   %9.3f (%.3f .. %.3f)' % (median(tc), min(tc), max(tc)),
                  '    %s; results %s' % (verdict, 'identical' if same else 'DIFFER')]
        print('\n'.join(lines[-4:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
