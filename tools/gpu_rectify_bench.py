"""Plate rectification throughput: the per-plate loop of rectify.perspective_transform on device frames, ONE
rectify.perspective_transform_batch call over the same quads, and one detect_plates call next to detect_batch alone, timed in the
same process for three workloads (512x512 B=32 K=10 'plate' and 'canvas', 1920x1080 B=8 K=10 'canvas').

Every row is warmed, then timed as R repeats of a >= 0.3 s window with a host clock; each call ends in a device synchronise (the loop's
single-plate calls end in their own blocking download; the batch call's arena stays on the device).  The spread is min / median / max
over the repeats.  The loop and batch rows warp synthetic plate quads (K per frame); detect_plates warps what a synthetic
DenseBoxLMLOC (f16) keeps.  Output bytes per batch call are printed so a kernel trace (--kernels-only: the batch calls alone, for a
`rocprofv3 --kernel-trace --stats` run) turns into bytes / kernel time.
usage: python tools/gpu_rectify_bench.py [--repeats R] [--kernels-only]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import densebox_amd as D
from densebox_amd import rectify, synth

WORKLOADS = [(512, 512, 32, 10, 'plate'), (512, 512, 32, 10, 'canvas'), (1080, 1920, 8, 10, 'canvas')]


def quads_for(rs, h, w, n):
    out = []
    for _ in range(n):
        cx, cy = rs.uniform(0.2, 0.8) * w, rs.uniform(0.2, 0.8) * h
        hw, hh = rs.uniform(0.06, 0.15) * w, rs.uniform(0.03, 0.08) * h
        c = np.array([[cx - hw, cy - hh], [cx + hw, cy - hh * 0.9], [cx + hw * 0.95, cy + hh], [cx - hw * 1.05, cy + hh * 1.1]])
        out.append((c + rs.uniform(-0.01, 0.01, size=(4, 2)) * np.array([w, h])).tolist())
    return out


def timed(fn, repeats, window=0.3):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(repeats):
        it, t0 = 0, time.perf_counter()
        while True:
            fn()
            torch.cuda.synchronize()
            it += 1
            dt = time.perf_counter() - t0
            if dt >= window and it >= 3:
                break
        per.append(dt / it * 1e3)
    per.sort()
    return per[0], per[len(per) // 2], per[-1]


def out_bytes(frames, quads, region):
    n = 0
    for f, qs in zip(frames, quads):
        h, w, c = f.shape
        for q in qs:
            job = rectify._rect_job(q, h, w, region)
            if job is not None:
                n += job[5] * job[6] * c
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--kernels-only', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'gpu_rectify_bench needs the MI355X'
    net = D.DenseBoxLMLOC(synth.vgg19_standin(0))
    synth.fill_params_(net, 11)
    net = net.cuda().eval()
    net.compute_dtype = 'f16'
    for (h, w, B, K, region) in WORKLOADS:
        rs = np.random.RandomState(h + B)
        x = torch.from_numpy(rs.randint(0, 256, size=(B, h, w, 3)).astype(np.uint8)).cuda()
        frames = list(x.unbind(0))
        quads = [quads_for(rs, h, w, K) for _ in range(B)]
        nplates = B * K
        nbytes = out_bytes(frames, quads, region)
        tag = '%4dx%-4d B=%-2d K=%d %-6s' % (w, h, B, K, region)
        if a.kernels_only:
            for _ in range(20):
                rectify.perspective_transform_batch(frames, quads, region=region)
            torch.cuda.synchronize()
            print('%s batch calls: 20, %d plates and %d output bytes per call' % (tag, nplates, nbytes), flush=True)
            continue

        def loop():
            res = []
            for f, qs in zip(frames, quads):
                for q in qs:
                    p = rectify.perspective_transform(f, q)
                    if region == 'plate':
                        x0, y0, oh, ow = rectify.plate_window(rectify.dst_rectangle(q), p.shape[0], p.shape[1])
                        p = p[y0:y0 + oh, x0:x0 + ow]
                    res.append(p)
            return res

        def batch():
            return rectify.perspective_transform_batch(frames, quads, region=region)

        def det():
            return net.detect_batch(x, K=K, max_batch=B)

        def plates():
            return net.detect_plates(x, K=K, max_batch=B, region=region)
        got = plates()
        kept = sum(p is not None for _, _, ps in got for p in ps)
        kept_bytes = sum(p.numel() for _, _, ps in got for p in ps if p is not None)
        rows_seen = sum(len(keep) for _, keep, _ in got)
        del got
        rows = [('per-plate loop of perspective_transform', loop, nplates),
                ('perspective_transform_batch (one call)', batch, nplates),
                ('detect_batch alone', det, 0),
                ('detect_plates (detect_batch + one warp)', plates, kept)]
        res = {}
        for name, fn, n in rows:
            lo, med, hi = timed(fn, a.repeats)
            res[name] = med
            print('%s %-42s %9.3f ms/call (min %.3f, max %.3f over %d repeats)  %d plates'
                  % (tag, name, med, lo, hi, a.repeats, n), flush=True)
        print('%s batch / loop speed-up %.2fx; detect_plates - detect_batch = %.3f ms; batch output %d bytes/call; detect_plates warps '
              '%d kept rows into %d plates, %d bytes/call'
              % (tag, res[rows[0][0]] / res[rows[1][0]], res[rows[3][0]] - res[rows[2][0]], nbytes, rows_seen, kept, kept_bytes), flush=True)
        del x, frames
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
