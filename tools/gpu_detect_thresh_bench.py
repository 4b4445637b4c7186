#!/usr/bin/env python3
"""Whole-call time of detect_batch_thresh against detect_batch(K = n_b) at equal row counts (the two produce identical rows then).

DenseBoxLMLOC f16; the network's score map is replaced by a crafted one with exactly n_b pixels above 0.5 per image (distinct
scores at random places, background below 0.4), so n_b is known; loc / landmark maps are the network's.  Both calls replay their
cached hipGraph; they alternate, 7 timed calls each after 3 warm ones; median with min-max, host clock around the call (which ends
in a stream synchronise).  --trace-loop N runs N calls of each and nothing else, for a kernel trace of its own.

Usage:  python tools/gpu_detect_thresh_bench.py [--out FILE] [--trace-loop N]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import densebox_amd as D  # noqa: E402
from densebox_amd import decode as DC, synth  # noqa: E402


def crafted_scores(B, rows, cols, n, seed):
    rs = np.random.RandomState(seed)
    s = (rs.rand(B, 1, rows, cols) * 0.4).astype(np.float32)
    vals = (np.float32(0.5) + np.arange(1, n + 1, dtype=np.float32) / np.float32(8192.0)).astype(np.float32)
    for b in range(B):
        s[b].reshape(-1)[rs.choice(rows * cols, n, replace=False)] = vals[rs.permutation(n)]
    return torch.from_numpy(s).cuda()


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--trace-loop', type=int, default=0)
    ap.add_argument('--quick', action='store_true', help='skip the K = 4096 top-K calls (seconds each on the old path)')
    args = ap.parse_args()
    net = D.DenseBoxLMLOC(synth.vgg19_standin(seed=0))
    synth.fill_params_(net, 11)
    net = net.cuda().eval()
    net.compute_dtype = 'f16'
    real_maps = DC._maps
    lines = ['detect_batch_thresh vs detect_batch(K = n_b): whole call, host clock around a synchronise, ms: median [min-max] of 7;',
             'DenseBoxLMLOC f16, crafted score map with n_b pixels above 0.5 per image.  measured on one MI355X',
             '%-12s %3s %5s %8s   %-28s %-28s' % ('input', 'B', 'n_b', 'max_dets', 'thresh', 'top-K (K = n_b)')]
    cases = [(512, 512, 32, n, 1024) for n in (10, 100, 1000)] + [(1080, 1920, 8, n, 1024) for n in (10, 100, 1000)]
    cases += [(1080, 1920, 1, 4096, 4096), (1080, 1920, 8, 4096, 4096)]
    for H, W, B, n, cap in cases:
        x = synth.synth_images(B, H, W, seed=3).cuda()
        sc = crafted_scores(B, H // 4, W // 4, n, seed=n + B)
        DC._maps = lambda kind, outs, sc=sc: (sc,) + tuple(real_maps(kind, outs)[1:])
        try:
            new = lambda: net.detect_batch_thresh(x, 0.5, max_dets=cap, max_batch=B)        # noqa: E731
            old = lambda: net.detect_batch(x, K=n, max_batch=B)                            # noqa: E731
            slow_old = n > 1024 and args.quick
            r_new = new()
            if not slow_old:
                r_old = old()
                for (dn, kn), (do, ko) in zip(r_new, r_old):
                    assert dn.tobytes() == do.tobytes() and kn == ko, 'results differ'
            if args.trace_loop:
                for _ in range(args.trace_loop):
                    new()
                    if not slow_old:
                        old()
                continue
            for _ in range(2):
                new()
                if not slow_old:
                    old()
            tn, to = [], []
            for _ in range(7):
                tn += timed(new, 1)
                if not slow_old:
                    to += timed(old, 1)
            f = lambda t: '%8.3f [%7.3f - %7.3f]' % (float(np.median(t)), min(t), max(t)) if t else 'not measured'   # noqa: E731
            lines.append('%-12s %3d %5d %8d   %-28s %-28s' % ('%dx%d' % (W, H), B, n, cap, f(tn), f(to)))
            print(lines[-1], flush=True)
        finally:
            DC._maps = real_maps
            net.__dict__.pop('_detect_graphs', None)
    if args.out and not args.trace_loop:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
