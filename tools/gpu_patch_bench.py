"""What the on-device patch sampler costs next to the composition that existed before it, and next to the training step it feeds.

32 device-resident frames of 1080 x 1920 with 8 plates each, n = 64 patches per batch (96 candidates, a tenth of them negatives):
(a) data.PatchSampler.next_batch() -- two launches and a 4-byte read -- against the plan made on the host by the Python restatement
    (tests/patch_ref.py, the same hash, so both cut the same patches) + resize.crop_resize_batch + one upload of the label rows;
(b) a DenseBoxLMLOC f16 training step (forward, loss, backward, SGD) fed by next_batch() against the same step on one resident
    synthetic batch.
Host clock around a device synchronise, the two sides of a pair alternating within this process, median and range of R timings.
--kernels-only: 20 next_batch() calls and nothing else, for a `rocprofv3 --kernel-trace --stats` run.
usage: python tools/gpu_patch_bench.py [--repeats R] [--kernels-only] [--no-step]"""
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
import patch_ref as R
from densebox_amd import data, labels as LB, resize, synth
from densebox_amd.dist import DataParallel
from densebox_amd.optim import SGD

N, FRAMES, H, W, SEED = 64, 32, 1080, 1920, 17


def timed_once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def report(name, v):
    s = sorted(v)
    print('%-78s %9.3f ms median (min %.3f, max %.3f over %d)' % (name, s[len(s) // 2], s[0], s[-1], len(s)), flush=True)


def scene():
    rs = np.random.RandomState(8)
    frames = list(torch.from_numpy(rs.randint(0, 256, size=(FRAMES, H, W, 3)).astype(np.uint8)).cuda().unbind(0))
    plates = []
    for _ in range(FRAMES):
        ps = []
        for _ in range(8):
            w, h = int(rs.randint(40, 200)), int(rs.randint(16, 80))
            x, y = int(rs.randint(0, W - w)), int(rs.randint(0, H - h))
            ps.append([x, y, x + w, y + int(rs.randint(0, 4)), x + w, y + h, x + int(rs.randint(0, 4)), y + h])
        plates.append(ps)
    return frames, plates


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--no-step', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'gpu_patch_bench needs the MI355X'
    frames, plates = scene()
    sampler = data.PatchSampler(frames, plates, N, oversample=1.5, neg_frac=0.1, seed=SEED)
    if a.kernels_only:
        for _ in range(20):
            sampler.next_batch()
        torch.cuda.synchronize()
        print('PatchSampler.next_batch: 20 calls, %d candidates -> %d patches of 240 x 240 x 3 each' % (sampler.M, N), flush=True)
        return
    rows, plate0 = data.plate_tables(plates, FRAMES)
    sizes = [(H, W)] * FRAMES
    host_counter = [0]

    def composed():
        p = R.plan(sizes, rows, plate0, sampler.M, N, seed=SEED, counter=host_counter[0], neg_frac=0.1)
        host_counter[0] += 1
        order = [s for f in range(FRAMES) for s in range(p['count']) if p['frames'][s] == f]
        windows = [[tuple(int(v) for v in p['windows'][s]) for s in range(p['count']) if p['frames'][s] == f] for f in range(FRAMES)]
        patches = resize.crop_resize_batch(frames, windows)
        lab = torch.from_numpy(np.concatenate([p['bbox'][order], p['vertices'][order], p['label'][order]], axis=1)).cuda()
        return patches, lab

    for _ in range(3):
        sampler.next_batch()
        composed()
    ts, tc = [], []
    for _ in range(a.repeats):
        ts.append(timed_once(sampler.next_batch))
        tc.append(timed_once(composed))
    print('%d frames of %d x %d on the device, %d candidates -> %d patches per batch' % (FRAMES, H, W, sampler.M, N))
    report('PatchSampler.next_batch (plan + cut on the device, 4-byte read)', ts)
    report('host plan (Python restatement) + crop_resize_batch + label upload', tc)
    print('status tally so far: %s' % sampler.status_tally(), flush=True)
    if a.no_step:
        return
    torch.manual_seed(0)
    net = D.DenseBoxLMLOC(synth.vgg19_standin(seed=0))
    synth.fill_params_(net, 11)
    net = net.cuda().train()
    net.compute_dtype = 'f16'
    dp = DataParallel(net, SGD(net.parameters(), lr=1e-9, momentum=0.9, weight_decay=5e-8))
    x, bbox, vert, lab = synth.synth_batch(N, seed=100, neg_frac=0.1)
    x = x.cuda()
    rs = np.random.RandomState(1234)

    def step(x_, bbox_, vert_, lab_):
        p = dp.global_positive_num(bbox_, lab_)
        _, half = LB.neg_counts(p, N)
        rn = np.stack([rs.choice(3600, half, replace=False) for _ in range(N)]) if half else np.zeros((N, 0), np.int64)
        lrn = rs.randint(0, 3600, size=(4, N, 1))
        return dp.step(x_, bbox_, vert_, lab_, rand_neg_indices=rn, lm_rand_neg_indices=lrn, positive_num_global=p)

    def resident():
        return step(x, bbox, vert, lab)

    def sampled():
        patches, b, v, l, _ = sampler.next_batch()
        return step(patches, b, v, l)

    for _ in range(6):
        resident()
        sampled()
    tr, tp = [], []
    for _ in range(a.repeats):
        tr.append(timed_once(resident))
        tp.append(timed_once(sampled))
    report('training step, batch %d f16, on one resident synthetic batch' % N, tr)
    report('training step, batch %d f16, fed by PatchSampler.next_batch (uint8 patches)' % N, tp)


if __name__ == '__main__':
    main()
