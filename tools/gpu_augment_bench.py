"""What the on-device patch augmentation costs next to the sampler it follows, next to the host stage it replaces, and next to the
training step it feeds.

32 device-resident frames of 1080 x 1920 with 8 plates each, n = 64 patches per batch (96 candidates, a tenth of them negatives):
(a) data.PatchSampler(augment=data.Augment()).next_batch() -- four launches and a 4-byte read -- against next_batch() without an
    augmenter in the same process;
(b) the same against the host stage a user would write without it: the un-augmented batch copied to the host, the NumPy restatement
    (tests/aug_ref.py, the same records) per patch, the result and the label rows uploaded;
(c) a DenseBoxLMLOC f16 training step (forward, loss, backward, SGD) fed by each of the two samplers.
Host clock around a device synchronise, the sides of a comparison alternating within this process, median and range of R timings.
--kernels-only: 20 augmented next_batch() calls and nothing else, for a `rocprofv3 --kernel-trace --stats` run.
usage: python tools/gpu_augment_bench.py [--repeats R] [--kernels-only] [--no-step]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import aug_ref as A
import densebox_amd as D
from densebox_amd import data, labels as LB, synth
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
    print('%-86s %9.3f ms median (min %.3f, max %.3f over %d)' % (name, s[len(s) // 2], s[0], s[-1], len(s)), flush=True)


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
    assert torch.cuda.is_available(), 'gpu_augment_bench needs the MI355X'
    frames, plates = scene()
    aug = data.Augment(seed=SEED)
    augmented = data.PatchSampler(frames, plates, N, oversample=1.5, neg_frac=0.1, seed=SEED, augment=aug)
    if a.kernels_only:
        for _ in range(20):
            augmented.next_batch()
        torch.cuda.synchronize()
        print('PatchSampler(augment=Augment()).next_batch: 20 calls, %d patches of 240 x 240 x 3 each' % N, flush=True)
        return
    plain = data.PatchSampler(frames, plates, N, oversample=1.5, neg_frac=0.1, seed=SEED)
    bank = aug.curves()
    f = aug.cfg()
    cfg = {k: (tuple(f.kind_w) if k == 'kind_w' else getattr(f, k)) for k in A.CFG_DEFAULT}
    host_counter = [0]

    def on_host():
        patches, _, _, _, count = plain.next_batch()
        raw, rows = patches.cpu().numpy(), plain.plan.labels_i32.cpu().numpy()
        p = A.plan(cfg, rows, count, seed=SEED, counter=host_counter[0])
        host_counter[0] += 1
        out = np.stack([A.augment(raw[s], p['params'][s], bank) for s in range(count)])
        lab = np.concatenate([p['bbox'], p['vertices'], p['label']], axis=1)
        return torch.from_numpy(out).cuda(), torch.from_numpy(lab).cuda()

    for _ in range(3):
        augmented.next_batch()
        plain.next_batch()
    on_host()
    ta, tp, th = [], [], []
    for _ in range(a.repeats):
        ta.append(timed_once(augmented.next_batch))
        tp.append(timed_once(plain.next_batch))
        th.append(timed_once(on_host))
    print('%d frames of %d x %d on the device, %d patches per batch' % (FRAMES, H, W, N))
    report('PatchSampler(augment=Augment()).next_batch (plan + cut + aug plan + augment, 4-byte read)', ta)
    report('PatchSampler.next_batch without an augmenter', tp)
    report('next_batch + batch to the host + NumPy restatement + upload', th)
    kinds = np.bincount(augmented.aug_params[:, 1].cpu().numpy(), minlength=4).tolist()
    print('last batch: %d flipped, %d refused, blur kinds none/3x3/5x5/box %s, %d with a curve, %d with noise'
          % (int((augmented.aug_params[:, 0] == 1).sum()), int((augmented.aug_params[:, 0] == 2).sum()), kinds,
             int((augmented.aug_params[:, 6] >= 0).sum()), int((augmented.aug_params[:, 7] > 0).sum())), flush=True)
    # the device side alone: launch() of each sampler captured into a graph (no Python between the launches), and the two new launches
    # between a pair of events, 20 in a row
    import gc
    graphs = []
    for smp in (augmented, plain):
        g = torch.cuda.CUDAGraph()
        gc.collect()
        with torch.cuda.graph(g):
            smp.launch()
        graphs.append(g)
    for g in graphs:
        g.replay()
    tga, tgp = [], []
    for _ in range(a.repeats):
        tga.append(timed_once(graphs[0].replay))
        tgp.append(timed_once(graphs[1].replay))
    report('one graph replay of launch() with the augmenter (4 launches + the tally add)', tga)
    report('one graph replay of launch() without it (2 launches + the tally add)', tgp)

    def events(fn, reps=20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    s_ = augmented
    tk = [events(lambda: data.apply_augment(s_.patches, s_.aug.params, s_.plan.count, s_.curves, s_.aug_patches)) for _ in range(a.repeats)]
    tq = [events(lambda: data.plan_augment(s_.plan.labels_i32, s_.plan.count, s_.aug_cfg, state=s_.aug_state, out=s_.aug)) for _ in range(a.repeats)]
    tc = [events(lambda: s_.aug_patches.copy_(s_.patches)) for _ in range(a.repeats)]
    report('dbx_patch_augment alone, events around 20 launches (the last batch\'s records)', tk)
    report('dbx_patch_aug_plan alone, events around 20 launches', tq)
    report('copy_ of the same 64 patches, events around 20', tc)
    # what each op costs: all 64 slots given the same injected record
    for name, rec in (('identity (the copy path)', A.record()), ('flip', A.record(flags=1)), ('saturation', A.record(sat=300)),
                      ('tone (gain, contrast, brightness, curve)', A.record(contrast=300, brightness=9, curve=1, gain=(250, 260, 270))),
                      ('noise', A.record(noise_amp=12, key=A.KEY)), ('binomial 3 x 3', A.record(blur=1)), ('binomial 5 x 5', A.record(blur=2)),
                      ('box 9', A.record(blur=3, box_len=9)), ('all ops, 5 x 5', dict(A.CASES)['all_binomial5'])):
        recs = torch.from_numpy(np.stack([A.to_row(rec)] * N)).cuda()
        t = [events(lambda: data.apply_augment(s_.patches, recs, s_.plan.count, s_.curves, s_.aug_patches)) for _ in range(a.repeats)]
        report('dbx_patch_augment, every slot: %s' % name, t)
    if a.no_step:
        return
    torch.manual_seed(0)
    net = D.DenseBoxLMLOC(synth.vgg19_standin(seed=0))
    synth.fill_params_(net, 11)
    net = net.cuda().train()
    net.compute_dtype = 'f16'
    dp = DataParallel(net, SGD(net.parameters(), lr=1e-9, momentum=0.9, weight_decay=5e-8))
    rs = np.random.RandomState(1234)

    def step(sampler):
        x_, bbox_, vert_, lab_, _ = sampler.next_batch()
        p = dp.global_positive_num(bbox_, lab_)
        _, half = LB.neg_counts(p, N)
        rn = np.stack([rs.choice(3600, half, replace=False) for _ in range(N)]) if half else np.zeros((N, 0), np.int64)
        lrn = rs.randint(0, 3600, size=(4, N, 1))
        return dp.step(x_, bbox_, vert_, lab_, rand_neg_indices=rn, lm_rand_neg_indices=lrn, positive_num_global=p)

    for _ in range(6):
        step(plain)
        step(augmented)
    tr, tg = [], []
    for _ in range(a.repeats):
        tr.append(timed_once(lambda: step(plain)))
        tg.append(timed_once(lambda: step(augmented)))
    report('training step, batch %d f16, fed by PatchSampler.next_batch' % N, tr)
    report('training step, batch %d f16, fed by PatchSampler(augment=Augment()).next_batch' % N, tg)


if __name__ == '__main__':
    main()
