"""What the on-device patch warp costs next to the sampler it follows, next to the host stage it replaces, and next to the training
step it feeds.

32 device-resident frames of 1080 x 1920 with 8 plates each, n = 64 patches per batch (96 candidates, a tenth of them negatives):
(a) data.PatchSampler(warp=data.Warp()).next_batch() -- four launches and a 4-byte read -- against next_batch() with warp=None, which
    makes exactly the launches the sampler made before it had a warper, in the same process;
(b) the warp launch alone between events, beside dbx_patch_augment (the default Augment's records) and a copy_ of the same bytes; and
    with every slot given the same injected record, per kind of warp and border;
(c) next_batch() against the host stage a user would write without it: the un-warped batch copied to the host, the NumPy restatement
    (tests/warp_aug_ref.py, the same records) per patch, the result and the label rows uploaded;
(d) a DenseBoxLMLOC f16 training step (forward, loss, backward, SGD) fed by each of the two samplers.
Host clock around a device synchronise, the sides of a comparison alternating within this process, median and range of R timings.
--kernels-only: 20 warped next_batch() calls and nothing else, for a `rocprofv3 --kernel-trace --stats` run.
usage: python tools/gpu_warp_bench.py [--repeats R] [--kernels-only] [--no-step]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import warp_aug_ref as WR
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
    assert torch.cuda.is_available(), 'gpu_warp_bench needs the MI355X'
    frames, plates = scene()
    warp = data.Warp(seed=SEED)
    warped = data.PatchSampler(frames, plates, N, oversample=1.5, neg_frac=0.1, seed=SEED, warp=warp)
    if a.kernels_only:
        for _ in range(20):
            warped.next_batch()
        torch.cuda.synchronize()
        print('PatchSampler(warp=Warp()).next_batch: 20 calls, %d patches of 240 x 240 x 3 each' % N, flush=True)
        return
    plain = data.PatchSampler(frames, plates, N, oversample=1.5, neg_frac=0.1, seed=SEED)
    bank = warp.bank()
    f = warp.cfg()
    cfg = {k: getattr(f, k) for k in WR.CFG_DEFAULT}
    host_counter = [0]

    def on_host():
        patches, _, _, _, count = plain.next_batch()
        raw, rows = patches.cpu().numpy(), plain.plan.labels_i32.cpu().numpy()
        p = WR.plan(cfg, rows, count, bank=bank, seed=SEED, counter=host_counter[0])
        host_counter[0] += 1
        out = np.stack([WR.warp(raw[s], p['params'][s], p['inv'][s]) for s in range(count)])
        lab = np.concatenate([p['bbox'], p['vertices'], p['label']], axis=1)
        return torch.from_numpy(out).cuda(), torch.from_numpy(lab).cuda()

    for _ in range(3):
        warped.next_batch()
        plain.next_batch()
    on_host()
    tw, tp, th = [], [], []
    for _ in range(a.repeats):
        tw.append(timed_once(warped.next_batch))
        tp.append(timed_once(plain.next_batch))
        th.append(timed_once(on_host))
    print('%d frames of %d x %d on the device, %d patches per batch' % (FRAMES, H, W, N))
    report('PatchSampler(warp=Warp()).next_batch (plan + cut + warp plan + warp, 4-byte read)', tw)
    report('PatchSampler.next_batch with warp=None (the launches the sampler made before)', tp)
    report('next_batch + batch to the host + NumPy restatement + upload', th)
    flags = warped.warp_params[:, 0]
    print('last batch: %d warped, %d refused by the label rule, %d degenerate, %d off'
          % (int((flags == 1).sum()), int((flags == 2).sum()), int((flags == 4).sum()), int((flags == 0).sum())), flush=True)
    # the device side alone: launch() of each sampler captured into a graph (no Python between the launches), and the two new launches
    # between a pair of events, 20 in a row
    import gc
    graphs = []
    for smp in (warped, plain):
        g = torch.cuda.CUDAGraph()
        gc.collect()
        with torch.cuda.graph(g):
            smp.launch()
        graphs.append(g)
    for g in graphs:
        g.replay()
    tgw, tgp = [], []
    for _ in range(a.repeats):
        tgw.append(timed_once(graphs[0].replay))
        tgp.append(timed_once(graphs[1].replay))
    report('one graph replay of launch() with the warper (4 launches + the tally add)', tgw)
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

    s_ = warped
    wp = s_.warp_plan
    aug = data.Augment(seed=SEED)
    curves = torch.from_numpy(aug.curves()).cuda()
    aug_state = torch.tensor([SEED, 0], dtype=torch.int64, device='cuda')
    aplan = data.plan_augment(s_.plan.labels_i32, s_.plan.count, aug.cfg(), state=aug_state)
    scratch = torch.zeros_like(s_.patches)
    tk = [events(lambda: data.apply_warp(s_.patches, wp.params, wp.inv, s_.plan.count, s_.warped)) for _ in range(a.repeats)]
    tq = [events(lambda: data.plan_warp(s_.plan.labels_i32, s_.plan.count, s_.warp_cfg, bank=s_.rot_bank, state=s_.warp_state, out=wp))
          for _ in range(a.repeats)]
    ta = [events(lambda: data.apply_augment(s_.patches, aplan.params, s_.plan.count, curves, scratch)) for _ in range(a.repeats)]
    tc = [events(lambda: scratch.copy_(s_.patches)) for _ in range(a.repeats)]
    report('dbx_patch_warp alone, events around 20 launches (the last batch\'s records)', tk)
    report('dbx_patch_warp_plan alone, events around 20 launches', tq)
    report('dbx_patch_augment alone on the same patches (the default Augment\'s records), events around 20', ta)
    report('copy_ of the same 64 patches, events around 20', tc)
    # what each kind costs: all 64 slots given the same injected record (negative label rows: nothing is refused)
    quads = dict(WR.CASES)
    zero_rows = torch.zeros((N, 12), dtype=torch.int32, device='cuda')
    for name, rec in (('not asked for (the copy path)', WR.record(flags=0)), ('identity quad, replicate', WR.record(border=1)),
                      ('rotation +15, replicate', WR.record(quads['rot_+15'], border=1)),
                      ('rotation +15, constant', WR.record(quads['rot_+15'], border=0, fill=WR.pack_fill(127, 127, 127))),
                      ('scale 0.85, replicate', WR.record(quads['scale_0.85'], border=1)),
                      ('scale 1.15, replicate', WR.record(quads['scale_1.15'], border=1)),
                      ('strong keystone, replicate', WR.record(quads['strong_keystone'], border=1)),
                      ('wholly outside, constant', WR.record(quads['outside'], border=0))):
        recs = torch.from_numpy(np.stack([WR.to_row(rec)] * N)).cuda()
        ip = data.plan_warp(zero_rows, s_.plan.count, s_.warp_cfg, params=recs)
        t = [events(lambda: data.apply_warp(s_.patches, ip.params, ip.inv, s_.plan.count, scratch)) for _ in range(a.repeats)]
        report('dbx_patch_warp, every slot: %s' % name, t)
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
        step(warped)
    tr, tg = [], []
    for _ in range(a.repeats):
        tr.append(timed_once(lambda: step(plain)))
        tg.append(timed_once(lambda: step(warped)))
    report('training step, batch %d f16, fed by PatchSampler.next_batch' % N, tr)
    report('training step, batch %d f16, fed by PatchSampler(warp=Warp()).next_batch' % N, tg)


if __name__ == '__main__':
    main()
