"""On-device evaluation next to the composition a user could write before it, at 512x512 B=32 on a synthetic DenseBoxLMLOC (f16),
threshold mode (max_dets=1024, the threshold chosen so that a few hundred pixels per frame pass):
  (a) evaluate_batch: forward, threshold decode, dbx_match_gt_batch and dbx_eval_append in one hipGraph replay, nothing copied back;
  (b) detect_batch_thresh + the NumPy matching of tests/eval_ref.py on the host, per frame.
The ground truth of a frame is a handful of its own kept boxes shifted by a few pixels, one of them ignored.  The frames are one CUDA
tensor.  The two are timed in turn, R rounds of a >= 0.2 s window each with a host clock; every call ends in a device synchronise.  The
figure is the median over the rounds, with min and max.  --kernels-only runs 20 evaluate_batch calls and nothing else, for a
`rocprofv3 --kernel-trace --stats` run of its own (the kernels are match_gt_batch_kernel and eval_append_kernel).
usage: python tools/gpu_evaluate_bench.py [--rounds R] [--kernels-only]"""
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
import eval_ref
from densebox_amd import evaluate, synth

H, W, B, CAP, N_GT = 512, 512, 32, 1024, 8


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
    assert torch.cuda.is_available(), 'gpu_evaluate_bench needs the MI355X'
    assert a.rounds >= 7, 'the median is taken over at least 7 alternating rounds'
    net = D.DenseBoxLMLOC(synth.vgg19_standin(0))
    synth.fill_params_(net, 11)
    net = net.cuda().eval()
    net.compute_dtype = 'f16'
    rs = np.random.RandomState(H + B)
    x = torch.from_numpy(rs.randint(0, 256, size=(B, H, W, 3)).astype(np.uint8)).cuda()
    top = net.detect_batch(x, K=256, max_batch=B)
    t = float(np.float32(np.median([d[-1, 4] for d, _ in top])))          # about 256 pixels per frame pass
    res = net.detect_batch_thresh(x, t, CAP, max_batch=B)
    boxes, ignore = [], []
    for d, keep in res:
        g = d[keep[:N_GT], :4] + rs.randint(-2, 3, size=(len(keep[:N_GT]), 4))
        boxes.append(g)
        ignore.append((np.arange(len(g)) == 1).astype(np.uint8))
    rows = sum(d.shape[0] for d, _ in res)
    kept = sum(len(k) for _, k in res)
    tag = '%4dx%-4d B=%-2d thresh max_dets=%d' % (W, H, B, CAP)
    ev = evaluate.Evaluator(capacity=1 << 20, max_gt=N_GT)

    def on_device():
        ev.reset()
        net.evaluate_batch(x, boxes, evaluator=ev, score_thresh=t, max_dets=CAP, max_batch=B, gt_ignore=ignore)

    def composed():
        out = []
        for (d, keep), g, ig in zip(net.detect_batch_thresh(x, t, CAP, max_batch=B), boxes, ignore):
            out.append(eval_ref.match_frame(d, keep, g, ig, None, 0.5))
        return out

    if a.kernels_only:
        for _ in range(20):
            on_device()
        torch.cuda.synchronize()
        print('%s evaluate_batch calls: 20, %d rows and %d kept rows per call' % (tag, rows, kept), flush=True)
        return
    on_device()
    s = ev.summary()
    host = composed()
    assert [s['tp'], s['fp'], s['ignored']] == [int(sum(h[4][i] for h in host)) for i in (1, 2, 3)], 'the two paths disagree'
    fns = [('(a) evaluate_batch (one graph replay, nothing copied back)', on_device),
           ('(b) detect_batch_thresh + NumPy matching on the host', composed)]
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
    ma, mb = (med[name] for name, _ in fns)
    print('%s (b) / (a) = %.2fx; %d rows, %d kept rows per call; tp %d fp %d ignored %d of %d GT boxes, AP %.4f'
          % (tag, mb / ma, rows, kept, s['tp'], s['fp'], s['ignored'], s['n_gt'], s['ap']), flush=True)


if __name__ == '__main__':
    main()
