"""The threshold pyramid against the composition a user could write before it existed.

DenseBoxLMLOC, f16, sizes (480, 720, 1080), max_dets 1365 (3 x 1365 <= 4096), 32 frames of 1080 x 1920, (a) device-resident and (b) as
host numpy arrays, at two thresholds picked on the 720 level of frame 0 to leave about 300 and about 3000 pixels above them (the second
is cut by max_dets).  After warm-up, net.detect_pyramid(score_thresh=...) and the composition -- one detect_batch_resized(score_thresh=...)
call per size, a host concatenate, decode.NMS per frame -- alternate within one process; median, min and max of R timings each (host
clock around a device synchronise).  A pair whose min-max ranges overlap is reported as "no difference shown".

Without --step this is a driver: every GPU step runs as a child process under its own time limit, and the first failure ends the run.
  --step timing   the timings; writes --out (default profiles/r11_pyramid_thresh.txt)
  --step trace    warm-up plus 5 detect_pyramid calls of workload (a) at the first threshold and nothing else; the driver runs it under
                  `rocprofv3 --kernel-trace --stats` (skipped with --no-trace) into --trace-dir
usage: python tools/gpu_pyramid_thresh_bench.py [--repeats R] [--out FILE] [--no-trace] [--trace-dir DIR]"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (480, 720, 1080)
CAP = 1365
PICKS = (300, 3000)


def timed_once(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def composition(net, frames, t):
    import numpy as np
    from densebox_amd import decode
    per = [net.detect_batch_resized(frames, size=s, score_thresh=t, max_dets=CAP) for s in SIZES]
    out = []
    for i in range(len(per[0])):
        d = np.concatenate([p[i][0] for p in per], axis=0)
        out.append((d, decode.NMS(d, 0.4) if len(d) else []))
    return out


def setup():
    import numpy as np
    import torch
    import densebox_amd as D
    from densebox_amd import decode, resize, synth
    assert torch.cuda.is_available(), 'gpu_pyramid_thresh_bench needs the MI355X'
    net = D.DenseBoxLMLOC(synth.vgg19_standin(0))
    synth.fill_params_(net, 11)
    net = net.cuda().eval()
    net.compute_dtype = 'f16'
    rs = np.random.RandomState(8)
    host = [rs.randint(0, 256, size=(1080, 1920, 3)).astype(np.uint8) for _ in range(32)]
    dev = [torch.from_numpy(f).cuda() for f in host]
    with torch.no_grad():
        s = decode._maps(net.KIND, net(resize.pad_resize_batch(dev[:1], SIZES[1])))[0][0]
    s = torch.sort(s.reshape(-1).float(), descending=True).values
    return net, host, dev, [float(s[c]) for c in PICKS]


def step_timing(a):
    import numpy as np
    net, host, dev, picks = setup()
    R = max(a.repeats, 7)
    lines = ['DenseBoxLMLOC f16, sizes %s, max_dets %d, 32 frames of 1080x1920 per call; one MI355X, median (min .. max) of %d alternating '
             'timings, ms per call' % (SIZES, CAP, R)]
    for want, t in zip(PICKS, picks):
        for name, frames in (('(a) device-resident frames', dev), ('(b) the same frames as host numpy arrays', host)):
            for _ in range(2):                               # warm both: plans, three 'level_thresh' graphs and three 'thresh' graphs
                got = net.detect_pyramid(frames, sizes=SIZES, score_thresh=t, max_dets=CAP, with_levels=True)
                ref = composition(net, frames, t)
            same = all(g[0].tobytes() == r[0].tobytes() and g[1] == r[1] for g, r in zip(got, ref))
            lv = np.stack([g[2] for g in got])
            tp, tc = [], []
            for _ in range(R):                               # alternating within one process
                tp.append(timed_once(lambda: net.detect_pyramid(frames, sizes=SIZES, score_thresh=t, max_dets=CAP)))
                tc.append(timed_once(lambda: composition(net, frames, t)))
            overlap = min(tc) <= max(tp) and min(tp) <= max(tc)
            verdict = 'no difference shown (the ranges overlap)' if overlap else ('the ranges are disjoint: detect_pyramid %.1f %% %s' % (
                abs(1.0 - median(tp) / median(tc)) * 100.0, 'less' if median(tp) < median(tc) else 'MORE'))
            lines += ['threshold %r (picked to leave %d pixels of frame 0 at 720) %s' % (t, want, name),
                      '    rows per frame at %s: mean %s, min %s, max %s; kept per frame: mean %.1f'
                      % (SIZES, lv.mean(axis=0).round(1).tolist(), lv.min(axis=0).tolist(), lv.max(axis=0).tolist(),
                         float(np.mean([len(g[1]) for g in got]))),
                      '    detect_pyramid(score_thresh)                                              %9.3f (%.3f .. %.3f)'
                      % (median(tp), min(tp), max(tp)),
                      '    3 x detect_batch_resized(score_thresh) + concatenate + 32 x decode.NMS    %9.3f (%.3f .. %.3f)'
                      % (median(tc), min(tc), max(tc)),
                      '    %s; results %s' % (verdict, 'identical' if same else 'DIFFER')]
            print('\n'.join(lines[-5:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def step_trace(a):
    import torch
    net, host, dev, picks = setup()
    for _ in range(3 + 5):
        net.detect_pyramid(dev, sizes=SIZES, score_thresh=picks[0], max_dets=CAP)
    torch.cuda.synchronize()
    print('detect_pyramid(score_thresh=%r, max_dets=%d): 3 warm-up + 5 calls on 32 device-resident 1080 x 1920 frames, sizes %s'
          % (picks[0], CAP, SIZES), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r11_pyramid_thresh.txt'))
    ap.add_argument('--step', choices=['timing', 'trace'])
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--trace-dir', default=os.path.join(ROOT, 'build', 'pyramid_thresh_trace'))
    a = ap.parse_args()
    if a.step:
        return {'timing': step_timing, 'trace': step_trace}[a.step](a)
    me = [sys.executable, os.path.abspath(__file__)]
    steps = [['timeout', '-k', '10', '480'] + me + ['--step', 'timing', '--repeats', str(a.repeats), '--out', a.out]]
    if not a.no_trace:
        steps.append(['timeout', '-k', '10', '300', 'rocprofv3', '--kernel-trace', '--stats', '-d', a.trace_dir, '--output-format', 'csv',
                      '--'] + me + ['--step', 'trace'])
    for cmd in steps:                                        # chained: nothing more is started on the GPU after a failure
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit('gpu_pyramid_thresh_bench: `%s` ended with status %d; stopping' % (' '.join(cmd), rc))


if __name__ == '__main__':
    main()
