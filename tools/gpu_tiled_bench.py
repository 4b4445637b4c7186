"""Tiled detection against the composition a user could write before it existed, on one MI355X.

DenseBoxLMLOC, f16, 8 device-resident frames of 2160 x 3840, tile = src = 512, overlap 128 (60 tiles per frame, 480 per call), K = 10.
After warm-up, alternating within one process, median and range of R timings each (host clock around a device synchronise):
  (a) net.detect_tiled
  (b) the composition with the public calls: resize.crop_resize_batch over the same windows, net.detect_batch over the tiles in chunks of
      32, and on the host the map to frame coordinates, the ownership rule and decode.NMS per frame
  (c) net.detect_batch on the whole frames, one frame per forward, if it fits -- DIFFERENT work (one 2160 x 3840 forward sees every
      plate at native size without tile borders, and takes gigabytes of activations): reported, not compared
then the time between events of the cut launch and of the two stitch launches, and (a) and (b) again with src = 256 (2 x magnification,
464 tiles per frame; K = 8 there, because 464 x 10 rows exceed the NMS's 4096 per frame).

Without --step this is a driver: the GPU step runs as a child process under its own time limit.
usage: python tools/gpu_tiled_bench.py [--repeats R] [--out FILE] [--no-whole]"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, B, TILE, OVERLAP = 2160, 3840, 8, 512, 128


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


def stat(v):
    return '%9.3f (%.3f .. %.3f)' % (median(v), min(v), max(v))


def composition(net, frames, table, K):
    """(b): the public calls and the host"""
    import numpy as np
    import torch
    from densebox_amd import decode, resize
    windows = [[(int(t['x0']), int(t['y0']), int(t['x0'] + t['side']), int(t['y0'] + t['side'])) for t in table[table['frame'] == b]]
               for b in range(len(frames))]
    x = resize.crop_resize_batch(frames, windows, size=(TILE, TILE))
    per = net.detect_batch(x, K=K, max_batch=32)
    dc = per[0][0].shape[1]
    xs, ys = [0, 2] + list(range(5, dc, 2)), [1, 3] + list(range(6, dc, 2))
    rows = [[] for _ in frames]
    for t, (d, _) in zip(table, per):
        d = d.copy()
        d[:, xs] = d[:, xs] * t['scale'] - (-np.float64(t['x0']))
        d[:, ys] = d[:, ys] * t['scale'] - (-np.float64(t['y0']))
        sx, sy = d[:, 0] + d[:, 2], d[:, 1] + d[:, 3]
        own = (t['lo2x'] <= sx) & (sx < t['hi2x']) & (t['lo2y'] <= sy) & (sy < t['hi2y'])
        rows[int(t['frame'])].append(d[own])
    out = []
    for r in rows:
        d = np.concatenate(r)
        out.append((d, decode.NMS(d, 0.4) if len(d) else []))
    return out


def event_ms(fn, repeats):
    import torch
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def step_timing(a):
    import numpy as np
    import torch
    import densebox_amd as D
    from densebox_amd import decode, synth, tiles
    assert torch.cuda.is_available(), 'gpu_tiled_bench needs the MI355X'
    net = D.DenseBoxLMLOC(synth.vgg19_standin(0))
    synth.fill_params_(net, 11)
    net = net.cuda().eval()
    net.compute_dtype = 'f16'
    rs = np.random.RandomState(8)
    frames = [torch.from_numpy(rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)).cuda() for _ in range(B)]
    R = max(a.repeats, 7)
    lines = ['DenseBoxLMLOC f16, %d device-resident frames of %d x %d, tile %d, overlap %d; one MI355X, median (min .. max) of %d '
             'alternating timings, ms per call' % (B, H, W, TILE, OVERLAP, R)]
    for src, K in ((512, 10), (256, 8)):
        table = tiles.call_table('bench', [(H, W)] * B, TILE, src, OVERLAP)
        for _ in range(2):
            got = net.detect_tiled(frames, tile=TILE, src=src, overlap=OVERLAP, K=K)
            ref = composition(net, frames, table, K)
        same = all(g[0].tobytes() == r[0].tobytes() and g[1] == r[1] for g, r in zip(got, ref))
        ta, tb = [], []
        for _ in range(R):
            ta.append(timed_once(lambda: net.detect_tiled(frames, tile=TILE, src=src, overlap=OVERLAP, K=K)))
            tb.append(timed_once(lambda: composition(net, frames, table, K)))
        overlap = min(tb) <= max(ta) and min(ta) <= max(tb)
        verdict = 'no difference shown (the ranges overlap)' if overlap else ('the ranges are disjoint: detect_tiled %.1f %% %s' % (
            abs(1.0 - median(ta) / median(tb)) * 100.0, 'less' if median(ta) < median(tb) else 'MORE'))
        lines += ['src %d (%d tiles per frame, %d per call), K %d: %d owned rows per call, %.1f kept per frame'
                  % (src, table.shape[0] // B, table.shape[0], K, sum(len(g[0]) for g in got), float(np.mean([len(g[1]) for g in got]))),
                  '    (a) detect_tiled                                                     %s' % stat(ta),
                  '    (b) crop_resize_batch + detect_batch + host map / ownership / NMS     %s' % stat(tb),
                  '    %s; results %s' % (verdict, 'identical' if same else 'DIFFER')]
        # the pieces between events: the cut launch, and the stitch launches on rows of the right shape
        cut = event_ms(lambda: tiles.cut(frames, table, TILE), R)
        n = table.shape[0]
        tdev = torch.from_numpy(table.view(np.uint8).copy()).cuda()
        st = tiles._Stitch('bench', table, tdev, B, K, 13, tiles.RULES['core'], tdev.device)
        x = tiles.cut(frames, table[:32], TILE)
        d = decode._run_chunk(net, 'level', x, (K, 0.4), decode._detect_batch_eager(K, 0.4), (False, False))[0]
        rows_ms = event_ms(lambda: [st.rows(d[:min(32, n - t0)], None, t0, min(32, n - t0)) for t0 in range(0, n, 32)], R)
        nms_ms = event_ms(lambda: st.nms(0.4), R)
        lines += ['    between events: the cut launch (%d jobs)                             %s' % (n, stat(cut)),
                  '    between events: %d dbx_tile_rows_batch launches                       %s' % ((n + 31) // 32, stat(rows_ms)),
                  '    between events: dbx_tile_nms_batch (3 launches; every tile delivers tile 0..31\'s rows)  %s' % stat(nms_ms)]
        print('\n'.join(lines[-7:]), flush=True)
    if not a.no_whole:
        try:
            for _ in range(2):
                net.detect_batch(frames[0].unsqueeze(0), K=10)
            tc = [timed_once(lambda: [net.detect_batch(f.unsqueeze(0), K=10) for f in frames]) for _ in range(3)]
            lines.append('(c) detect_batch on the %d whole frames, one per forward (different work, not a comparison)  %s' % (B, stat(tc)))
        except RuntimeError as e:
            lines.append('(c) detect_batch on a whole %d x %d frame does not fit: %s' % (H, W, str(e).splitlines()[0][:160]))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r23_tiled.txt'))
    ap.add_argument('--step', choices=['timing'])
    ap.add_argument('--no-whole', action='store_true')
    a = ap.parse_args()
    if a.step:
        return step_timing(a)
    cmd = ['timeout', '-k', '10', '540', sys.executable, os.path.abspath(__file__), '--step', 'timing', '--repeats', str(a.repeats), '--out', a.out]
    if a.no_whole:
        cmd.append('--no-whole')
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        sys.exit('gpu_tiled_bench: `%s` ended with status %d; stopping' % (' '.join(cmd), rc))


if __name__ == '__main__':
    main()
