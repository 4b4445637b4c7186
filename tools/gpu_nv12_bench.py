"""NV12 frames in and out next to what a user could write before them, on 32 device-resident 1080 x 1920 NV12 frames (pitch = width) and a
synthetic DenseBoxLMLOC (f16), K=10:
  1. each conversion launch alone (dbx_nv12_to_rgb_batch, dbx_rgb_to_nv12_batch on a table made once) next to a device-to-device copy_
     that moves the same number of bytes (4.5 per pixel: a copy_ of 2.25 bytes per pixel reads and writes them), 20 launches between
     two events;
  2. detect_batch_resized_nv12 (the fused resize, size 720) next to nv12_to_rgb_batch + detect_batch_resized, whole calls on a host clock;
     and the two resize paths alone -- pad_resize_batch_nv12 next to nv12_to_rgb_batch + pad_resize_batch -- 10 calls between two events;
  3. redact_batch_nv12 at 512 x 512, 32 streams, next to redact_batch on resident RGB frames: the cost of the two conversions;
  4. redact_batch_nv12 next to the host composition: the frames to the host, the NumPy restatement (tests/nv12_ref.py) to RGB, redact_batch,
     the restatement back to NV12; its output is asserted equal before anything is timed.
Every figure is the median of R alternating rounds with min and max.
usage: python tools/gpu_nv12_bench.py [--rounds R]"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import densebox_amd as D
from densebox_amd import _lib, color, redact, resize, synth, track
from densebox_amd._lib import check, stream_ptr
import nv12_ref as N

H, W, B, K, SIZE = 1080, 1920, 32, 10, 720


def window(fn, seconds=0.2):
    it, t0 = 0, time.perf_counter()
    while True:
        fn()
        torch.cuda.synchronize()
        it += 1
        dt = time.perf_counter() - t0
        if dt >= seconds and it >= 3:
            return dt / it * 1e3


def events(fn, n):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def alternate(fns, rounds, timer):
    """{name: (median, min, max)} of `rounds` alternating timings of every (name, fn)"""
    for _, fn in fns:
        fn()
    torch.cuda.synchronize()
    per = {name: [] for name, _ in fns}
    for _ in range(rounds):
        for name, fn in fns:
            per[name].append(timer(fn))
    return {name: (sorted(v)[len(v) // 2], min(v), max(v)) for name, v in per.items()}


def apart(a, b):
    return 'disjoint' if a[2] < b[1] or b[2] < a[1] else 'overlapping'


def show(tag, res, unit, scale=1.0):
    for name, (m, lo, hi) in res.items():
        print('%s %-64s %9.3f %s (min %.3f, max %.3f)' % (tag, name, m * scale, unit, lo * scale, hi * scale), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'gpu_nv12_bench needs the MI355X'
    assert a.rounds >= 7, 'the median is taken over at least 7 alternating rounds'
    net = D.DenseBoxLMLOC(synth.vgg19_standin(0))
    synth.fill_params_(net, 11)
    net = net.cuda().eval()
    net.compute_dtype = 'f16'
    rs = np.random.RandomState(H + B)
    nv = torch.from_numpy(rs.randint(0, 256, size=(B, H * 3 // 2, W)).astype(np.uint8)).cuda()
    tag = '%dx%d B=%d' % (W, H, B)

    # ---- 1. the launches alone
    rgb = torch.empty((B, H, W, 3), dtype=torch.uint8, device='cuda')
    back = torch.empty_like(nv)
    L, par = _lib.lib(), color.Params().record()

    def table(y_of, rgb_of):
        rec = (_lib.Nv12Frame * B)()
        for b, r in enumerate(rec):
            r.y, r.uv, r.rgb = y_of[b].data_ptr(), y_of[b].data_ptr() + H * W, rgb_of[b].data_ptr()
            r.h, r.w, r.pitch_y, r.pitch_uv, r.pitch_rgb = H, W, W, W, 3 * W
        return torch.frombuffer(rec, dtype=torch.uint8).cuda()
    t_to, t_from = table(nv, rgb), table(back, rgb)
    half_a = torch.empty(B * H * W * 9 // 4, dtype=torch.uint8, device='cuda')
    half_b = torch.empty_like(half_a)
    fns = [('dbx_nv12_to_rgb_batch', lambda: check(L.dbx_nv12_to_rgb_batch(C.c_void_p(t_to.data_ptr()), B, H, W, C.byref(par), stream_ptr()))),
           ('dbx_rgb_to_nv12_batch', lambda: check(L.dbx_rgb_to_nv12_batch(C.c_void_p(t_from.data_ptr()), B, H, W, C.byref(par), stream_ptr()))),
           ('copy_ moving the same bytes', lambda: half_b.copy_(half_a))]
    res = alternate(fns, a.rounds, lambda fn: events(fn, 20))
    show(tag, res, 'us per launch', 1e3)
    cp = res['copy_ moving the same bytes']
    print('%s to_rgb / copy = %.2f (ranges %s), from_rgb / copy = %.2f (ranges %s); %.1f MB moved per launch'
          % (tag, res['dbx_nv12_to_rgb_batch'][0] / cp[0], apart(res['dbx_nv12_to_rgb_batch'], cp), res['dbx_rgb_to_nv12_batch'][0] / cp[0],
             apart(res['dbx_rgb_to_nv12_batch'], cp), B * H * W * 4.5 / 1e6), flush=True)
    del rgb, back, half_a, half_b

    # ---- 2. the resized detection, fused and in two launches
    def fused():
        return net.detect_batch_resized_nv12(nv, SIZE, K=K, max_batch=B)

    def two_step():
        return net.detect_batch_resized(color.nv12_to_rgb_batch(nv), SIZE, K=K, max_batch=B)
    got, want = fused(), two_step()
    assert all(np.array_equal(g[0], w[0]) and g[1] == w[1] for g, w in zip(got, want)), 'the two detection paths disagree'
    res = alternate([('detect_batch_resized_nv12 (fused resize)', fused), ('nv12_to_rgb_batch + detect_batch_resized', two_step)], a.rounds, window)
    show(tag + ' size=%d' % SIZE, res, 'ms/call')
    f, t = res['detect_batch_resized_nv12 (fused resize)'], res['nv12_to_rgb_batch + detect_batch_resized']
    print('%s fused - two launches = %+.3f ms (ranges %s)' % (tag, f[0] - t[0], apart(f, t)), flush=True)
    res = alternate([('pad_resize_batch_nv12 (one launch)', lambda: resize.pad_resize_batch_nv12(nv, SIZE)),
                     ('nv12_to_rgb_batch + pad_resize_batch (two launches)', lambda: resize.pad_resize_batch(color.nv12_to_rgb_batch(nv), SIZE))],
                    a.rounds, lambda fn: events(fn, 10))
    show(tag + ' size=%d' % SIZE, res, 'us per call', 1e3)
    f, t = res['pad_resize_batch_nv12 (one launch)'], res['nv12_to_rgb_batch + pad_resize_batch (two launches)']
    print('%s resize alone: fused / two launches = %.2f (ranges %s)' % (tag, f[0] / t[0], apart(f, t)), flush=True)

    # ---- 3. and 4. redaction with NV12 on both sides
    h = w = 512
    small = torch.from_numpy(rs.randint(0, 256, size=(B, h * 3 // 2, w)).astype(np.uint8)).cuda()
    x = color.nv12_to_rgb_batch(small).clone()
    style = redact.Redaction()
    tr_a, tr_b, tr_c = (track.Tracker(B, max_tracks=64) for _ in range(3))

    def nv12_both_sides():
        return net.redact_batch_nv12(small, tracker=tr_a, K=K, max_batch=B, style=style)

    def resident_rgb():
        return net.redact_batch(x, tracker=tr_b, K=K, max_batch=B, style=style)

    def host_composition():
        frames = small.cpu().numpy()
        xs = torch.from_numpy(np.stack([N.nv12_to_rgb(f) for f in frames])).cuda()
        res = net.redact_batch(xs, tracker=tr_c, K=K, max_batch=B, style=style)
        painted = torch.stack([r[3] for r in res]).cpu().numpy()
        return torch.from_numpy(np.stack([N.rgb_to_nv12(p) for p in painted])).cuda()
    got, want = nv12_both_sides(), host_composition()
    assert all(np.array_equal(g[3].cpu().numpy(), w.cpu().numpy()) for g, w in zip(got, want)), 'the two redaction paths disagree'
    resident_rgb()
    tag = '%dx%d B=%d' % (w, h, B)
    res = alternate([('(a) redact_batch_nv12 (NV12 in, NV12 out)', nv12_both_sides), ('(b) redact_batch on resident RGB', resident_rgb),
                     ('(c) frames to the host + NumPy both ways around redact_batch', host_composition)], a.rounds, window)
    show(tag, res, 'ms/call')
    ra, rb, rc = (res[k] for k in res)
    print('%s (a) - (b) = %+.3f ms (ranges %s); (c) / (a) = %.2fx (ranges %s)' % (tag, ra[0] - rb[0], apart(ra, rb), rc[0] / ra[0], apart(ra, rc)),
          flush=True)


if __name__ == '__main__':
    main()
