"""Annotated frames on the device next to what a user could write before them, at 512x512 B=32 (32 camera streams, one frame each per
call) on a synthetic DenseBoxLMLOC (f16), top-K mode, K=10:
  (a) annotate_batch(tracker=...): forward, decode + NMS, the two tracking launches and dbx_draw_overlay_batch in one hipGraph replay;
      dets, keep, ids come back, the annotated frames stay on the device (the frames are a CUDA tensor);
  (b) track_batch alone (what the drawing adds to a call is (a) - (b));
  (c) track_batch + the frames to the host + the fastest NumPy drawing of the same pixels (slices for the outline and the label
      background, one masked assignment per label and disc); its output is asserted equal to (a)'s before anything is timed.
The frames are one CUDA tensor, the same for every call.  The three are timed in turn, R rounds of a >= 0.2 s window each with a host
clock; every call ends in a device synchronise.  The figure is the median over the rounds, with min and max.  --kernels-only runs 20
dbx_draw_overlay_batch launches on the rows of one call and 20 device-to-device copy_ of the same frames and nothing else, for a
`rocprofv3 --kernel-trace --stats` run of its own (the kernel is draw_overlay_batch_kernel); it also prints both as timed by events
in this process (20 launches between two events), and the share of tiles that carry rows.
usage: python tools/gpu_overlay_bench.py [--rounds R] [--kernels-only]"""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import densebox_amd as D
from densebox_amd import rows, synth, track, viz
from densebox_amd.frames import overlay_table

H, W, B, K = 512, 512, 32, 10


def window(fn, seconds=0.2):
    it, t0 = 0, time.perf_counter()
    while True:
        fn()
        torch.cuda.synchronize()
        it += 1
        dt = time.perf_counter() - t0
        if dt >= seconds and it >= 3:
            return dt / it * 1e3


class HostPainter:
    """the default style's pixels with slices and small masks"""

    def __init__(self, style):
        self.st, s, r = style, style.font_scale, style.radius
        font = viz.font()
        bits = ((font[:, :, None] >> np.arange(6)) & 1).astype(bool)                    # [14, 8, 6]
        self.glyph = np.kron(bits, np.ones((s, s), bool)) if s else None                # [14, 8 s, 6 s]
        yy, xx = np.mgrid[-r:r + 1, -r:r + 1] if r >= 0 else (None, None)
        self.disc = None if r < 0 else xx * xx + yy * yy <= r * r
        self.box, self.txt, self.mark = (np.array(c[:3], np.uint8) for c in (style.box_color, style.text_color, style.mark_color))

    @staticmethod
    def _fill(out, x0, x1, y0, y1, col):
        h, w = out.shape[:2]
        x0, x1, y0, y1 = max(x0, 0), min(x1, w - 1), max(y0, 0), min(y1, h - 1)
        if x0 <= x1 and y0 <= y1:
            out[y0:y1 + 1, x0:x1 + 1] = col

    @staticmethod
    def _mask(out, x, y, m, col):
        h, w = out.shape[:2]
        x0, x1, y0, y1 = max(x, 0), min(x + m.shape[1], w), max(y, 0), min(y + m.shape[0], h)
        if x0 < x1 and y0 < y1:
            out[y0:y1, x0:x1][m[y0 - y:y1 - y, x0 - x:x1 - x]] = col

    def draw(self, img, d, keep, tid):
        out = img.copy()
        t, s, r = self.st.thickness, self.st.font_scale, self.st.radius
        a = t // 2
        b = t - a
        for j, k in enumerate(keep):
            row = d[k].tolist()
            if not all(math.isfinite(v) and abs(v) < 2.0 ** 30 for v in row[:4]):
                continue
            X1, Y1, X2, Y2 = (int(v + 0.5) for v in row[:4])
            L, R, Tp, Bt = min(X1, X2), max(X1, X2), min(Y1, Y2), max(Y1, Y2)
            self._fill(out, L - a, R + a, Tp - a, min(Tp + b - 1, Bt + a), self.box)
            self._fill(out, L - a, R + a, max(Bt - b + 1, Tp - a), Bt + a, self.box)
            self._fill(out, L - a, min(L + b - 1, R + a), Tp - a, Bt + a, self.box)
            self._fill(out, max(R - b + 1, L - a), R + a, Tp - a, Bt + a, self.box)
            if s > 0:
                v = row[4]
                text = ('#%d ' % tid[j] if tid is not None and tid[j] >= 0 else '') + ('%.3f' % v if math.isfinite(v) and abs(v) < 1000 else '---')
                tw, th = 6 * s * len(text), 8 * s
                self._fill(out, X1, X1 + tw + 3, Y1 - th - 5, Y1, self.box)
                self._mask(out, X1 + 2, Y1 - 2 - th, np.concatenate([self.glyph['0123456789.-# '.index(ch)] for ch in text], axis=1), self.txt)
            if r >= 0 and len(row) == 13:
                for q in range(4):
                    vx, vy = row[5 + 2 * q], row[6 + 2 * q]
                    if math.isfinite(vx) and math.isfinite(vy) and abs(vx) < 2.0 ** 30 and abs(vy) < 2.0 ** 30:
                        self._mask(out, int(vx) - r, int(vy) - r, self.disc, self.mark)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--kernels-only', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'gpu_overlay_bench needs the MI355X'
    assert a.rounds >= 7, 'the median is taken over at least 7 alternating rounds'
    net = D.DenseBoxLMLOC(synth.vgg19_standin(0))
    synth.fill_params_(net, 11)
    net = net.cuda().eval()
    net.compute_dtype = 'f16'
    rs = np.random.RandomState(H + B)
    x = torch.from_numpy(rs.randint(0, 256, size=(B, H, W, 3)).astype(np.uint8)).cuda()
    tag = '%4dx%-4d B=%-2d K=%d' % (W, H, B, K)
    style = viz.Style()
    painter = HostPainter(style)
    tr_a, tr_b, tr_c = (track.Tracker(B, max_tracks=64) for _ in range(3))

    def on_device():
        return net.annotate_batch(x, tracker=tr_a, K=K, max_batch=B)

    def alone():
        return net.track_batch(x, tracker=tr_b, K=K, max_batch=B)

    def composed():
        res = net.track_batch(x, tracker=tr_c, K=K, max_batch=B)
        frames = x.cpu().numpy()
        return [painter.draw(frames[i], d, keep, tid) for i, (d, keep, tid, _) in enumerate(res)]

    if a.kernels_only:
        res = alone()
        d = torch.from_numpy(np.stack([r[0] for r in res])).cuda()
        keep = np.zeros((B, K + 1), np.int32)
        ids = np.full((B, K), -1, np.int32)
        for i, (_, kl, tid, _) in enumerate(res):
            keep[i, 0], keep[i, 1:1 + len(kl)], ids[i, :len(kl)] = len(kl), kl, tid
        keep, ids = torch.from_numpy(keep).cuda(), torch.from_numpy(ids).cuda()
        out = torch.empty_like(x)
        table = overlay_table(list(x.unbind(0)), list(out.unbind(0)))

        drows = rows.Rows(d, keep, None, B, K)

        def launch():
            viz._draw_launch(table, 3, H, W, drows, ids, None, None, 0, 0, style)

        def copy():
            out.copy_(x)
        times = {}
        for name, fn in (('dbx_draw_overlay_batch', launch), ('copy_ of the same frames', copy), ('dbx_draw_overlay_batch', launch),
                         ('copy_ of the same frames', copy)):
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times.setdefault(name, []).append(e0.elapsed_time(e1) / 20 * 1e3)
        launch()
        torch.cuda.synchronize()
        drawn = out.cpu().numpy()
        frames = x.cpu().numpy()
        tiles = (drawn != frames).any(axis=3).reshape(B, H // 16, 16, W // 128, 128).any(axis=(2, 4))
        for name, v in times.items():
            print('%s %-28s %s us per launch (20 launches between two events, two passes)' % (tag, name, ' / '.join('%.1f' % t for t in v)), flush=True)
        print('%s overlay / copy = %.2f; %d of %d tiles carry painted pixels; %.1f MB read + written per launch'
              % (tag, min(times['dbx_draw_overlay_batch']) / min(times['copy_ of the same frames']), int(tiles.sum()), tiles.size,
                 2 * x.numel() / 1e6), flush=True)
        return
    got = on_device()
    want = composed()
    assert all(np.array_equal(g[3].cpu().numpy(), w) for g, w in zip(got, want)), 'the two paths disagree'
    kept = sum(len(g[1]) for g in got)
    fns = [('(a) annotate_batch(tracker) (one graph replay)', on_device), ('(b) track_batch alone', alone),
           ('(c) track_batch + frames to the host + NumPy drawing', composed)]
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
        print('%s %-52s %9.3f ms/call (min %.3f, max %.3f over %d alternating rounds)' % (tag, name, med[name], v[0], v[-1], a.rounds), flush=True)
    ma, mb, mc = (med[name] for name, _ in fns)
    print('%s (a) - (b) = %+.3f ms; (c) / (a) = %.2fx; %d kept rows per call' % (tag, ma - mb, mc / ma, kept), flush=True)


if __name__ == '__main__':
    main()
