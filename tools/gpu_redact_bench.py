"""Redacted frames on the device next to what a user could write before them, at 512x512 B=32 (32 camera streams, one frame each per
call) on a synthetic DenseBoxLMLOC (f16), top-K mode, K=10, the default Redaction (pixelate, quads):
  (a) net.redact_batch(tracker=...): forward, decode + NMS, the two tracking launches and dbx_redact_batch in one hipGraph replay; dets,
      keep, ids come back, the redacted frames stay on the device (the frames are a CUDA tensor);
  (b) track_batch alone (what the redaction adds to a call is (a) - (b));
  (c) track_batch + the tracker's table and the frames to the host + a NumPy redaction of the same pixels (the restatement's integer
      rules; masks over each region's bounding rectangle, block sums by np.add.reduceat, window sums from an integral image) + the
      upload of the result; its output is asserted equal to (a)'s before anything is timed.
The frames are one CUDA tensor, the same for every call.  The three are timed in turn, R rounds of a >= 0.2 s window each with a host
clock; every call ends in a device synchronise.  The figure is the median over the rounds, with min and max.  --kernels-only runs 20
dbx_redact_batch launches per method (fill, pixelate 12, blur 8) on the rows and the tracker's table of one call and 20 device-to-device
copy_ of the same frames, each between two events, two passes; it also prints the share of tiles that carry redacted pixels.
usage: python tools/gpu_redact_bench.py [--rounds R] [--kernels-only]"""
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
from densebox_amd import redact, rows, synth, track
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


def _tdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def _sgn(v):
    return (v > 0) - (v < 0)


class HostRedactor:
    """dbx_redact_batch's pixels in NumPy, one frame at a time, working on bounding rectangles only"""

    def __init__(self, st, det_cols, max_age):
        self.st, self.quad = st, (st.shape == 'quad' or (st.shape is None and det_cols == 13)) and det_cols == 13
        self.coast = max_age if st.coast is None else st.coast

    def _box(self, b, h, w):
        if not all(math.isfinite(v) and abs(v) < 2.0 ** 30 for v in b):
            return None
        X1, Y1, X2, Y2 = (int(v + 0.5) for v in b)
        L, R, Tp, Bt = min(X1, X2), max(X1, X2), min(Y1, Y2), max(Y1, Y2)
        gx = self.st.grow + _tdiv((R - L + 1) * self.st.grow_pct, 100)
        gy = self.st.grow + _tdiv((Bt - Tp + 1) * self.st.grow_pct, 100)
        return max(L - gx, 0), min(R + gx, w - 1), max(Tp - gy, 0), min(Bt + gy, h - 1)

    def _quad(self, lm):
        if not all(math.isfinite(v) and abs(v) < 2.0 ** 20 for v in lm):
            return None
        P = [(int(lm[2 * q] + 0.5), int(lm[2 * q + 1] + 0.5)) for q in range(4)]
        if sum(P[q][0] * P[(q + 1) % 4][1] - P[(q + 1) % 4][0] * P[q][1] for q in range(4)) == 0:
            return None
        S = (sum(p[0] for p in P), sum(p[1] for p in P))
        return [tuple(4 * p[a] + _tdiv((4 * p[a] - S[a]) * self.st.grow_pct, 100) + 4 * self.st.grow * _sgn(4 * p[a] - S[a]) for a in range(2))
                for p in P]

    @staticmethod
    def _tri(a, b, c, X, Y):
        area2 = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
        if area2 == 0:
            return False
        s = _sgn(area2)
        return ((s * ((b[0] - a[0]) * (Y - a[1]) - (b[1] - a[1]) * (X - a[0])) >= 0) & (s * ((c[0] - b[0]) * (Y - b[1]) - (c[1] - b[1]) * (X - b[0])) >= 0)
                & (s * ((a[0] - c[0]) * (Y - c[1]) - (a[1] - c[1]) * (X - c[0])) >= 0))

    def mask(self, h, w, d, keep, live):
        m = np.zeros((h, w), bool)

        def box(b):
            r = self._box(b, h, w)
            if r is not None and r[0] <= r[1] and r[2] <= r[3]:
                m[r[2]:r[3] + 1, r[0]:r[1] + 1] = True
        for k in keep:
            row = d[k].tolist()
            if row[4] < self.st.min_score or self._box(row[:4], h, w) is None:
                continue
            G = self._quad(row[5:13]) if self.quad else None
            if G is None:
                box(row[:4])
                continue
            xa, xb = max(min(g[0] for g in G) >> 2, 0), min(max(g[0] for g in G) >> 2, w - 1)
            ya, yb = max(min(g[1] for g in G) >> 2, 0), min(max(g[1] for g in G) >> 2, h - 1)
            if xa <= xb and ya <= yb:
                X, Y = 4 * np.arange(xa, xb + 1, dtype=np.int64)[None, :], 4 * np.arange(ya, yb + 1, dtype=np.int64)[:, None]
                m[ya:yb + 1, xa:xb + 1] |= self._tri(G[0], G[1], G[2], X, Y) | self._tri(G[0], G[2], G[3], X, Y)
        if self.coast > 0:
            for t in live:
                if t['id'] >= 0 and 1 <= t['age'] <= self.coast:
                    box(t['box'].tolist())
        return m

    def redact(self, img, d, keep, live):
        h, w, c = img.shape
        m = self.mask(h, w, d, keep, live)
        out = img.copy()
        if not m.any():
            return out
        ys, xs = np.nonzero(m.any(axis=1))[0], np.nonzero(m.any(axis=0))[0]
        ya, yb, xa, xb = int(ys[0]), int(ys[-1]) + 1, int(xs[0]), int(xs[-1]) + 1
        if self.st.method == 'fill':
            out[m] = np.array(self.st.color[:c], np.uint8)
            return out
        if self.st.method == 'pixelate':
            s = self.st.cell
            ya, xa, yb, xb = ya // s * s, xa // s * s, min(-(-yb // s) * s, h), min(-(-xb // s) * s, w)
            crop = img[ya:yb, xa:xb].astype(np.int64)
            ri, ci = np.arange(0, yb - ya, s), np.arange(0, xb - xa, s)
            sums = np.add.reduceat(np.add.reduceat(crop, ri, axis=0), ci, axis=1)
            n = (np.diff(np.append(ri, yb - ya))[:, None] * np.diff(np.append(ci, xb - xa))[None, :])[:, :, None]
            val = np.repeat(np.repeat((sums + n // 2) // n, s, axis=0)[:yb - ya], s, axis=1)[:, :xb - xa]
        else:
            r = self.st.radius
            A = (2 * r + 1) ** 2
            yi, xi = np.clip(np.arange(ya - r, yb + r), 0, h - 1), np.clip(np.arange(xa - r, xb + r), 0, w - 1)
            pad = img[yi][:, xi].astype(np.int64)
            S = np.zeros((pad.shape[0] + 1, pad.shape[1] + 1, c), np.int64)
            S[1:, 1:] = pad.cumsum(axis=0).cumsum(axis=1)
            k = 2 * r + 1
            val = (S[k:, k:] - S[:-k, k:] - S[k:, :-k] + S[:-k, :-k] + A // 2) // A
        sub = m[ya:yb, xa:xb]
        out[ya:yb, xa:xb][sub] = val[sub]
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--kernels-only', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'gpu_redact_bench needs the MI355X'
    assert a.rounds >= 7, 'the median is taken over at least 7 alternating rounds'
    net = D.DenseBoxLMLOC(synth.vgg19_standin(0))
    synth.fill_params_(net, 11)
    net = net.cuda().eval()
    net.compute_dtype = 'f16'
    rs = np.random.RandomState(H + B)
    x = torch.from_numpy(rs.randint(0, 256, size=(B, H, W, 3)).astype(np.uint8)).cuda()
    tag = '%4dx%-4d B=%-2d K=%d' % (W, H, B, K)
    style = redact.Redaction()
    tr_a, tr_b, tr_c = (track.Tracker(B, max_tracks=64) for _ in range(3))
    host = HostRedactor(style, 13, tr_c.max_age)

    def on_device():
        return net.redact_batch(x, tracker=tr_a, K=K, max_batch=B, style=style)

    def alone():
        return net.track_batch(x, tracker=tr_b, K=K, max_batch=B)

    def composed():
        res = net.track_batch(x, tracker=tr_c, K=K, max_batch=B)
        live = tr_c.live()
        frames = x.cpu().numpy()
        out = np.stack([host.redact(frames[i], d, keep, live[i]) for i, (d, keep, _, _) in enumerate(res)])
        return torch.from_numpy(out).cuda()

    if a.kernels_only:
        res = alone()
        d = torch.from_numpy(np.stack([r[0] for r in res])).cuda()
        keep = np.zeros((B, K + 1), np.int32)
        for i, (_, kl, _, _) in enumerate(res):
            keep[i, 0], keep[i, 1:1 + len(kl)] = len(kl), kl
        keep = torch.from_numpy(keep).cuda()
        out = torch.empty_like(x)
        table = overlay_table(list(x.unbind(0)), list(out.unbind(0)))
        drows = rows.Rows(d, keep, None, B, K)
        state = tr_b._buffers(x.device)[0]
        tracks_at = state.data_ptr() + tr_b._layout()[0]
        methods = [('fill', redact.Redaction(method='fill')), ('pixelate 12', redact.Redaction(method='pixelate', cell=12)),
                   ('blur 8', redact.Redaction(method='blur', radius=8))]

        def launcher(st):
            rec = st.record(13, tr_b.max_age)
            return lambda: redact._redact_launch(table, 3, H, W, drows, tracks_at, tr_b.streams, 0, tr_b.max_tracks, rec)

        def copy():
            out.copy_(x)
        fns = [('dbx_redact_batch ' + n, launcher(st)) for n, st in methods] + [('copy_ of the same frames', copy)]
        times = {}
        for name, fn in fns + fns:
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times.setdefault(name, []).append(e0.elapsed_time(e1) / 20 * 1e3)
        fns[0][1]()
        torch.cuda.synchronize()
        tiles = (out.cpu().numpy() != x.cpu().numpy()).any(axis=3).reshape(B, H // 16, 16, W // 64, 64).any(axis=(2, 4))
        for name, v in times.items():
            print('%s %-28s %s us per launch (20 launches between two events, two passes)' % (tag, name, ' / '.join('%.1f' % t for t in v)), flush=True)
        cp = min(times['copy_ of the same frames'])
        print('%s redact / copy = %s; %d of %d tiles carry redacted pixels; %.1f MB read + written per launch'
              % (tag, ', '.join('%s %.2f' % (n, min(times['dbx_redact_batch ' + n]) / cp) for n, _ in methods), int(tiles.sum()), tiles.size,
                 2 * x.numel() / 1e6), flush=True)
        return
    got = on_device()
    want = composed()
    assert all(np.array_equal(g[3].cpu().numpy(), w.cpu().numpy()) for g, w in zip(got, want)), 'the two paths disagree'
    kept = sum(len(g[1]) for g in got)
    changed = sum(int((g[3] != x[i]).any(dim=2).sum()) for i, g in enumerate(got))
    fns = [('(a) redact_batch(tracker) (one graph replay)', on_device), ('(b) track_batch alone', alone),
           ('(c) track_batch + table and frames to the host + NumPy + upload', composed)]
    for _, fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    per = {name: [] for name, _ in fns}
    for _ in range(a.rounds):
        for name, fn in fns:
            per[name].append(window(fn))
    med, rng = {}, {}
    for name, _ in fns:
        v = sorted(per[name])
        med[name], rng[name] = v[len(v) // 2], (v[0], v[-1])
        print('%s %-64s %9.3f ms/call (min %.3f, max %.3f over %d alternating rounds)' % (tag, name, med[name], v[0], v[-1], a.rounds), flush=True)
    (na, _), (nb, _), (nc, _) = fns
    ma, mb, mc = med[na], med[nb], med[nc]

    def apart(p, q):
        return 'disjoint' if rng[p][1] < rng[q][0] or rng[q][1] < rng[p][0] else 'overlapping'
    print('%s (a) - (b) = %+.3f ms (ranges %s); (c) / (a) = %.2fx (ranges %s); %d kept rows and %d changed pixels per call'
          % (tag, ma - mb, apart(na, nb), mc / ma, apart(na, nc), kept, changed), flush=True)


if __name__ == '__main__':
    main()
