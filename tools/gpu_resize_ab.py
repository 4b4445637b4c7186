"""Same-box A/B of dbx_resize_cubic_batch_u8 between two builds of the library -- this tree's and another (--other: a build of another
commit, or one made by tools/build_variant.sh) -- loaded into ONE process: pad_resize's jobs of 32 resident 1080 x 1920 frames to 720, 512
and 240, 20 launches between two events, 7 alternating rounds after one warm-up round, median with min and max.  The outputs of the two
builds are asserted equal.
usage: python tools/gpu_resize_ab.py --other PATH/libdensebox_hip.so"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from densebox_amd import _lib, resize


def load(path):
    L = C.CDLL(path)
    for name in ('dbx_resize_batch_workspace_bytes', 'dbx_resize_cubic_batch_u8', 'dbx_last_error'):
        res, args = _lib.SIGNATURES[name]
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--other', required=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'gpu_resize_ab needs the MI355X'
    libs = [('other', load(a.other)), ('this', load(_lib.LIB_PATH))]
    rs = np.random.RandomState(8)
    frames = torch.from_numpy(rs.randint(0, 256, size=(32, 1080, 1920, 3)).astype(np.uint8)).cuda()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for size in (720, 512, 240):
        spec = resize._pad_spec(list(frames.unbind(0)), size)
        n = len(spec)
        jobs = (_lib.ResizeJob * n)()
        for i, (r, (b, cx0, cy0, cw, ch, pl, pt, pr, pb, jh, jw)) in enumerate(zip(jobs, spec)):
            r.src, r.sh, r.sw = frames[b].data_ptr(), 1080, 1920
            r.cx0, r.cy0, r.cw, r.ch, r.pad_l, r.pad_t, r.pad_r, r.pad_b, r.pad_value = cx0, cy0, cw, ch, pl, pt, pr, pb, resize.PAD_VALUE
            r.dh, r.dw, r.dst_off = jh, jw, i * jh * jw * 3
        per, outs = {name: [] for name, _ in libs}, {}
        for rnd in range(8):
            for name, L in libs:
                out = torch.empty((n, size, size, 3), dtype=torch.uint8, device='cuda')
                ws = torch.empty(L.dbx_resize_batch_workspace_bytes(n), dtype=torch.uint8, device='cuda')

                def fn():
                    rc = L.dbx_resize_cubic_batch_u8(jobs, n, 3, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), stream)
                    assert rc == 0, L.dbx_last_error()
                fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    per[name].append(e0.elapsed_time(e1) / 20 * 1e3)
                outs[name] = out
        assert torch.equal(outs['other'], outs['this']), 'the two builds disagree'
        for name, v in per.items():
            v = sorted(v)
            print('pad_resize 32 x 1080x1920 -> %-3d %-5s %8.1f us per launch (min %.1f, max %.1f over 7 alternating rounds)'
                  % (size, name, v[len(v) // 2], v[0], v[-1]), flush=True)


if __name__ == '__main__':
    main()
