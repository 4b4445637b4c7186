#!/usr/bin/env python3
"""Writes tests/golden/decode_thresh.npz: one crafted DenseBoxLMLOC map set (64 x 96 map pixels, about 1500 candidates above
t = 0.5 in 12 clusters, all candidate scores distinct: tests/thresh_ref.craft_maps) with the rows and the keep list the REFERENCE
itself gives for them: parse_DetLMLOC(maps, K = n) and NMS(rows, 0.4), n = the number of pixels above t.  n > 1024 pins the large
NMS path to the reference directly.  The reference is imported unmodified with the stub modules oracle/gen_golden.py uses; it
exists in the build container only, and nothing of it is written but its results.

Usage:  python tools/gen_decode_thresh_golden.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from oracle.gen_golden import R  # noqa: E402  (the reference module, stubs in place)
import thresh_ref  # noqa: E402

ROWS, COLS, N_CAND, PLATES, T, NMS_T, SEED = 64, 96, 1500, 12, 0.5, 0.4, 1010


def main():
    m = thresh_ref.craft_maps(SEED, ROWS, COLS, N_CAND, PLATES, T)
    n = int((m['score'] > np.float32(T)).sum())
    assert n == N_CAND and len(np.unique(m['score'][m['score'] > np.float32(T)])) == n
    ts = {k: torch.from_numpy(v) for k, v in m.items()}
    rows = R.parse_DetLMLOC(ts['score'], ts['loc'], ts['lm_heat'], ts['lm_loc'], ROWS * 4, COLS * 4, K=n)
    keep = R.NMS(rows, NMS_T)
    out = os.path.join(ROOT, 'tests', 'golden', 'decode_thresh.npz')
    np.savez_compressed(out, score=m['score'], loc=m['loc'], lm_heat=m['lm_heat'], lm_loc=m['lm_loc'], t=np.float32(T),
                        nms_thresh=np.float64(NMS_T), rows=np.asarray(rows, np.float64), keep=np.asarray(keep, np.int64))
    print(out, os.path.getsize(out), 'bytes; n =', n, 'kept', len(keep))


if __name__ == '__main__':
    main()
