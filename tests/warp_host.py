"""The host exports of the training patch warp (dbx_patch_warp_params_host, dbx_patch_warp_host: the kernels' own __host__ __device__
functions) called through ctypes, and the bitwise comparison of a plan with the restatement's; shared by tests/test_warp_ref.py and
tests/test_hip_warp.py."""
import ctypes as C

import numpy as np

import warp_aug_ref as W

from densebox_amd import _lib

p = lambda a: a.ctypes.data_as(C.c_void_p)              # noqa: E731


def _cfg(**kw):
    cfg = dict(W.CFG_DEFAULT)
    cfg.update(kw)
    f = _lib.PatchWarpCfg()
    for k, v in cfg.items():
        setattr(f, k, v)
    return cfg, f


def host_plan(cfg, rows, count, params_in=None, bank=None, seed=0, counter=0):
    n = max(count, 1)
    out = dict(params=np.full((n, 16), -7, np.int32), labels=np.full((n, 12), -7, np.int32), bbox=np.full((n, 4), -7, np.float32),
               vertices=np.full((n, 8), -7, np.float32), label=np.full((n, 1), -7, np.float32), fwd=np.full((n, 9), -7, np.float64),
               inv=np.full((n, 9), -7, np.float64))
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    rec = np.ascontiguousarray(np.stack([W.to_row(r) if isinstance(r, dict) else r for r in params_in])) if params_in is not None else None
    bank = np.ascontiguousarray(bank, dtype=np.int32) if bank is not None else None
    _lib.check(_lib.lib().dbx_patch_warp_params_host(C.byref(_cfg(**cfg)[1]), seed, counter, p(rec) if rec is not None else None,
                                                     p(bank) if bank is not None else None, p(rows), count, p(out['params']), p(out['labels']),
                                                     p(out['bbox']), p(out['vertices']), p(out['label']), p(out['fwd']), p(out['inv'])))
    return {k: v[:count] for k, v in out.items()}


def host_warp(patch, row, inv):
    out = np.zeros_like(patch)
    row, inv = np.ascontiguousarray(row, dtype=np.int32), np.ascontiguousarray(inv, dtype=np.float64)
    _lib.check(_lib.lib().dbx_patch_warp_host(p(np.ascontiguousarray(patch)), p(row), p(inv), patch.shape[2], p(out)))
    return out


def same_plan(got, want):
    for k in ('params', 'labels'):
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:4].tolist())
    for k in ('bbox', 'vertices', 'label'):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    for k in ('fwd', 'inv'):
        bad = np.argwhere(got[k].view(np.uint64) != want[k].view(np.uint64))
        assert len(bad) == 0, (k, bad[:4].tolist(), got[k][bad[0][0]], want[k][bad[0][0]])
