"""The C-ABI boundary of the training patch warp without a GPU: the symbols are declared, bound and exported with the ABI version still
13; the struct layouts are the documented ones; every bad argument is refused on the host with its code and message before any launch;
data.Warp makes the cfg and the bank the header describes."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_aug_ref as W                                # noqa: E402

from densebox_amd import _build, _lib, data             # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('dbx_patch_warp_plan', 'dbx_patch_warp', 'dbx_patch_warp_params_host', 'dbx_patch_warp_host')
ERR_ARG = -1


def test_symbols_are_declared_bound_and_exported_without_a_version_bump():
    header = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    lib = _build.build(verbose=False)
    L = _lib.lib()
    exported = subprocess.run(['nm', '-D', '--defined-only', lib], capture_output=True, text=True).stdout
    for name in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in _lib.SIGNATURES and name not in _lib.MISSING and hasattr(L, name), name
        assert re.search(r' T %s\b' % name, exported), name
    assert L.dbx_version() == _lib.ABI_VERSION == 13 and '#define DBX_ABI_VERSION 13' in header
    assert 'training patch warp' in header and 'also at 13, without a bump: dbx_patch_warp_rec' in header


def test_struct_layouts_are_the_documented_ones():
    assert C.sizeof(_lib.PatchWarpRec) == 64 and C.sizeof(_lib.PatchWarpCfg) == 72 and C.sizeof(_lib.PatchWarpIO) == 96
    offs = {n: getattr(_lib.PatchWarpRec, n).offset for n, _ in _lib.PatchWarpRec._fields_}
    assert offs == dict(flags=0, border=4, fill=8, rot=12, quad=16, scale=48, aspect=52, shear=56, reserved=60)
    offs = {n: getattr(_lib.PatchWarpCfg, n).offset for n, _ in _lib.PatchWarpCfg._fields_}
    assert offs == dict(p_warp=0, rot_lo=8, rot_hi=12, scale_lo=16, scale_hi=20, aspect_lo=24, aspect_hi=28, shear_lo=32, shear_hi=36, tx=40,
                        ty=44, jitter=48, margin=52, border=56, fill=60, R=64, reserved=68)
    assert [n for n, _ in _lib.PatchWarpIO._fields_] == ['labels_in', 'count', 'params_in', 'state', 'rot', 'params', 'labels', 'bbox',
                                                        'vertices', 'label', 'fwd', 'inv']
    assert len(data.WARP_FIELDS) == len(W.FIELDS) == 16 and data.WARP_IDENTITY_QUAD == W.IDENTITY_QUAD
    # the header's layout comment names the same offsets
    header = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    for word in ('dbx_patch_warp_rec (64 bytes', 'dbx_patch_warp_cfg (72 bytes', 'flags 0', 'border 4', 'fill 8', 'rot 12', 'quad 16', 'scale 48',
                 'aspect 52', 'shear 56', 'reserved 60', 'tx 40', 'R 64', '96 bytes: 12 pointers'):
        assert word in header, word


def _io(**kw):
    io = _lib.PatchWarpIO()
    for k, _ in _lib.PatchWarpIO._fields_:
        setattr(io, k, 0x1000)                          # never followed: every call below is refused before a launch
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def _refused(rc, word):
    msg = _lib.lib().dbx_last_error().decode()
    assert rc == ERR_ARG and word in msg, (rc, msg)
    with pytest.raises(RuntimeError, match=re.escape(word)):
        _lib.check(rc)


CFG_BAD = [
    (dict(p_warp=1.5), 'p_warp'), (dict(p_warp=-0.1), 'p_warp'), (dict(p_warp=float('nan')), 'p_warp'),
    (dict(rot_lo=3, rot_hi=2), 'rot range'), (dict(rot_hi=31), 'leaves the bank'), (dict(rot_lo=-1), 'leaves the bank'),
    (dict(R=30), 'leaves the bank'), (dict(R=-1), 'R=-1'),
    (dict(scale_lo=0), 'scale'), (dict(scale_hi=65536), 'scale'), (dict(scale_lo=300, scale_hi=299), 'scale'),
    (dict(aspect_lo=0), 'aspect'), (dict(aspect_hi=65536), 'aspect'), (dict(aspect_lo=283), 'aspect'),
    (dict(shear_lo=-65536), 'shear'), (dict(shear_hi=65536), 'shear'), (dict(shear_lo=27), 'shear'),
    (dict(tx=65537), 'tx='), (dict(tx=-1), 'tx='), (dict(ty=65537), 'ty='), (dict(ty=-1), 'ty='), (dict(jitter=65537), 'jitter='),
    (dict(jitter=-1), 'jitter='), (dict(margin=-1), 'margin'), (dict(margin=120), 'margin'), (dict(border=2), 'border'),
    (dict(border=-1), 'border'),
]


def _cfg(**kw):
    cfg = dict(W.CFG_DEFAULT)
    cfg.update(kw)
    f = _lib.PatchWarpCfg()
    for k, v in cfg.items():
        setattr(f, k, v)
    return f


p = lambda a: a.ctypes.data_as(C.c_void_p)              # noqa: E731


def _host_args(count=4):
    """(label rows, the seven outputs side by side in one zeroed buffer, the call's last nine arguments)."""
    rows = np.zeros((count, 12), np.int32)
    out = np.zeros((7, count * 9), np.float64)          # a row holds the largest output, [count][9] doubles
    return rows, out, [p(rows), count] + [p(out[k]) for k in range(7)]


@pytest.mark.parametrize('bad,word', CFG_BAD, ids=[str(b) for b, _ in CFG_BAD])
def test_a_bad_cfg_is_refused_by_the_plan_and_by_the_host_function(bad, word):
    L = _lib.lib()
    _refused(L.dbx_patch_warp_plan(C.byref(_io(params_in=None)), C.byref(_cfg(**bad)), 4, None), word)
    _refused(L.dbx_patch_warp_plan(C.byref(_io()), C.byref(_cfg(**bad)), 4, None), word)          # in injected mode as well
    bank = W.rot_bank(-15, 15)
    rows, out, tail = _host_args()
    _refused(L.dbx_patch_warp_params_host(C.byref(_cfg(**bad)), 0, 0, None, p(bank), *tail), word)
    assert not out.any()


def test_a_rot_range_outside_an_unused_bank_is_fine_and_so_is_no_bank():
    rows, out, tail = _host_args(2)
    assert _lib.lib().dbx_patch_warp_params_host(C.byref(_cfg(p_warp=0.0, R=0, rot_lo=-5, rot_hi=40)), 3, 4, None, None, *tail) == 0
    rec = out[0].view(np.int32)[:32].reshape(2, 16)     # the records come first
    assert not rec[:, 0].any() and (rec[:, 4:12] == np.array(W.IDENTITY_QUAD)).all() and (rec[:, 3] >= -5).all() and (rec[:, 3] <= 40).all()
    assert np.array_equal(out[5, :9], np.array(W.EYE)) and np.array_equal(out[6, 9:18], np.array(W.EYE))
    _refused(_lib.lib().dbx_patch_warp_params_host(C.byref(_cfg()), 3, 4, None, None, *tail), 'null rot bank')
    _refused(_lib.lib().dbx_patch_warp_plan(C.byref(_io(params_in=None, rot=None)), C.byref(_cfg()), 4, None), 'null rot bank')
    # injected mode needs neither the bank nor the state
    recs = np.stack([W.to_row(W.record())] * 2)
    assert _lib.lib().dbx_patch_warp_params_host(C.byref(_cfg()), 0, 0, p(recs), None, *tail) == 0


def test_plan_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    good = _cfg()
    _refused(L.dbx_patch_warp_plan(None, C.byref(good), 4, None), 'null io')
    _refused(L.dbx_patch_warp_plan(C.byref(_io()), None, 4, None), 'null cfg')
    for n in (0, -3, 4097):
        _refused(L.dbx_patch_warp_plan(C.byref(_io()), C.byref(good), n, None), 'n=%d' % n)
    for k in ('labels_in', 'count'):
        _refused(L.dbx_patch_warp_plan(C.byref(_io(**{k: None})), C.byref(good), 4, None), 'null input')
    _refused(L.dbx_patch_warp_plan(C.byref(_io(params_in=None, state=None)), C.byref(good), 4, None), 'null state')
    for k in ('params', 'labels', 'bbox', 'vertices', 'label', 'fwd', 'inv'):
        _refused(L.dbx_patch_warp_plan(C.byref(_io(**{k: None})), C.byref(good), 4, None), 'null output')


def test_warp_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    V = C.c_void_p
    size = 240 * 240 * 3
    a, b = 0x40000000, 0x40000000 + 8 * size            # never followed
    call = lambda patches=a, params=0x1000, inv=0x3000, count=0x2000, n=8, c=3, out=b: L.dbx_patch_warp(   # noqa: E731
        V(patches) if patches else None, V(params) if params else None, V(inv) if inv else None, V(count) if count else None, n, c,
        V(out) if out else None, None)
    for k in ('patches', 'params', 'inv', 'out'):
        _refused(call(**{k: None}), 'null argument')
    _refused(call(count=None), 'null count')
    for c in (0, 5, -1):
        _refused(call(c=c), 'c=%d' % c)
    for n in (0, 4097, -1):
        _refused(call(n=n), 'n=%d' % n)
    for out in (a, a + 1, a + 8 * size - 1, a - 8 * size + 1):
        _refused(call(out=out), 'overlap')
    # the host function: the same checks for one patch
    patch, rec, eye = np.zeros((240, 240, 3), np.uint8), W.to_row(W.record()), np.array(W.EYE)
    res = np.zeros_like(patch)
    _refused(L.dbx_patch_warp_host(p(patch), p(rec), p(eye), 3, p(patch)), 'overlap')
    _refused(L.dbx_patch_warp_host(None, p(rec), p(eye), 3, p(res)), 'null argument')
    _refused(L.dbx_patch_warp_host(p(patch), None, p(eye), 3, p(res)), 'null argument')
    _refused(L.dbx_patch_warp_host(p(patch), p(rec), None, 3, p(res)), 'null argument')
    _refused(L.dbx_patch_warp_host(p(patch), p(rec), p(eye), 5, p(res)), 'c=5')
    assert L.dbx_patch_warp_host(p(patch), p(rec), p(eye), 3, p(res)) == 0


def test_params_host_refuses_a_bad_count_and_null_pointers():
    L = _lib.lib()
    bank = W.rot_bank(-15, 15)
    rows, out, tail = _host_args(2)
    for count in (-1, 4097):
        _refused(L.dbx_patch_warp_params_host(C.byref(_cfg()), 0, 0, None, p(bank), p(rows), count, *tail[2:]), 'count=')
    _refused(L.dbx_patch_warp_params_host(C.byref(_cfg()), 0, 0, None, p(bank), None, 2, *tail[2:]), 'null argument')
    _refused(L.dbx_patch_warp_params_host(C.byref(_cfg()), 0, 0, None, p(bank), p(rows), 2, *(tail[2:8] + [None])), 'null argument')
    _refused(L.dbx_patch_warp_params_host(None, 0, 0, None, p(bank), *tail), 'null cfg')
    assert L.dbx_patch_warp_params_host(C.byref(_cfg()), 0, 0, None, p(bank), None, 0, *([None] * 7)) == 0


def test_the_default_warp_makes_the_documented_cfg_and_bank():
    w = data.Warp()
    f = w.cfg()
    assert {k: getattr(f, k) for k in W.CFG_DEFAULT} == W.CFG_DEFAULT and f.reserved == 0
    bank = w.bank()
    assert bank.dtype == np.int32 and bank.shape == (31, 2) and bank[15].tolist() == [65536, 0]
    assert bank[0].tolist() == [int(np.rint(np.cos(np.deg2rad(-15.0)) * 65536)), int(np.rint(np.sin(np.deg2rad(-15.0)) * 65536))]
    assert np.array_equal(bank, W.rot_bank(-15, 15))
    g = data.Warp(border='constant', fill=(1, 2, 3, 200), rotate=(0, 0), translate=2.5, jitter=0.25, margin=0).cfg()
    assert (g.border, g.fill, g.R, g.rot_lo, g.rot_hi, g.tx, g.ty, g.jitter, g.margin) == (0, W.pack_fill(1, 2, 3, 200), 1, 0, 0, 40, 40, 4, 0)
    i = data.Warp.identity(seed=3)
    assert i.cfg().p_warp == 0.0 and i.seed == 3 and i.bank().tolist() == [[65536, 0]]
    with pytest.raises(RuntimeError, match='border'):
        data.Warp(border='wrap')
    with pytest.raises(RuntimeError, match='whole degrees'):
        data.Warp(rotate=(-1.5, 2))


def test_python_front_end_refuses_what_the_library_refuses():
    with pytest.raises(RuntimeError, match='scale'):
        _lib.check(_lib.lib().dbx_patch_warp_plan(C.byref(_io(params_in=None)), C.byref(data.Warp(scale=(0.0, 1.0)).cfg()), 4, None))
    with pytest.raises(RuntimeError, match='p_warp'):
        _lib.check(_lib.lib().dbx_patch_warp_plan(C.byref(_io(params_in=None)), C.byref(data.Warp(p=1.01).cfg()), 4, None))
    with pytest.raises(RuntimeError, match='margin'):
        _lib.check(_lib.lib().dbx_patch_warp_plan(C.byref(_io(params_in=None)), C.byref(data.Warp(margin=120).cfg()), 4, None))
