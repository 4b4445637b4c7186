"""The C-ABI boundary of the patch augmentation without a GPU: the symbols are declared, bound and exported with the ABI version still
13; the struct layouts are the documented ones; every bad argument is refused on the host with its code and message before any launch."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug_ref as A                                     # noqa: E402

from densebox_amd import _build, _lib, data             # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('dbx_patch_aug_plan', 'dbx_patch_augment', 'dbx_patch_aug_params_host', 'dbx_patch_augment_host', 'dbx_patch_plan_host')
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
    assert 'training patch augmentation' in header


def test_struct_layouts_are_the_documented_ones():
    assert C.sizeof(_lib.PatchAug) == 64 and C.sizeof(_lib.PatchAugCfg) == 112 and C.sizeof(_lib.PatchAugIO) == 72
    offs = {n: getattr(_lib.PatchAug, n).offset for n, _ in _lib.PatchAug._fields_}
    assert offs == dict(flags=0, blur=4, box_len=8, sat=12, contrast=16, brightness=20, curve=24, noise_amp=28, key_lo=32, key_hi=36, gain=40,
                        reserved=52)
    offs = {n: getattr(_lib.PatchAugCfg, n).offset for n, _ in _lib.PatchAugCfg._fields_}
    assert offs == dict(p_flip=0, p_blur=8, p_curve=16, p_noise=24, kind_w=32, box_lo=44, box_hi=48, sat_lo=52, sat_hi=56, contrast_lo=60,
                        contrast_hi=64, brightness_lo=68, brightness_hi=72, gain_lo=76, gain_hi=80, noise_lo=84, noise_hi=88, curve_lo=92,
                        curve_hi=96, G=100, reserved=104)
    assert [n for n, _ in _lib.PatchAugIO._fields_] == ['labels_in', 'count', 'params_in', 'state', 'params', 'labels', 'bbox', 'vertices',
                                                       'label']
    assert len(data.AUG_FIELDS) == len(A.FIELDS) == 16
    # the header's layout comment names the same offsets
    header = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    for word in ('dbx_patch_aug (64 bytes', 'dbx_patch_aug_cfg (112 bytes', 'kind_w 32', 'G 100', 'key_lo 32', 'gain 40'):
        assert word in header, word


def _io(**kw):
    io = _lib.PatchAugIO()
    for k, _ in _lib.PatchAugIO._fields_:
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
    (dict(p_flip=1.5), 'p_flip'), (dict(p_blur=-0.1), 'p_blur'), (dict(p_curve=float('nan')), 'p_curve'), (dict(p_noise=2.0), 'p_noise'),
    (dict(G=-1), 'G=-1'), (dict(curve_hi=4), 'leaves the bank'), (dict(curve_lo=-1), 'leaves the bank'), (dict(G=2), 'leaves the bank'),
    (dict(curve_lo=3, curve_hi=2), 'leaves the bank'),
    (dict(box_lo=4), 'box length'), (dict(box_hi=11), 'box length'), (dict(box_hi=8), 'box length'), (dict(box_lo=1), 'box length'),
    (dict(box_lo=7, box_hi=5), 'box length'),
    (dict(kind_w=(0, 0, 0)), 'blur kind weight'), (dict(kind_w=(1, -1, 1)), 'blur kind weight'),
    (dict(sat_lo=-1), 'saturation'), (dict(sat_lo=400), 'saturation'), (dict(contrast_hi=70000), 'contrast'), (dict(gain_lo=300), 'gain'),
    (dict(noise_hi=-2), 'noise amplitude'), (dict(brightness_lo=-256), 'brightness'), (dict(brightness_hi=256), 'brightness'),
]


def _cfg(**kw):
    cfg = dict(A.CFG_DEFAULT)
    cfg.update(kw)
    f = _lib.PatchAugCfg()
    for k, v in cfg.items():
        if k == 'kind_w':
            f.kind_w[:] = v
        else:
            setattr(f, k, v)
    return f


@pytest.mark.parametrize('bad,word', CFG_BAD, ids=[str(b) for b, _ in CFG_BAD])
def test_a_bad_cfg_is_refused_by_the_plan_and_by_the_host_function(bad, word):
    L = _lib.lib()
    _refused(L.dbx_patch_aug_plan(C.byref(_io()), C.byref(_cfg(**bad)), 4, None), word)
    rows = np.zeros((4, 12), np.int32)
    out = np.zeros((4, 16), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731
    _refused(L.dbx_patch_aug_params_host(C.byref(_cfg(**bad)), 0, 0, None, p(rows), 4, p(out), p(out), p(out), p(out), p(out)), word)
    assert not out.any()


def test_a_curve_range_outside_an_unused_bank_is_fine_and_an_empty_bank_too():
    rows, out = np.zeros((2, 12), np.int32), np.zeros((2, 16), np.int32)
    lab, f4, f8, f1 = np.ones((2, 12), np.int32), np.ones((2, 4), np.float32), np.ones((2, 8), np.float32), np.ones((2, 1), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731
    rc = _lib.lib().dbx_patch_aug_params_host(C.byref(_cfg(p_curve=0.0, G=0, curve_lo=0, curve_hi=0)), 3, 4, None, p(rows), 2, p(out), p(lab),
                                              p(f4), p(f8), p(f1))
    assert rc == 0 and (out[:, 6] == -1).all() and not lab.any() and not f1.any()


def test_plan_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    good = _cfg()
    _refused(L.dbx_patch_aug_plan(None, C.byref(good), 4, None), 'null io')
    _refused(L.dbx_patch_aug_plan(C.byref(_io()), None, 4, None), 'null cfg')
    for n in (0, -3, 4097):
        _refused(L.dbx_patch_aug_plan(C.byref(_io()), C.byref(good), n, None), 'n=%d' % n)
    for k in ('labels_in', 'count'):
        _refused(L.dbx_patch_aug_plan(C.byref(_io(**{k: None})), C.byref(good), 4, None), 'null input')
    _refused(L.dbx_patch_aug_plan(C.byref(_io(params_in=None, state=None)), C.byref(good), 4, None), 'null state')
    for k in ('params', 'labels', 'bbox', 'vertices', 'label'):
        _refused(L.dbx_patch_aug_plan(C.byref(_io(**{k: None})), C.byref(good), 4, None), 'null output')


def test_augment_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    V = C.c_void_p
    size = 240 * 240 * 3
    a, b = 0x40000000, 0x40000000 + 8 * size            # never followed
    call = lambda patches=a, params=0x1000, count=0x2000, curves=0x3000, G=4, n=8, c=3, out=b: L.dbx_patch_augment(   # noqa: E731
        V(patches) if patches else None, V(params) if params else None, V(count) if count else None, V(curves) if curves else None, G, n, c,
        V(out) if out else None, None)
    for k in ('patches', 'params', 'curves', 'out'):
        _refused(call(**{k: None}), 'null argument')
    _refused(call(count=None), 'null count')
    for c in (0, 5, -1):
        _refused(call(c=c), 'c=%d' % c)
    for n in (0, 4097, -1):
        _refused(call(n=n), 'n=%d' % n)
    _refused(call(G=-1), 'G=-1')
    for out in (a, a + 1, a + 8 * size - 1, a - 8 * size + 1):
        _refused(call(out=out), 'overlap')
    # the host function: the same checks for one patch
    patch, rec = np.zeros((240, 240, 3), np.uint8), A.to_row(A.record())
    p = lambda x: x.ctypes.data_as(V)                   # noqa: E731
    res = np.zeros_like(patch)
    _refused(L.dbx_patch_augment_host(p(patch), p(rec), None, 0, 3, p(patch)), 'overlap')
    _refused(L.dbx_patch_augment_host(p(patch), p(rec), None, 1, 3, p(res)), 'null argument')
    _refused(L.dbx_patch_augment_host(None, p(rec), None, 0, 3, p(res)), 'null argument')
    _refused(L.dbx_patch_augment_host(p(patch), None, None, 0, 3, p(res)), 'null argument')
    _refused(L.dbx_patch_augment_host(p(patch), p(rec), None, 0, 5, p(res)), 'c=5')
    _refused(L.dbx_patch_augment_host(p(patch), p(rec), None, -2, 3, p(res)), 'G=-2')
    assert L.dbx_patch_augment_host(p(patch), p(rec), None, 0, 3, p(res)) == 0


def test_params_host_refuses_a_bad_count_and_null_pointers():
    L = _lib.lib()
    rows, out = np.zeros((2, 12), np.int32), np.zeros((2, 16), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731
    for count in (-1, 4097):
        _refused(L.dbx_patch_aug_params_host(C.byref(_cfg()), 0, 0, None, p(rows), count, p(out), p(out), p(out), p(out), p(out)), 'count=')
    _refused(L.dbx_patch_aug_params_host(C.byref(_cfg()), 0, 0, None, None, 2, p(out), p(out), p(out), p(out), p(out)), 'null argument')
    _refused(L.dbx_patch_aug_params_host(None, 0, 0, None, p(rows), 2, p(out), p(out), p(out), p(out), p(out)), 'null cfg')
    assert L.dbx_patch_aug_params_host(C.byref(_cfg()), 0, 0, None, None, 0, None, None, None, None, None) == 0


def test_plan_host_is_exported_for_the_cpu_suite():
    """dbx_patch_plan_host does for the plan what the two new host functions do for the augmentation."""
    g = _lib.PatchGeom()
    verts = (C.c_int32 * 8)(100, 100, 160, 100, 160, 120, 100, 121)
    assert _lib.lib().dbx_patch_plan_host(0, 640, 480, verts, 1, 0.0, 0.0, 15.0, 0, C.byref(g)) == 0 and g.status == 0
    assert list(g.labels)[:4] == [90, 89, 150, 149]     # org = (130 - 120, 111 - 42) = (10, 69): (121 - 69) / 84 * 240 = 148.6


def test_python_front_end_refuses_what_the_library_refuses():
    with pytest.raises(RuntimeError, match='box length'):
        _lib.check(_lib.lib().dbx_patch_aug_plan(C.byref(_io()), C.byref(data.Augment(box=(3, 8)).cfg()), 4, None))
    with pytest.raises(RuntimeError, match='p_flip'):
        _lib.check(_lib.lib().dbx_patch_aug_plan(C.byref(_io()), C.byref(data.Augment(flip=1.01).cfg()), 4, None))
