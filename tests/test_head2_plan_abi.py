"""The C-ABI boundary of dbx_head2_backward_up_plan without a GPU: the symbol is declared, bound and exported with the ABI version still
13; the struct layouts are the documented ones; bad arguments are refused on the host with their code and message; the query follows no
pointer of a view (it runs on views whose ptr is NULL) and fills every field of its result."""
import ctypes as C
import os
import re
import subprocess

import pytest

from densebox_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'dbx_head2_backward_up_plan'


def _views(n=2, h=17, w=33, hs=9, ws=17, nh=4):
    return (_lib.View(None, n, h, w, 0, 512 * nh, 0, 512 * nh), _lib.View(None, n, hs, ws, 1, 512 * nh, 0, 512 * nh))


def test_symbol_is_declared_bound_and_exported_without_a_version_bump():
    header = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    lib = _build.build(verbose=False)
    L = _lib.lib()
    exported = subprocess.run(['nm', '-D', '--defined-only', lib], capture_output=True, text=True).stdout
    assert re.search(r'\b%s\s*\(' % NAME, code) and 'dbx_head2_up_plan_t' in code
    assert NAME in _lib.SIGNATURES and NAME not in _lib.MISSING and hasattr(L, NAME)
    assert re.search(r' T %s\b' % NAME, exported)
    assert L.dbx_version() == _lib.ABI_VERSION == 13 and '#define DBX_ABI_VERSION 13' in header


def test_struct_layouts_are_the_documented_ones():
    assert C.sizeof(_lib.Head2UpHalf) == 24 and C.sizeof(_lib.Head2UpLaunch) == 20 and C.sizeof(_lib.Head2UpPlan) == 140
    offs = {n: getattr(_lib.Head2UpHalf, n).offset for n, _ in _lib.Head2UpHalf._fields_}
    assert offs == dict(px_lo=0, px_n=4, own_lo=8, own_hi=12, ix_lo=16, ix_n=20)
    offs = {n: getattr(_lib.Head2UpLaunch, n).offset for n, _ in _lib.Head2UpLaunch._fields_}
    assert offs == dict(head0=0, heads=4, kj=8, groups=12, blocks=16)
    offs = {n: getattr(_lib.Head2UpPlan, n).offset for n, _ in _lib.Head2UpPlan._fields_}
    assert offs == dict(fused=0, halves=4, half=8, launches=56, launch=60)
    header = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    for word in ('dbx_head2_up_half 24 bytes', 'dbx_head2_up_launch 20 bytes', 'dbx_head2_up_plan_t 140 bytes', 'launches 56, launch 60'):
        assert word in header, word


def test_query_fills_every_field_and_overwrites_stale_ones():
    L = _lib.lib()
    hv, gv = _views()
    out = _lib.Head2UpPlan()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    assert L.dbx_head2_backward_up_plan(_lib.BF16, C.byref(hv), C.byref(gv), (C.c_int32 * 4)(1, 4, 4, 8), 4, C.byref(out)) == 0
    assert (out.fused, out.halves, out.launches) == (1, 2, 3)
    assert [(l.head0, l.heads, l.kj, l.groups, l.blocks) for l in out.launch] == [(0, 1, 1, 2, 4), (1, 2, 4, 2, 4), (3, 1, 8, 2, 4), (0, 0, 0, 0, 0)]
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    assert L.dbx_head2_backward_up_plan(_lib.F32, C.byref(hv), C.byref(gv), (C.c_int32 * 4)(1, 4, 4, 8), 4, C.byref(out)) == 0
    assert bytes(out) == bytes(C.sizeof(out))               # the two passes: all zero


@pytest.mark.parametrize('bad,code,word', [
    (dict(hid=None), -1, 'null argument'), (dict(dg=None), -1, 'null argument'), (dict(k=None), -1, 'null argument'),
    (dict(out=None), -1, 'null argument'), (dict(dtype=7), -3, 'unknown dtype'), (dict(nh=0), -1, 'nh in 1..4'), (dict(nh=5), -1, 'nh in 1..4'),
    (dict(nh=3), -1, '512*nh channels'), (dict(ks=(1, 4, 0, 8)), -1, 'k in 1..8'), (dict(ks=(1, 4, 9, 8)), -1, 'k in 1..8'),
    (dict(dg_n=3), -1, 'batch and channels'),
])
def test_bad_arguments_are_refused(bad, code, word):
    L = _lib.lib()
    hv, gv = _views()
    if 'dg_n' in bad:
        gv.n = bad['dg_n']
    ks = bad.get('ks', (1, 4, 4, 8))
    out = _lib.Head2UpPlan()
    args = [bad.get('dtype', _lib.BF16), None if 'hid' in bad else C.byref(hv), None if 'dg' in bad else C.byref(gv),
            None if 'k' in bad else (C.c_int32 * 4)(*ks), bad.get('nh', 4), None if 'out' in bad else C.byref(out)]
    rc = L.dbx_head2_backward_up_plan(*args)
    assert rc == code and word in L.dbx_last_error().decode(), (rc, L.dbx_last_error())
    with pytest.raises(RuntimeError, match=re.escape(word)):
        _lib.check(rc)
