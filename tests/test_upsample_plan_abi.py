"""The C-ABI boundary of dbx_upsample_bilinear_bwd_plan without a GPU: the symbol is declared, bound and exported with the ABI version
still 13; the struct layout is the documented one; bad arguments are refused on the host with their code and message; the query follows
no pointer of a view (it runs on views whose ptr is NULL) and fills every field of its result."""
import ctypes as C
import os
import re
import subprocess

import pytest

from densebox_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'dbx_upsample_bilinear_bwd_plan'


def _views(n=1, h=11, w=49, hs=6, ws=25, c=512):
    """(dy, dx): the gradient of the up-sampled map on pad 0 and of its source on pad 1."""
    return (_lib.View(None, n, h, w, 0, c, 0, c), _lib.View(None, n, hs, ws, 1, c, 0, c))


def test_symbol_is_declared_bound_and_exported_without_a_version_bump():
    header = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    lib = _build.build(verbose=False)
    L = _lib.lib()
    exported = subprocess.run(['nm', '-D', '--defined-only', lib], capture_output=True, text=True).stdout
    assert re.search(r'\b%s\s*\(' % NAME, code) and 'dbx_upsample_bwd_plan_t' in code
    assert NAME in _lib.SIGNATURES and NAME not in _lib.MISSING and hasattr(L, NAME)
    assert re.search(r' T %s\b' % NAME, exported)
    assert L.dbx_version() == _lib.ABI_VERSION == 13 and '#define DBX_ABI_VERSION 13' in header
    assert re.search(r'also at 13, without a bump: dbx_upsample_bwd_plan_t, %s' % NAME, header)
    assert '`%s`' % NAME in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_struct_layout_is_the_documented_one():
    assert C.sizeof(_lib.UpsampleBwdPlan) == 16
    offs = {n: getattr(_lib.UpsampleBwdPlan, n).offset for n, _ in _lib.UpsampleBwdPlan._fields_}
    assert offs == dict(kernel=0, nseg=4, workgroups=8, lds_bytes=12)
    header = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    for word in ('dbx_upsample_bwd_plan_t 16 bytes', 'kernel 0, nseg 4, workgroups 8'):
        assert word in header, word
    assert re.search(r'lds_bytes\s+\*?\s*12\)', header)


def test_the_flat_forward_kernel_is_gone():
    """Nothing launched upsample_kernel<T> (dbx_upsample_bilinear always takes upsample_rows_kernel): the dead kernel is deleted, and the
    backward dispatcher decides through the helper the query reports."""
    src = open(os.path.join(ROOT, 'densebox_amd', 'csrc', 'aux_ops.hip')).read()
    assert not re.search(r'\bupsample_kernel\b', src)
    assert len(re.findall(r'\bupsample_bwd_plan\(', src)) == 3          # its definition, the dispatcher, the query


def test_query_fills_every_field_and_overwrites_stale_ones():
    L = _lib.lib()
    dy, dx = _views()
    out = _lib.UpsampleBwdPlan()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    assert L.dbx_upsample_bilinear_bwd_plan(_lib.BF16, C.byref(dy), C.byref(dx), C.byref(out)) == 0
    assert (out.kernel, out.nseg, out.workgroups, out.lds_bytes) == (2, 3, 9, 49 * 12)          # the walk: 3 pairs x 3 segments
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    assert L.dbx_upsample_bilinear_bwd_plan(_lib.F32, C.byref(dy), C.byref(dx), C.byref(out)) == 0
    assert (out.kernel, out.nseg, out.workgroups, out.lds_bytes) == (2, 3, 9, 49 * 12)          # 128 groups of 4 floats
    dy, dx = _views(c=504)                                                                      # 63 groups of 8: the tabulated rows
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    assert L.dbx_upsample_bilinear_bwd_plan(_lib.F16, C.byref(dy), C.byref(dx), C.byref(out)) == 0
    assert (out.kernel, out.nseg, out.workgroups, out.lds_bytes) == (1, 0, 6, 25 * 36)
    dy, dx = _views(h=9, w=17, hs=3, ws=5, c=16)                                                # up-sampling by 4: the flat gather
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    assert L.dbx_upsample_bilinear_bwd_plan(_lib.F16, C.byref(dy), C.byref(dx), C.byref(out)) == 0
    assert (out.kernel, out.nseg, out.workgroups, out.lds_bytes) == (0, 0, 1, 0)


@pytest.mark.parametrize('bad,code,word', [
    (dict(dy=None), -1, 'null argument'), (dict(dx=None), -1, 'null argument'), (dict(out=None), -1, 'null argument'),
    (dict(dtype=7), -3, 'unknown dtype'), (dict(dtype=-1), -3, 'unknown dtype'), (dict(dx_n=3), -1, 'one batch and channel count'),
    (dict(dx_c=256), -1, 'one batch and channel count'), (dict(c=12), -1, 'multiple of 16 bytes'), (dict(dx_h=0), -1, 'every extent >= 1'),
])
def test_bad_arguments_are_refused(bad, code, word):
    L = _lib.lib()
    dy, dx = _views(c=bad.get('c', 512))
    for k in ('n', 'c', 'h'):
        if 'dx_' + k in bad:
            setattr(dx, k, bad['dx_' + k])
    out = _lib.UpsampleBwdPlan()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    args = [bad.get('dtype', _lib.BF16), None if 'dy' in bad else C.byref(dy), None if 'dx' in bad else C.byref(dx),
            None if 'out' in bad else C.byref(out)]
    rc = L.dbx_upsample_bilinear_bwd_plan(*args)
    assert rc == code and word in L.dbx_last_error().decode(), (rc, L.dbx_last_error())
    assert bytes(out) == b'\x5a' * C.sizeof(out)                      # a refused query writes nothing
    with pytest.raises(RuntimeError, match=re.escape(word)):
        _lib.check(rc)
