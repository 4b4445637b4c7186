"""CPU-side checks of the patch sampler's C ABI: dbx_patch_plan_host (the kernel's own __host__ __device__ geometry) equals the Python
restatement bit for bit on the whole fixture; dbx_patch_draw equals the restatement's hash; the struct layouts are the header's;
every bad argument is refused on the host with DBX_ERR_ARG and a message; the float32 label outputs are what the reference's dataset
reads from a file name built from the int32 row."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patch_ref as R                                   # noqa: E402

from densebox_amd import _lib, data                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'patch_plan.npz')


def _host(kind, W, H, verts, d0, d1, radius=15.0, th=0):
    v = np.ascontiguousarray(np.asarray(verts, dtype=np.int32).reshape(-1, 8))
    g = _lib.PatchGeom()
    rc = _lib.lib().dbx_patch_plan_host(kind, W, H, v.ctypes.data_as(C.c_void_p) if len(v) else None, len(v), d0, d1, radius, th, C.byref(g))
    assert rc == 0, _lib.lib().dbx_last_error()
    return g.status, (g.x0, g.y0, g.x1, g.y1), list(g.labels)


def test_plan_host_equals_the_restatement_on_the_fixture():
    g = np.load(GOLDEN)
    bad = []
    for i in range(len(g['pos_status'])):
        W, H = (int(v) for v in g['pos_size'][i])
        d0, d1 = (float(v) for v in g['pos_draws'][i])
        got, want = _host(0, W, H, g['pos_verts'][i], d0, d1), R.positive(W, H, g['pos_verts'][i], d0, d1)
        if got != want or got[0] != g['pos_status'][i]:
            bad.append((i, got, want))
    assert not bad, bad[:3]
    for i in range(len(g['neg_status'])):
        W, H = (int(v) for v in g['neg_size'][i])
        cx, cy = (float(v) for v in g['neg_centre'][i])
        plates, th = g['neg_plates'][i][:g['neg_nplates'][i]], int(g['neg_th'][i])
        got, want = _host(1, W, H, plates, cx, cy, th=th), R.negative(W, H, plates, cx, cy, th)
        if got != want or got[0] != g['neg_status'][i]:
            bad.append((i, got, want))
    assert not bad, bad[:3]


def test_plan_host_other_radii_and_refused_inputs():
    rs = np.random.RandomState(5)
    for _ in range(300):
        W, H = int(rs.randint(60, 2000)), int(rs.randint(60, 1200))
        x, y, w, h = int(rs.randint(0, W - 30)), int(rs.randint(0, H - 20)), int(rs.randint(1, 30)), int(rs.randint(1, 20))
        verts = [x, y, x + w, y, x + w, y + h, x, y + h]
        d0, d1, radius = float(rs.uniform(-1, 1)), float(rs.uniform(-1, 1)), float(rs.choice([0.0, 1.5, 15.0, 40.0]))
        assert _host(0, W, H, verts, d0, d1, radius) == R.positive(W, H, verts, d0, d1, radius)
    assert _host(0, 640, 480, [-1, 200, 60, 200, 60, 230, 0, 230], 0.0, 0.0)[0] == 4
    assert _host(0, 640, 480, [0, 200, 60, 200, 60, 480, 0, 230], 0.0, 0.0)[0] == 4
    assert _host(0, 640, 480, [300, 200, 360, 200, 360, 230, 300, 230], float('nan'), 0.0)[0] == 2
    for centre in ((119.0, 300.0), (520.0, 300.0), (300.5, 300.0), (300.0, 360.0), (float('nan'), 300.0)):
        assert _host(1, 640, 480, [], *centre)[0] == 5 == R.negative(640, 480, [], *centre)[0]
    assert _host(1, 240, 480, [], 120.0, 200.0)[0] == 5
    assert _host(1, 640, 480, [], 519.0, 359.0) == (0, (399, 239, 639, 479), [0] * 12)


def test_draw_equals_the_restatement_hash():
    L = _lib.lib()
    rs = np.random.RandomState(11)
    pairs = 0
    for seed, counter in [(0, 0), (0, 1), (1, 0), (-1, 7), (2 ** 63 - 1, 2 ** 40), (12345, 99)] + \
            [(int(rs.randint(0, 2 ** 31)), int(rs.randint(0, 2 ** 31))) for _ in range(94)]:
        i0 = int(rs.randint(0, 4096 - 1000))
        out = np.zeros((1000, 4), np.uint64)
        assert L.dbx_patch_draw(seed, counter, i0, 1000, out.ctypes.data_as(C.c_void_p)) == 0
        want = np.array([[R.draw_hash(seed, counter, i0 + r, j) for j in range(4)] for r in range(1000)], dtype=np.uint64)
        assert np.array_equal(out, want), (seed, counter)
        pairs += 1000
        u = -1.0 + 2.0 * ((out >> np.uint64(11)).astype(np.float64) * 2.0 ** -53)
        assert u.min() >= -1.0 and u.max() < 1.0
        assert np.array_equal(u[:, 2], [R.uniform(int(h)) for h in out[:, 2]])
        k = (out >> np.uint64(11)) % np.uint64(1920 - 240)
        assert k.max() < 1680 and (120 + k).max() < 1920 - 120
    assert pairs >= 100000
    # the 53-bit draws cover their range evenly enough to rule out a stuck bit
    assert 0.45 < (u < 0).mean() < 0.55 and len(np.unique(out)) == out.size


def _header_struct(name):
    src = open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read()
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), src, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r'(const\s+)?(\w+)\s*(\*?)\s*(.*)', decl)
        ctype, star, names = m.group(2), m.group(3), m.group(4)
        for nm in names.split(','):
            nm = nm.strip()
            arr = re.match(r'(\w+)\[(\d+)\]', nm)
            fields.append((arr.group(1) if arr else nm.lstrip('*'), ctype, bool(star) or nm.startswith('*'), int(arr.group(2)) if arr else 0))
    return fields


@pytest.mark.parametrize('name,cls,size', [('dbx_patch_job', _lib.PatchJob, 96), ('dbx_patch_geom', _lib.PatchGeom, 72),
                                           ('dbx_patch_plan_io', _lib.PatchPlanIO, 136)])
def test_struct_layouts_match_the_header(name, cls, size):
    scalar = {'int32_t': C.c_int32, 'double': C.c_double, 'float': C.c_float, 'int64_t': C.c_int64, 'uint8_t': C.c_uint8}
    fields = _header_struct(name)
    assert [f[0] for f in fields] == [f[0] for f in cls._fields_]
    for (nm, ctype, is_ptr, arr), (_, binding) in zip(fields, cls._fields_):
        want = C.c_void_p if is_ptr else (scalar[ctype] * arr if arr else scalar[ctype])
        assert C.sizeof(want) == C.sizeof(binding), nm
    assert C.sizeof(cls) == size
    doc = re.sub(r'\s+', ' ', open(os.path.join(ROOT, 'include', 'densebox_hip.h')).read())
    if name == 'dbx_patch_job':
        for nm, off in re.findall(r'(\w+) (\d+)', re.search(r'dbx_patch_job \(96 bytes.*?reserved 92', doc).group(0).split(':', 1)[1]):
            if hasattr(cls, nm):
                assert getattr(cls, nm).offset == int(off), nm
        assert cls.frame.offset == 84 and cls.tiles_x.offset == 80 and cls.scale_x.offset == 16
    if name == 'dbx_patch_geom':
        assert (cls.status.offset, cls.x0.offset, cls.labels.offset, cls.reserved.offset) == (0, 4, 20, 68)


def _io(**over):
    io = _lib.PatchPlanIO()
    for k, _ in _lib.PatchPlanIO._fields_:
        setattr(io, k, 0x1000)
    for k, v in over.items():
        setattr(io, k, v)
    return io


def _plan_rc(io=None, n_frames=2, n_plates=3, c=3, M=8, n=4, neg_frac=0.1, radius=15.0, th=0):
    return _lib.lib().dbx_patch_plan(C.byref(io) if io is not None else None, n_frames, n_plates, c, M, n, neg_frac, radius, th, None)


PLAN_REFUSALS = [
    ('null io', dict(io=None)), ('M negative', dict(M=-1)), ('M above 4096', dict(M=4097)), ('n zero', dict(n=0)),
    ('c zero', dict(c=0)), ('c five', dict(c=5)), ('neg_frac negative', dict(neg_frac=-0.01)), ('neg_frac above one', dict(neg_frac=1.01)),
    ('neg_frac nan', dict(neg_frac=float('nan'))), ('no frames', dict(n_frames=0)), ('negative plates', dict(n_plates=-1)),
    ('radius negative', dict(radius=-1.0)), ('radius infinite', dict(radius=float('inf'))), ('th negative', dict(th=-1)),
] + [('null ' + k, dict(io=_io(**{k: None}))) for k, _ in _lib.PatchPlanIO._fields_ if k not in ('cand', 'draws', 'state')] + [
    ('cand without draws', dict(io=_io(draws=None))), ('draws without cand', dict(io=_io(cand=None))),
    ('device mode without state', dict(io=_io(cand=None, draws=None, state=None))),
]


@pytest.mark.parametrize('what,kw', PLAN_REFUSALS, ids=[w for w, _ in PLAN_REFUSALS])
def test_plan_refuses_bad_arguments_before_any_launch(what, kw):
    kw = dict(kw)
    kw.setdefault('io', _io())
    assert _plan_rc(**kw) == -1, what
    assert b'patch_plan' in _lib.lib().dbx_last_error()


def test_cut_host_draw_and_tables_refuse_bad_arguments():
    L = _lib.lib()
    p = C.c_void_p(0x1000)
    for args in [(None, p, 4, 3, p), (p, None, 4, 3, p), (p, p, 4, 3, None), (p, p, 0, 3, p), (p, p, -1, 3, p), (p, p, 4, 0, p),
                 (p, p, 4, 5, p), (p, p, (1 << 24) // 60 + 1, 3, p)]:
        assert L.dbx_patch_cut(*args, None) == -1 and b'patch_cut' in L.dbx_last_error(), args
    v = (C.c_int32 * 8)(300, 200, 360, 200, 360, 230, 300, 230)
    g = _lib.PatchGeom()
    for args in [(2, 640, 480, v, 1, 0.0, 0.0, 15.0, 0, C.byref(g)), (0, 640, 480, v, 2, 0.0, 0.0, 15.0, 0, C.byref(g)),
                 (0, 0, 480, v, 1, 0.0, 0.0, 15.0, 0, C.byref(g)), (0, 640, 480, None, 1, 0.0, 0.0, 15.0, 0, C.byref(g)),
                 (0, 640, 480, v, 1, 0.0, 0.0, 15.0, 0, None), (1, 640, 480, v, -1, 300.0, 300.0, 15.0, 0, C.byref(g)),
                 (1, 640, 480, v, 1, 300.0, 300.0, 15.0, -1, C.byref(g)), (0, 640, 480, v, 1, 0.0, 0.0, -2.0, 0, C.byref(g))]:
        assert L.dbx_patch_plan_host(*args) == -1 and b'patch_plan_host' in L.dbx_last_error(), args
    assert L.dbx_patch_draw(0, 0, 0, 1, None) == -1 and L.dbx_patch_draw(0, 0, -1, 1, p) == -1 and L.dbx_patch_draw(0, 0, 0, -1, p) == -1
    assert b'patch_draw' in L.dbx_last_error()

    def tables(plates, plate0, n_frames, cand=None):
        pl = np.ascontiguousarray(np.asarray(plates, dtype=np.int32).reshape(-1, 9))
        p0 = np.asarray(plate0, dtype=np.int32)
        cd = np.ascontiguousarray(np.asarray(cand, dtype=np.int32).reshape(-1, 2)) if cand is not None else None
        rc = L.dbx_patch_check_tables(pl.ctypes.data_as(C.c_void_p), len(pl), p0.ctypes.data_as(C.c_void_p), n_frames,
                                      cd.ctypes.data_as(C.c_void_p) if cd is not None else None, len(cd) if cd is not None else 0)
        return rc, L.dbx_last_error()
    row = lambda f: [f, 1, 1, 9, 1, 9, 5, 1, 5]
    assert tables([row(0), row(0), row(2)], [0, 2, 2, 3], 3)[0] == 0
    rc, msg = tables([row(0), row(2), row(1)], [0, 1, 2, 3], 3)
    assert rc == -1 and b'not sorted by frame' in msg
    assert tables([row(0), row(3)], [0, 1, 1, 2], 3)[0] == -1                      # a frame that does not exist
    assert tables([row(0), row(1)], [0, 1, 1, 2], 3)[0] == -1                      # plate0 is not the prefix
    assert tables([row(0), row(1)], [0, 1, 2, 2], 3, [[0, 1], [1, 2]])[0] == 0
    for cand in ([[0, 2]], [[0, -1]], [[1, 3]], [[1, -1]], [[2, 0]]):
        rc, msg = tables([row(0), row(1)], [0, 1, 2, 2], 3, cand)
        assert rc == -1 and b'candidate 0' in msg, cand
    with pytest.raises(RuntimeError, match='not sorted by frame'):
        data.plate_tables(np.array([row(1), row(0)], dtype=np.int32), 2)
    rows, plate0 = data.plate_tables([[row(0)[1:]], [], [row(0)[1:], row(0)[1:]]], 3)
    assert rows[:, 0].tolist() == [0, 2, 2] and plate0.tolist() == [0, 1, 1, 3]


def test_float_labels_are_what_the_dataset_reads_from_the_file_name():
    g = np.load(GOLDEN)
    keep = np.nonzero(g['pos_status'] == 0)[0]
    sizes = [(int(h), int(w)) for w, h in g['pos_size'][keep]]
    plates = np.concatenate([np.arange(len(keep), dtype=np.int32)[:, None], g['pos_verts'][keep]], axis=1)
    cand = np.stack([np.zeros(len(keep), np.int32), np.arange(len(keep), dtype=np.int32)], axis=1)
    p = R.plan(sizes, plates, np.arange(len(keep) + 1), len(keep), len(keep) + 1, cand=cand, draws=g['pos_draws'][keep])
    assert p['count'] == len(keep) and np.array_equal(p['labels'], g['pos_labels'][keep])
    rows = np.concatenate([p['labels'], np.zeros((1, 12), np.int32)])              # and one negative
    bbox, vertices, labels = data.collate_labels([R.label_name(r) for r in rows])
    f32 = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert np.array_equal(f32(bbox.numpy()), f32((rows[:, :4] / 4.0).astype(np.float32)))
    assert np.array_equal(f32(bbox.numpy()[:-1]), f32(p['bbox'])) and np.array_equal(f32(vertices.numpy()[:-1]), f32(p['vertices']))
    assert labels.numpy().reshape(-1).tolist() == [1.0] * len(keep) + [0.0]
