#!/usr/bin/env python
"""Records which packed weight images the engine's one-launch pack table holds, and which kernels a step launches, as the fixture
tests/golden/pack_manifest.json (data only).  Needs the GPU.

    python tools/gen_pack_manifest_golden.py [--out tests/golden/pack_manifest.json]

Run it on the commit whose behaviour is to be kept; tests/test_hip_pack_manifest.py replays record() on the current code and requires
equality.  Per configuration -- every KIND x {f16, bf16, f32} x {train, eval} x {default, each of SWITCHES}, at the shape of
tests/golden/train_<KIND>.npz -- it stores

  jobs     the dbx_pack_multi table as the device holds it after Engine.plan() + Engine._prepare_weights(), one row per job:
           [source parameter name, destination ordinal by first appearance, destination bytes, co, ci, taps, mode, ktot, cin_pad, row_off,
           k_off, rows_lim], and the launch's max_elems
  profile  the ordered [kernel, flops] list of Engine.profile over one training step (forward, loss, backward) / one eval forward

and the job table alone of a 16-bit training plan at batch 64 of 240x240: only there do the register-streamed kernels, and with them the
fragment-order images (pack modes 4 and 5), qualify.  Equal lists are stored once (`lists`) and referred to by index."""
import argparse
import contextlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import densebox_amd as D                                     # noqa: E402
from densebox_amd import _lib, labels as LB, synth          # noqa: E402

KINDS = ('DenseBox', 'DenseBoxLM', 'DenseBoxLMLOC')
DTYPES = ('f16', 'bf16', 'f32')
# the switches Python reads on every call (the library caches its own per process: left alone)
SWITCHES = (None, ('DBX_LIN_BWD', '0'), ('DBX_HEADS_FUSED', '0'), ('DBX_REFINE_LINEAR', '0'), ('DBX_HEADS_GEN', '0'), ('DBX_F32_LIN', '1'))
BIG = (64, 240, 240)
JOB = np.dtype([('src', '<u8'), ('dst', '<u8'), ('co', '<i4'), ('ci', '<i4'), ('taps', '<i4'), ('mode', '<i4'), ('ktot', '<i8'),
                ('cin_pad', '<i4'), ('row_off', '<i4'), ('k_off', '<i4'), ('rows_lim', '<i4')])
assert JOB.itemsize == 56


@contextlib.contextmanager
def switch(sw):
    names = [s[0] for s in SWITCHES if s]
    saved = {k: os.environ.pop(k, None) for k in names}
    if sw:
        os.environ[sw[0]] = sw[1]
    try:
        yield
    finally:
        for k in names:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def make_net(kind):
    net = getattr(D, kind)(synth.vgg19_standin(seed=0))
    synth.fill_params_(net, 11)
    return net.cuda()


def golden_batch(kind):
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'train_%s.npz' % kind), allow_pickle=False)
    n = int(g['batch'])
    x, bbox, vert, lab = synth.synth_batch(n, seed=7, neg_frac=0.0)
    _, half = LB.neg_counts(int(LB.positive_count(bbox, lab).sum()), n)
    rn = synth.synth_rand_neg_indices(n, half, seed=1)
    lrn = None if kind == 'DenseBox' else synth.synth_rand_neg_indices(4 * n, 1, seed=2).reshape(4, n, 1)
    return x.cuda(), bbox, vert, lab, rn, lrn


def pack_jobs(net, dtype, train, n, h, w):
    """A fresh engine's pack table for this plan, read back from the device, pointers normalised."""
    net._engine = None
    net.train(train)
    net.compute_dtype = dtype
    eng = net.engine()
    dt = _lib.DTYPE_ID[dtype]
    P = eng.plan(n, h, w, dt, torch.device('cuda', torch.cuda.current_device()), train)
    eng._prepare_weights(dt, train, P)
    torch.cuda.synchronize()
    (tab,) = eng._tables.values()
    rec = np.frombuffer(tab[0].cpu().numpy().tobytes(), dtype=JOB)
    assert len(rec) == tab[1]
    names = {p.data_ptr(): k for k, p in net.named_parameters()}
    sizes = {t.data_ptr(): t.numel() * t.element_size() for cache in (eng.wcache, eng.bias_cache) for _, t in cache.values()
             if torch.is_tensor(t)}
    dst, rows = {}, []
    for r in rec:
        d = int(r['dst'])
        dst.setdefault(d, len(dst))
        rows.append([names[int(r['src'])], dst[d], sizes[d]] + [int(r[f]) for f in JOB.names[2:]])
    return {'max_elems': int(tab[2]), 'rows': rows}


def step_profile(net, train, batch):
    """[kernel, flops] of every launch the engine brackets, over one training step / one eval forward of the engine pack_jobs() left."""
    x, bbox, vert, lab, rn, lrn = batch
    eng = net.engine()
    eng.profile = []
    if train:
        for p in net.parameters():
            p.grad = None
        loss = net.loss(net(x), bbox, vert, lab, rand_neg_indices=rn, lm_rand_neg_indices=lrn)
        loss.backward()
    else:
        with torch.no_grad():
            net(x)
    torch.cuda.synchronize()
    prof, eng.profile = eng.profile, None
    return [[e['kernel'], float(e['flops'])] for e in prof]


def record(kind, dtype, net=None):
    """{configuration name: {'jobs': ..., 'profile': ...}} of one (KIND, dtype), in a fixed order."""
    net = make_net(kind) if net is None else net
    batch = golden_batch(kind)
    n, _, h, w = batch[0].shape
    out = {}
    for train in (True, False):
        for sw in SWITCHES:
            with switch(sw):
                name = '%s/%s/%s/%s' % (kind, dtype, 'train' if train else 'eval', '%s=%s' % sw if sw else 'default')
                out[name] = {'jobs': pack_jobs(net, dtype, train, n, h, w), 'profile': step_profile(net, train, batch)}
    if dtype != 'f32':
        with switch(None):
            out['%s/%s/train/default@%dx%dx%d' % ((kind, dtype) + BIG)] = {'jobs': pack_jobs(net, dtype, True, *BIG)}
    net._engine = None
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'pack_manifest.json'))
    args = ap.parse_args()
    lists, index, configs = [], {}, {}

    def intern(v):
        s = json.dumps(v)
        if s not in index:
            index[s] = len(lists)
            lists.append(v)
        return index[s]
    for kind in KINDS:
        net = make_net(kind)
        for dtype in DTYPES:
            for name, c in record(kind, dtype, net).items():
                configs[name] = {k: intern(v) for k, v in c.items()}
    modes = sorted({r[6] for name, c in configs.items() if '@' in name for r in lists[c['jobs']]['rows']})
    with open(args.out, 'w') as f:
        json.dump({'lists': lists, 'configs': configs}, f, separators=(',', ':'))
        f.write('\n')
    print('%d configurations, %d distinct lists, pack modes at batch %d: %s' % (len(configs), len(lists), BIG[0], modes))
    print('%s: %d bytes' % (args.out, os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
