"""The host layer that decides which packed weight image each launch reads, pinned against a recording of an earlier commit
(tests/golden/pack_manifest.json, written by tools/gen_pack_manifest_golden.py): the one-launch pack table as the device holds it, the
kernels a step launches, and the steady state of training -- no packing launch after the first step."""
import importlib.util
import json
import os

import pytest
import torch

from conftest import GOLDEN, ROOT
from densebox_amd.optim import SGD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def recorder():
    spec = importlib.util.spec_from_file_location('gen_pack_manifest_golden', os.path.join(ROOT, 'tools', 'gen_pack_manifest_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def manifest():
    with open(os.path.join(GOLDEN, 'pack_manifest.json')) as f:
        return json.load(f)


def test_recording_covers_the_fragment_order_images(manifest):
    """The batch-64 recordings are there for the fragment-order images (at the small shape every image is plain order).  They hold mode 5
    (the image dbx_heads1_dgrad_gen reads) and NO mode 4: the 8-phase kernels take every forward GEMM that the register-streamed-weights
    kernel used to, so no default plan packs a forward image in fragment order.  Mode 4 is NOT covered by this file."""
    big = [c for name, c in manifest['configs'].items() if '@' in name]
    assert len(big) == 6
    modes = {r[6] for c in big for r in manifest['lists'][c['jobs']]['rows']}
    assert modes == {0, 1, 2, 5}, modes


@pytest.mark.parametrize('dtype', ['f16', 'bf16', 'f32'])
@pytest.mark.parametrize('kind', ['DenseBox', 'DenseBoxLM', 'DenseBoxLMLOC'])
def test_pack_table_and_launches_equal_the_recording(recorder, manifest, kind, dtype):
    got = recorder.record(kind, dtype)
    want = {name: c for name, c in manifest['configs'].items() if name.startswith('%s/%s/' % (kind, dtype))}
    assert list(got) == list(want) and len(got) == (13 if dtype != 'f32' else 12)
    for name, c in got.items():
        for what, v in c.items():
            ref = manifest['lists'][want[name][what]]
            v = json.loads(json.dumps(v))
            if what == 'jobs':
                assert v['max_elems'] == ref['max_elems'], name
                v, ref = v['rows'], ref['rows']
            assert len(v) == len(ref) and len(v) > 0, (name, what, len(v), len(ref))
            for i, (a, b) in enumerate(zip(v, ref)):
                assert a == b, (name, what, i, a, b)


class _CountingLib:
    """engine.L with the packing entry points counted; everything else is the library's own attribute."""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in ('dbx_pack_weight', 'dbx_pack_multi'):
            return fn

        def counted(*args):
            self._calls.append(name)
            return fn(*args)
        return counted


@pytest.mark.parametrize('dtype', ['f16', 'bf16'])
@pytest.mark.parametrize('kind', ['DenseBox', 'DenseBoxLM', 'DenseBoxLMLOC'])
def test_no_packing_launch_after_the_first_training_step(recorder, kind, dtype, monkeypatch):
    """optim.SGD.step() emits every packed image the next step reads (dbx_sgd_pack_step): with hash dropout, steps 2 and 3 launch neither
    dbx_pack_multi nor a single-image dbx_pack_weight.  An image a call site fetches but the table does not hold would show here as one
    dbx_pack_weight per step."""
    monkeypatch.setenv('DBX_SGD_PACK', '1')
    net = recorder.make_net(kind).train()
    net.compute_dtype = dtype
    assert net.dropout_masks is None
    x, bbox, vert, lab, rn, lrn = recorder.golden_batch(kind)
    opt = SGD(net.parameters(), lr=1e-9, momentum=0.9, weight_decay=5e-8)
    eng = net.engine()
    calls = []
    eng.L = _CountingLib(eng.L, calls)
    per_step = []
    for _ in range(3):
        del calls[:]
        opt.zero_grad()
        loss = net.loss(net(x), bbox, vert, lab, rand_neg_indices=rn, lm_rand_neg_indices=lrn)
        loss.backward()
        opt.step()
        per_step.append(list(calls))
    torch.cuda.synchronize()
    assert eng.last_plan.drop_hash
    print('packing launches per step:', per_step)
    assert per_step[0] == ['dbx_pack_multi']
    assert per_step[1] == [] and per_step[2] == []
