"""The launches of one forward, in issue order, held to a recording: models/engine.py chooses a kernel per layer (_Conv.route,
_Residual.route) and every kernel has one launcher; a change to either that adds, drops, swaps or reorders a launch, a weight pack
or a layout copy shows here as a diff against tests/golden/engine_launches.json.

The recording was taken from the engine as it stood before the routing moved into the two route functions, with `_forward_log`
below: the FIRST eager forward of an engine on a freshly folded weight bundle (so the weight packs are in it), fp16 (routing does not
look at which 16-bit type), at the two shapes of tests/test_gpu_engine_schedule.py -- (3, 256, 384) reaches the 40-wide and 20-wide
tile kinds and the K-split workspace -- with the default knobs and with the up2 epilogue and the band kernel switched off.  Per
forward it holds the ordered conv_exact.record_key tuples (+ the layout / merge passes and the two pack entry points by name) and the
number of torch ops that did work on a stream (engine_schedule.Recorder: cat, contiguous copies, zeros of a workspace, ...).  Host
issue order is deterministic."""
import argparse
import json
import os

import pytest
import torch

import conv_exact as cx
import engine_schedule as es
from offsetguided_amd import models
from offsetguided_amd.models import engine as E
from test_gpu_engine_schedule import DEFAULTS, PASSES

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'engine_launches.json')
PACKS = ('og_conv3x3_pack_w16', 'og_conv_band_pack_w16')
SHAPES = [(1, 128, 128), (3, 256, 384)]
KNOBS = [{}, {'CONV_UP2': 0, 'CONV_BAND_MAX_PIXELS': 0}]


def case_id(shape, knobs):
    return 'x'.join(map(str, shape)) + '/' + (','.join(f'{k}={v}' for k, v in knobs.items()) or 'default')


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    return torch.device("cuda:0")


def make_model(dev):
    import bench
    p = argparse.ArgumentParser()
    models.net_cli(p)
    m, _ = models.model_factory(p.parse_args(['--no-pretrain']))
    bench.bench_init(m, 1234)
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def model(dev):
    yield make_model(dev)
    E.invalidate_engine_cache()
    torch.cuda.empty_cache()


def _forward_log(model, dev, monkeypatch, shape, knobs):
    """-> (ordered launch keys as JSON would hand them back, number of torch ops that did work) of the first eager forward of a
    strict fp16 engine on a fresh weight bundle."""
    for k, v in {**DEFAULTS, **knobs}.items():
        monkeypatch.setattr(E, k, v)
    E.invalidate_engine_cache()
    eng = models.InferenceEngine(model, *shape, device=dev, dtype=torch.float16, use_graph=False)
    assert eng.strict
    x = torch.randn(shape[0], 3, *shape[1:], device=dev, generator=torch.Generator(dev).manual_seed(shape[2]))
    keys = []
    cx.record_launches(monkeypatch, keys.append, extra=PASSES + PACKS)
    rec = es.Recorder(monkeypatch, eng._layers)
    with rec.recording(dev):
        out = eng.forward_raw(x)
    torch.cuda.synchronize(dev)
    assert eng.torch_conv_calls == [] and all(bool(torch.isfinite(o).all()) for o in out)
    ops = [e.name for e in rec.log if isinstance(e, es.Launch) and e.name.startswith('torch.')]
    assert len(keys) == len([e for e in rec.log if isinstance(e, es.Launch)]) - len(ops)      # both recorders saw every launch
    return json.loads(json.dumps(keys)), len(ops)


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: case_id((), k)[1:])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_forward_issues_the_recorded_launches_in_order(dev, model, monkeypatch, shape, knobs):
    with open(GOLDEN) as f:
        want = json.load(f)[case_id(shape, knobs)]
    got, torch_ops = _forward_log(model, dev, monkeypatch, shape, knobs)
    exp = want['launches']
    assert len(exp) > 150
    first = next((i for i, (g, e) in enumerate(zip(got, exp)) if g != e), min(len(got), len(exp)))
    if got != exp:
        print(f'first difference at launch {first} of {len(got)} (recorded: {len(exp)}):\n  got      {got[first:first + 1]}\n'
              f'  recorded {exp[first:first + 1]}')
    assert got == exp, f'launch {first}: {got[first:first + 1]} != recorded {exp[first:first + 1]}'
    print(f'torch ops that did work: {torch_ops} (recorded: {want["torch_ops"]})')
    assert torch_ops == want['torch_ops']
