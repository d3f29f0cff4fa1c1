"""The schedule models/engine.py runs its kernels under -- up1 branches on side streams, trunk-first forks, the shared deep stream,
HIP-graph capture and replay, two engines in flight on two lanes -- held to a serial forward of the same launches, bit for bit.

The chain the comparison stands on:
  * every conv entry point is exact on exact operands (tests/test_gpu_conv_exact.py), the layer glue is exact against a CPU
    restatement (tests/test_gpu_engine_exact.py, eager, branches on) and the engine is within tolerance of the fp32 module
    (tests/test_gpu_backbone.py);
  * every kernel is run-to-run deterministic (the split-K last arriver sums the slabs in slice order) and the schedule knobs
    (BRANCHES, BRANCH_MAX_DEPTH, TRUNK_FIRST, DEEP_SHARED, CONV_WARM_NEXT) choose no kernel -- asserted here on the recorded launches;
  * hence the reference: the same model and dtype through InferenceEngine(use_graph=False) with BRANCHES = 0, everything on the
    caller's stream, and torch.equal on the bit patterns of every head.  The kernel-selecting knobs (CONV_UP2,
    CONV_BAND_MAX_PIXELS, CONV_TILED) are the same on both sides.
Every engine sees a different input on every replay (random, constant and 100x-scaled batches in turn): a consumer that runs ahead of
its producer reads the previous replay's activation, which is then far from the right one.

Part 1 proves the absence of a race only for the timings that occurred.  Part 2 does not depend on timing: the order in which an
eager forward issues launches, event records and waits is logged and checked for happens-before (tests/engine_schedule.py)."""
import argparse
from collections import Counter

import pytest
import torch

import conv_exact as cx
import engine_schedule as es
from offsetguided_amd import _lib, models
from offsetguided_amd.models import engine as E

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
SMALL, MID, BENCH = (1, 128, 128), (3, 256, 384), (8, 640, 640)
DEFAULTS = dict(BRANCHES=1, BRANCH_MAX_DEPTH=4, TRUNK_FIRST=2, DEEP_SHARED=3, CONV_WARM_NEXT=1,
                CONV_UP2=1, CONV_BAND_MAX_PIXELS=1024, CONV_TILED=7)
KERNEL_KNOBS = ('CONV_UP2', 'CONV_BAND_MAX_PIXELS', 'CONV_TILED')
# one schedule knob away from the default at a time (the defaults themselves are TRUNK_FIRST 2, DEEP_SHARED 3, BRANCH_MAX_DEPTH 4,
# CONV_WARM_NEXT 1), then the combinations of test_gpu_backbone.test_engine_schedule_knobs (its third, DEEP_SHARED = 2, is in the list)
GRID = [{}, {'TRUNK_FIRST': 0}, {'TRUNK_FIRST': 1}, {'DEEP_SHARED': 0}, {'DEEP_SHARED': 2}, {'BRANCH_MAX_DEPTH': 0}, {'CONV_WARM_NEXT': 0},
        {'CONV_UP2': 0, 'TRUNK_FIRST': 0}, {'TRUNK_FIRST': 1, 'CONV_BAND_MAX_PIXELS': 0, 'DEEP_SHARED': 0}]
PASSES = ('og_upsample2_add', 'og_bias_act', 'og_nchw_f32_to_nhwc', 'og_nhwc_bf16_to_nchw_f32', 'og_nhwc_f16_to_nchw_f32')


def _id(knobs):
    return '-'.join(f'{k}={v}' for k, v in knobs.items()) or 'default'


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    """model_factory + bench.bench_init with the heads at their real magnitude (test_gpu_backbone._bench_model)."""
    import bench
    p = argparse.ArgumentParser()
    models.net_cli(p)
    m, _ = models.model_factory(p.parse_args(['--no-pretrain']))
    bench.bench_init(m, 1234)
    for head in m.headnets:
        for c in head.modules():
            if isinstance(c, torch.nn.Conv2d):
                c.weight.data.mul_(1e4)
    yield m.to(dev).eval()
    _bases.clear()
    _refs.clear()
    torch.cuda.empty_cache()


def _set(monkeypatch, knobs):
    for k, v in {**DEFAULTS, **knobs}.items():
        monkeypatch.setattr(E, k, v)


_bases, _refs = {}, {}


def _engine(model, dev, shape, dtype, use_graph):
    """All engines of one dtype share one weight bundle (like=)."""
    eng = models.InferenceEngine(model, *shape, device=dev, dtype=dtype, use_graph=use_graph, like=_bases.get(dtype))
    _bases.setdefault(dtype, eng)
    assert eng._layers is _bases[dtype]._layers and eng.strict
    return eng


def _inputs(dev, shape):
    """Six batches: random, constant, random, 100 x random, random, constant."""
    g = torch.Generator(dev).manual_seed(shape[0] * 1000 + shape[2])
    r = [torch.randn(shape[0], 3, *shape[1:], device=dev, generator=g) for _ in range(4)]
    return [r[0], torch.full_like(r[0], 0.75), r[1], 100 * r[2], r[3], torch.full_like(r[0], -0.5)]


def _bits(t):
    return t.view(torch.int32)


def _launches(monkeypatch, forward):
    """-> (Counter of (entry point, integer arguments) over one call of forward(), its result)"""
    seen = Counter()
    with monkeypatch.context() as m:
        cx.record_launches(m, lambda key: seen.update([key]), extra=PASSES)
        out = forward()
    return seen, out


def _reference(model, dev, monkeypatch, shape, dtype, knobs=None):
    """(inputs, outputs of the serial forward, its launches): BRANCHES = 0, eager, on the current stream.  Computed once per (shape,
    dtype, kernel-selecting knobs), cloned, never written again."""
    kernel = {k: {**DEFAULTS, **(knobs or {})}[k] for k in KERNEL_KNOBS}
    key = (shape, dtype, tuple(kernel.items()))
    if key not in _refs:
        with monkeypatch.context() as m:
            _set(m, {**kernel, 'BRANCHES': 0})
            eng = _engine(model, dev, shape, dtype, use_graph=False)
            xs, outs = _inputs(dev, shape), []
            launches, first = _launches(m, lambda: eng.forward_raw(xs[0]))
            for i, x in enumerate(xs):
                outs.append([o.clone() for o in (first if i == 0 else eng.forward_raw(x))])
                torch.cuda.synchronize(dev)
        assert sum(launches.values()) > 150
        for a, b in zip(outs, outs[1:]):         # a stale activation has to show: no two inputs in a row give the same heads
            assert not any(torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b))
        _refs[key] = (xs, outs, launches)
    return _refs[key]


def _mismatch(got, exp):
    """'' or: the first differing head and the bounding box of the differing values."""
    assert len(got) == len(exp)
    for h, (g, e) in enumerate(zip(got, exp)):
        assert g.shape == e.shape and g.dtype == e.dtype == torch.float32
        if not torch.equal(_bits(g), _bits(e)):
            bad = (_bits(g) != _bits(e)).nonzero()
            return (f'head {h}: {len(bad)} of {g.numel()} values differ inside (n, c, y, x) = {bad.min(0).values.tolist()} .. '
                    f'{bad.max(0).values.tolist()}')
    return ''


def _assert_replays(outs, ref, what):
    for i, (got, exp) in enumerate(zip(outs, ref, strict=True)):
        bad = _mismatch(got, exp)
        assert not bad, f'{what}: replay {i} differs from the serial forward, {bad}'


def _replay_all(eng, xs, dev):
    """Every input through the engine back to back, the outputs cloned on the stream before the next replay overwrites them."""
    outs = [[o.clone() for o in eng.forward_raw(x)] for x in xs]
    torch.cuda.synchronize(dev)
    return outs


def _same_kernels(model, dev, monkeypatch, shape, dtype, knobs, ref):
    """The scheduled eager forward issues the multiset of (entry point, integer arguments) the serial reference issued, and gives
    its bits."""
    xs, outs, launches = ref
    eager = _engine(model, dev, shape, dtype, use_graph=False)
    seen, out = _launches(monkeypatch, lambda: eager.forward_raw(xs[0]))
    torch.cuda.synchronize(dev)
    assert seen == launches, f'{_id(knobs)}: launches differ from the serial forward: {(seen - launches) + (launches - seen)}'
    _assert_replays([out], outs[:1], f'eager {_id(knobs)} {shape}')
    return eager


# ---------------------------------------------------------------------------------------------- 1. scheduled == serial, bit for bit
@pytest.mark.parametrize("dtype", [F16, BF16], ids=['fp16', 'bf16'])
@pytest.mark.parametrize("shape", [SMALL, MID])
def test_graph_replays_equal_the_serial_forward(dev, model, monkeypatch, shape, dtype):
    ref = _reference(model, dev, monkeypatch, shape, dtype)
    _set(monkeypatch, {})
    _same_kernels(model, dev, monkeypatch, shape, dtype, {}, ref)
    eng = _engine(model, dev, shape, dtype, use_graph=True)
    _assert_replays(_replay_all(eng, ref[0], dev), ref[1], f'graph {shape} {dtype}')


def test_graph_replays_equal_the_serial_forward_at_the_bench_shape(dev, model, monkeypatch):
    """8 x 640 x 640, fp16: the only shape at which the side branches really overlap the deep levels they were scheduled against."""
    ref = _reference(model, dev, monkeypatch, BENCH, F16)
    _set(monkeypatch, {})
    eng = _engine(model, dev, BENCH, F16, use_graph=True)
    try:
        _assert_replays(_replay_all(eng, ref[0], dev), ref[1], 'graph 8 x 640 x 640 fp16')
    finally:
        del eng
        for k in [k for k in _refs if k[0] == BENCH]:
            _refs.pop(k)
        torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", [F16, BF16], ids=['fp16', 'bf16'])
@pytest.mark.parametrize("shape", [SMALL, MID])
def test_eager_branches_equal_the_serial_forward(dev, model, monkeypatch, shape, dtype):
    """use_graph=False with the branches on: the configuration tests/test_gpu_engine_exact.py stands on."""
    ref = _reference(model, dev, monkeypatch, shape, dtype)
    _set(monkeypatch, {})
    eng = _same_kernels(model, dev, monkeypatch, shape, dtype, {}, ref)
    _assert_replays(_replay_all(eng, ref[0], dev), ref[1], f'eager with branches {shape} {dtype}')


@pytest.mark.parametrize("knobs", GRID[1:], ids=_id)
def test_schedule_knobs_equal_the_serial_forward(dev, model, monkeypatch, knobs):
    ref = _reference(model, dev, monkeypatch, MID, F16, knobs)
    _set(monkeypatch, knobs)
    _same_kernels(model, dev, monkeypatch, MID, F16, knobs, ref)
    eng = _engine(model, dev, MID, F16, use_graph=True)
    _assert_replays(_replay_all(eng, ref[0], dev), ref[1], f'graph {_id(knobs)}')


def test_a_knob_that_selected_a_kernel_would_be_seen(dev, model, monkeypatch):
    """The launch comparison has teeth: against the default reference, a forward with a kernel-selecting knob moved differs."""
    xs, _, launches = _reference(model, dev, monkeypatch, MID, F16)
    _set(monkeypatch, {'CONV_BAND_MAX_PIXELS': 0})
    eager = _engine(model, dev, MID, F16, use_graph=False)
    seen, _ = _launches(monkeypatch, lambda: eager.forward_raw(xs[0]))
    torch.cuda.synchronize(dev)
    assert seen != launches and any(k[0] == 'conv_band' for k in launches - seen)


def _two_lanes(dev, engines, inputs, batches):
    """evaluate.run_images' pattern: batch i on lane i % 2 through engine i % 2, no host synchronisation in between; an engine's
    outputs are cloned on its lane before its next replay, which waits for the event recorded behind the clone (slot[2] there)."""
    lanes = _lib.lane_streams(dev, 2)
    cur = torch.cuda.current_stream(dev)
    done, outs = [None, None], []
    for i in range(batches):
        k = i % 2
        lanes[k].wait_stream(cur)
        if done[k] is not None:
            lanes[k].wait_event(done[k])
        with torch.cuda.stream(lanes[k]):
            outs.append([o.clone() for o in engines[k].forward_raw(inputs[k][i // 2])])
            done[k] = torch.cuda.Event()
            done[k].record(lanes[k])
    torch.cuda.synchronize(dev)
    return outs


@pytest.mark.parametrize("shapes", [(MID, MID), (SMALL, MID)], ids=['same-shape', 'two-shapes'])
def test_two_engines_in_flight_equal_the_serial_forward(dev, model, monkeypatch, shapes):
    """Engines A and B share one _Layers bundle, one set of _Level objects and their _side tables; twelve batches alternately."""
    refs = [_reference(model, dev, monkeypatch, s, F16) for s in shapes]
    _set(monkeypatch, {})
    engines = [_engine(model, dev, s, F16, use_graph=True) for s in shapes]
    # B sees the inputs in another order than A, so the two never work on the same input at the same time
    order = [list(range(6)), [3, 0, 5, 2, 1, 4]]
    inputs = [[refs[k][0][j] for j in order[k]] for k in (0, 1)]
    outs = _two_lanes(dev, engines, inputs, 12)
    for i, got in enumerate(outs):
        k = i % 2
        bad = _mismatch(got, refs[k][1][order[k][i // 2]])
        assert not bad, f'batch {i} (engine {"AB"[k]}, {shapes[k]}) differs from the serial forward, {bad}'


def test_engine_churn_then_equal_the_serial_forward(dev, model, monkeypatch):
    """Five graph engines of alternating shapes built and dropped (their warm-up and side streams go back through release_stream and
    the _side eviction), then a sixth one checked like the first test's."""
    ref = _reference(model, dev, monkeypatch, MID, F16)
    small = _reference(model, dev, monkeypatch, SMALL, F16)
    _set(monkeypatch, {})
    for i in range(5):
        eng = _engine(model, dev, (SMALL, MID)[i % 2], F16, use_graph=True)
        eng.forward_raw((small, ref)[i % 2][0][i])
        del eng
    eng = _engine(model, dev, MID, F16, use_graph=True)
    _assert_replays(_replay_all(eng, ref[0], dev), ref[1], 'graph engine after churn')


# --------------------------------------------------------------------------------------------------------- 2. issue-order audit
def _warm(eng, x, dev):
    """One forward before the log begins: weights are packed and scratch is sized there, not in the schedule under audit."""
    eng.forward_raw(x)
    torch.cuda.synchronize(dev)


def _recorded_forward(dev, model, monkeypatch, knobs):
    _set(monkeypatch, knobs)
    eng = _engine(model, dev, SMALL, F16, use_graph=False)
    x = _inputs(dev, SMALL)[0]
    _warm(eng, x, dev)
    rec = es.Recorder(monkeypatch, eng._layers)
    with rec.recording(dev):
        eng.forward_raw(x)
    torch.cuda.synchronize(dev)
    return rec


def _trunk(log):
    return next(e.stream for e in log if isinstance(e, es.Launch))


def _assert_clean(rec):
    findings = es.check(rec.log, rec.readonly)
    assert findings == ([], []), es.report(rec.log, findings)


@pytest.mark.parametrize("knobs", GRID, ids=_id)
def test_issue_order_is_race_free(dev, model, monkeypatch, knobs):
    rec = _recorded_forward(dev, model, monkeypatch, knobs)
    log, k = rec.log, {**DEFAULTS, **knobs}
    launches = [e for e in log if isinstance(e, es.Launch)]
    assert len(launches) > 150 and all(e.reads and e.writes for e in launches) and rec.readonly
    _assert_clean(rec)
    # the log is the forked forward: one join per forked level on the trunk, and as many streams as the knobs ask for
    forked = 2 * (min(k['BRANCH_MAX_DEPTH'], 4) + 1)
    shared = 5 - k['DEEP_SHARED'] if k['DEEP_SHARED'] and k['DEEP_SHARED'] <= k['BRANCH_MAX_DEPTH'] else 0
    assert len([e for e in log if isinstance(e, es.Wait) and e.stream == _trunk(log)]) == forked
    assert len({e.stream for e in launches}) == 1 + forked - (2 * shared - 1 if shared else 0)


def test_two_lanes_issue_order_is_race_free(dev, model, monkeypatch):
    """Eager engines A and B on the two lanes, four batches: their accesses are unordered -- the lanes do overlap -- and meet only on
    read-only bytes."""
    _set(monkeypatch, {})
    engines = [_engine(model, dev, s, F16, use_graph=False) for s in (SMALL, MID)]
    inputs = [_inputs(dev, s)[:2] for s in (SMALL, MID)]
    for eng, xs in zip(engines, inputs):
        _warm(eng, xs[0], dev)
    rec = es.Recorder(monkeypatch, engines[0]._layers)
    with rec.recording(dev):
        _two_lanes(dev, engines, inputs, 4)
    log = rec.log
    lanes = [s.cuda_stream for s in _lib.lane_streams(dev, 2)]
    on = [[i for i, e in enumerate(log) if isinstance(e, es.Launch) and e.stream == s] for s in lanes]
    assert len(on[0]) > 100 and len(on[1]) > 100
    # no stream serves both engines (models/engine.py: "two engines in flight must not serialise their branches on one stream")
    used = [{e.stream for e in log if isinstance(e, es.Launch) and e.label.startswith(f'engine {eng._id} ')} for eng in engines]
    assert len(used[0]) == len(used[1]) == 8 and not used[0] & used[1], sorted(used[0] & used[1])
    clocks = es._clocks(log)
    assert not es.happens_before(clocks, on[0][0], on[1][-1]) and not es.happens_before(clocks, on[1][0], on[0][-1])
    _assert_clean(rec)


DEPTH3, DEPTH4 = 'kps.0.low2.low2.low2', 'kps.0.low2.low2.low2.low2'


@pytest.mark.parametrize("knobs,level", [({'DEEP_SHARED': 0}, DEPTH3), ({}, DEPTH4)], ids=['own-streams-depth3', 'shared-stream-depth4'])
def test_a_join_taken_out_of_the_log_is_reported(dev, model, monkeypatch, knobs, level):
    """The audit has teeth, shown on the LOG of a correct forward, never on a schedule that runs: with the join of one level deleted
    the checker's one minimal finding is that level's last up1 launch against the merge the join guarded.  Depth 3 is taken from the
    log with every branch on its own stream: on the shared deep stream (the default) its join is implied by the join of depth 4,
    which the trunk passes first and whose event is recorded behind both branches -- there the load-bearing join is depth 4's."""
    rec = _recorded_forward(dev, model, monkeypatch, knobs)
    log = rec.log
    _assert_clean(rec)
    at = es.joins(log, level, _trunk(log))
    assert len(at) == 1, at
    cut = es.without(log, at[0])
    races, bad = es.check(cut, rec.readonly)
    assert races and not bad
    # every finding has the cut branch on its earlier side; of those that are no consequence of another, one ends on the trunk
    # (another stream that shares the branch's scratch in the second stack may lose its order too)
    assert len({cut[r.first].stream for r in races}) == 1 and cut[races[0].first].stream != _trunk(log)
    worst = [r for r in es.minimal(races, cut) if cut[r.second].stream == _trunk(log)]
    assert len(worst) == 1, es.report(cut, (worst, []))
    branch, merge = cut[worst[0].first], cut[worst[0].second]
    consumer = next(e for e in cut[at[0]:] if isinstance(e, es.Launch) and e.stream == _trunk(log)
                    and any(lo < w[1] and w[0] < hi for w in branch.writes for lo, hi in e.reads))
    assert merge is consumer and merge.name == 'og_upsample2_add' and merge.label.split(':')[0].endswith(level), es.describe(cut, worst[0])
    assert branch.stream != merge.stream and f'{level[4:]}.up1.' in branch.label, es.describe(cut, worst[0])
    assert merge.name in es.describe(cut, worst[0]) and branch.label in es.describe(cut, worst[0])
