"""GPU: the range report (include/og_decoder.h "range report", csrc/range.hip).  og_range_stats and og_range_probe word for word against
the numpy restatement (tests/range_common.py) on directed values, every length round a workgroup's chunk and every element offset off
a 16-byte boundary, between guards of inf and NaN, without a host wait; InferenceEngine(probe=True) against the tensors an eager
engine hands out; planted overflow / flush cases in activations and folded weights; evaluate.run_images --range-report."""
import contextlib
import json

import numpy as np
import pytest
import torch

import engine_refresh_common as rc
import range_common as rg
from offsetguided_amd import _lib, evaluate, models
from offsetguided_amd.models import engine as eng_mod, range_report

pytestmark = pytest.mark.gpu

TORCH = {'f32': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16}
PAIRS = [('f32', 'f16'), ('f32', 'bf16'), ('f16', 'f16'), ('bf16', 'bf16')]
GUARD = 16      # elements on either side of every view


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests selected but no HIP device is visible')
    _lib.load()
    return torch.device('cuda:0')


@contextlib.contextmanager
def no_host_wait():
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode('default')


def _place(bits, off, source, dev):
    """A device view of the elements `bits` that starts `off` elements past a 16-byte boundary, GUARD elements of inf and NaN on
    either side of it (a vector head or tail that read outside the view would count them) -> (buffer, view)."""
    wide = source == 'f32'
    inf, nan = (0x7f800000, 0x7fc00001) if wide else (rg.LP[source][0], rg.LP[source][0] | 1)
    guard = np.array([inf, nan | (0x80000000 if wide else 0x8000)] * (GUARD // 2), np.uint32 if wide else np.uint16)
    pad = np.zeros(off, guard.dtype) + guard[0]
    host = np.concatenate([guard, pad, bits.astype(guard.dtype), guard])
    base = torch.from_numpy(host.view(np.int32 if wide else np.int16)).to(dev).view(TORCH[source])
    view = base[GUARD + off:GUARD + off + bits.size]
    assert base.data_ptr() % 16 == 0 and (bits.size == 0 or view.data_ptr() % 16 == (off * view.element_size()) % 16)
    return base, view


def _bits(source, n, seed):
    """n patterns of the source type: the directed values first, seeded random patterns behind them."""
    rs = np.random.RandomState(seed)
    if source == 'f32':
        return np.concatenate([rg.directed32(), rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)])[:n]
    return np.concatenate([rg.directed16(source), rs.randint(0, 2 ** 16, n).astype(np.uint16)])[:n]


@pytest.mark.parametrize('source,target', PAIRS, ids=[f'{s}-to-{t}' for s, t in PAIRS])
def test_both_entry_points_word_for_word(dev, source, target):
    lib = _lib.load()
    chunk = lib.og_range_chunk_elems()
    per16 = 4 if source == 'f32' else 8
    lengths = [0, 1, 7, 8, 9, 200, chunk - 1, chunk, chunk + 1, 2 * chunk + 5]
    cases = [(n, off) for n in lengths for off in range(per16)]           # every length at every element offset of a 16-byte group
    data = [_bits(source, n, 10 * n + off) for n, off in cases]
    placed = [_place(b, off, source, dev) for b, (_, off) in zip(data, cases)]
    views = [v for _, v in placed]
    tiny = [_place(_bits(source, 1 + i % 13, 1000 + i)[::-1].copy(), i % per16, source, dev) for i in range(300)]
    t_dtype = TORCH[target]
    with no_host_wait():
        table = range_report.range_stats(views, t_dtype)
        probed = torch.zeros_like(table)
        for i, v in enumerate(views):
            range_report.probe(v, t_dtype, probed, i)
        many = range_report.range_stats([v for _, v in tiny], t_dtype)
        shared = range_report.range_stats(views[-3:], t_dtype, rows=[0, 0, 1])
        twice = range_report.range_stats(views, t_dtype, out=table.clone())
    table, probed, many, shared, twice = (t.cpu().numpy() for t in (table, probed, many, shared, twice))
    want = np.stack([rg.stats_ref(b, source, target) for b in data])
    for (n, off), got, ref in zip(cases, table, want):
        assert np.array_equal(got, ref), f'length {n}, offset {off}: {dict(zip(rg.NAMES, got))} != {dict(zip(rg.NAMES, ref))}'
    assert want[:, 1:3].sum() > 0 and want[-1, 0] == 2 * chunk + 5 and (want[:per16] == 0).all()
    assert np.array_equal(probed, table)                                   # og_range_probe == the table form
    tiny_bits = [_bits(source, 1 + i % 13, 1000 + i)[::-1] for i in range(300)]
    assert np.array_equal(many, np.stack([rg.stats_ref(b, source, target) for b in tiny_bits]))
    assert np.array_equal(shared, np.stack([rg.combine(want[-3:-1]), want[-1]]))     # two table rows, one stats row
    assert np.array_equal(twice[:, :7], 2 * want[:, :7]) and np.array_equal(twice[:, 7:], want[:, 7:])


def test_table_rows_without_workgroups_between_the_others(dev):
    """Empty rows in the middle and at the end of a table (the case above has them only at its front): the smallest table in which a
    wrong bisection hands a workgroup a neighbouring row."""
    chunk = _lib.load().og_range_chunk_elems()
    lengths = [9, 0, 0, chunk + 1, 0]
    data = [_bits('f32', n, 70 + i) for i, n in enumerate(lengths)]
    placed = [_place(b, 1 + i % 3, 'f32', dev) for i, b in enumerate(data)]
    with no_host_wait():
        got = range_report.range_stats([v for _, v in placed], torch.float16)
    got = got.cpu().numpy()
    want = np.stack([rg.stats_ref(b, 'f32', 'f16') for b in data])
    assert want[:, 0].tolist() == lengths and not want[[1, 2, 4]].any()
    for n, g, w in zip(lengths, got, want):
        assert np.array_equal(g, w), f'length {n}: {dict(zip(rg.NAMES, g))} != {dict(zip(rg.NAMES, w))}'


def test_refused_types(dev):
    lib = _lib.load()
    x = torch.zeros(64, dtype=torch.float16, device=dev)
    row = torch.zeros(9, dtype=torch.int64, device=dev)
    rc_ = lib.og_range_probe(_lib.ptr(x), 64, 1, 2, _lib.ptr(row), _lib.stream_ptr(dev))      # fp16 source, bf16 target
    assert rc_ == _lib.OG_EINVAL and b'source type' in lib.og_last_error()
    assert lib.og_range_probe(_lib.ptr(x), 64, 1, 0, _lib.ptr(row), _lib.stream_ptr(dev)) == _lib.OG_EINVAL   # fp32 is no target
    assert lib.og_range_stats(None, None, 1, 1, 1, _lib.ptr(row), None) == _lib.OG_EINVAL
    for call in (lambda: range_report.probe(x, torch.bfloat16, row.view(1, 9), 0), lambda: range_report.range_stats([x], torch.bfloat16)):
        assert pytest.raises(_lib.OgError, call).value.code == _lib.OG_EINVAL
    torch.cuda.synchronize(dev)
    assert not row.any()


# ---- the engine ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model():
    eng_mod.invalidate_engine_cache()
    return rc.perturb(rc.make_model(), 1).eval()


@pytest.fixture(scope='module')
def probing(dev, model):
    """dtype -> the probing graph engine of the module (batch 1, 128 x 128), built once"""
    made = {}

    def get(dtype):
        if dtype not in made:
            made[dtype] = models.InferenceEngine(model, 1, 128, 128, dtype=dtype, device=dev, probe=True)
        return made[dtype]
    return get


def _inputs(shape, dev, n=3):
    return [torch.randn(shape, generator=torch.Generator().manual_seed(40 + i)).to(dev) for i in range(n)]


def _run(engine, x):
    out = [o.clone() for o in engine.forward_raw(x)]
    torch.cuda.synchronize()
    return out


def _tensor_words(t, target):
    source = {torch.float32: 'f32', torch.float16: 'f16', torch.bfloat16: 'bf16'}[t.dtype]
    host = t.cpu().contiguous()
    bits = host.view(torch.int32).numpy().view(np.uint32) if source == 'f32' else host.view(torch.int16).numpy().view(np.uint16)
    return rg.stats_ref(bits, source, target)


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16], ids=['f16', 'bf16'])
def test_probing_engine(dev, model, probing, dtype):
    target = 'f16' if dtype == torch.float16 else 'bf16'
    engine = probing(dtype)
    plain = models.InferenceEngine(model, 1, 128, 128, dtype=dtype, device=dev, like=engine)
    eager = models.InferenceEngine(model, 1, 128, 128, dtype=dtype, device=dev, like=engine, use_graph=False, probe=True)
    assert plain._layers is engine._layers and eager._layers is engine._layers       # the weight bundle is shared as before
    assert plain.probe_stats is None and engine.probe_stats is not None and engine._graph is not None
    with pytest.raises(_lib.OgError):
        plain.activation_report()
    engine.reset_probes()
    eager.reset_probes()
    taps = []
    eager.probe_tap = lambda name, t: taps.append((name, t.detach().clone()))
    xs = _inputs(engine.shape, dev)
    for x in xs:
        got, want, serial = _run(engine, x), _run(plain, x), _run(eager, x)
        assert all(torch.equal(a, b) for a, b in zip(got, want)) and all(torch.equal(a, b) for a, b in zip(got, serial))
    report = engine.activation_report()
    points = len(report)
    assert len(taps) == 3 * points and points == engine.probe_stats.shape[0] > 100
    rows = engine.probe_stats.cpu().numpy()
    for i, entry in enumerate(report):
        mine = taps[i::points]
        assert [name for name, _ in mine] == [entry['name']] * 3 and list(mine[0][1].shape) == entry['shape']
        assert entry['n'] == 3 * int(np.prod(entry['shape']))
        ref = rg.combine([_tensor_words(t, target) for _, t in mine])
        assert np.array_equal(rows[i], ref), f"probe {i} {entry['name']} ({entry['route']}): {rows[i]} != {ref}"
        assert (entry['n'], entry['nan'], entry['inf'], entry['zero'], entry['sub']) == tuple(int(ref[j]) for j in (0, 1, 2, 4, 6))
    assert np.array_equal(eager.probe_stats.cpu().numpy(), rows)
    seen = {e['name'] for e in report} | {w for e in report for w in e['with']}
    assert {c.name for c, _ in engine._layers._convs()} <= seen
    assert {e['route'] for e in report} >= {'stem', 'heads', 'pointwise'} and any(e['with'] for e in report)
    engine.reset_probes()
    torch.cuda.synchronize(dev)
    assert not engine.probe_stats.any()
    with pytest.raises(_lib.OgError, match='16-bit'):
        models.InferenceEngine(model, 1, 128, 128, dtype=torch.float32, device=dev, use_graph=False, probe=True)


def test_planted_activation_overflow(dev, model, probing):
    """One mid-network BatchNorm's gamma times the power of two that lifts the fp32 output of its layer past 65504 (computed from
    the fp32 forward of the module: the largest output of the layer on this input): fp16's first probe with inf is that layer, bf16
    has none."""
    f16, bf16 = probing(torch.float16), probing(torch.bfloat16)
    layer = f16._layers.kps[0].low1[0].c1
    mods = dict(model.named_modules())
    bn = mods[layer.bn_name]
    x = _inputs(f16.shape, dev, 1)[0]
    peak = []
    hook = bn.register_forward_hook(lambda m, i, o: peak.append(float(torch.relu(o).max())))
    keep = bn.weight.detach().clone()
    try:
        with torch.no_grad():
            model(x.cpu())
            assert 0 < peak[0] < 65504
            power = int(np.ceil(np.log2(65504 / peak[0]))) + 1
            bn.weight.mul_(2.0 ** power)
            model(x.cpu())
        assert 65504 < peak[1] < 2.0 ** 20
        reports = []
        for engine in (f16, bf16):
            engine.refresh()
            engine.reset_probes()
            engine.forward_raw(x)
            reports.append(engine.activation_report())
    finally:
        hook.remove()
        with torch.no_grad():
            bn.weight.copy_(keep)
        for engine in (f16, bf16):
            engine.refresh()
            engine.reset_probes()
    first = next(e for e in reports[0] if e['inf'] > 0)
    assert first['name'] == layer.name and first['nan'] == 0
    assert not any(e['inf'] or e['nan'] for e in reports[1])
    assert max(e['max'] for e in reports[1]) > 65504


def _folded_words(conv, bn, dtype):
    stats = (bn.weight, bn.bias, bn.running_mean, bn.running_var)
    _, scale = rc.folded_bias(conv.weight.shape[0], None, tuple(s.detach().numpy() for s in stats) + (bn.eps,))
    with np.errstate(over='ignore', under='ignore'):
        w = conv.weight.detach().numpy() * scale[:, None, None, None]
    return dict(zip(rg.NAMES, rg.stats_ref(w.view(np.uint32), 'f32', 'f16' if dtype == torch.float16 else 'bf16')))


def test_planted_weight_overflow_and_flush(dev, model, probing):
    """One layer's running variance 0 (eps is then all that is left under the root) and its gamma the power of two that takes the
    median folded weight to 65520; another layer's gamma the power of two that takes its median folded weight to 2^-25.  The report's
    folded.over / folded.flush equal the restated fold's, stored.inf = folded.over, and every layer obeys stored = cast(folded)."""
    engine = probing(torch.float16)
    big, small = engine._layers.kps[0].low1[1].c1, engine._layers.kps[0].low1[1].c2
    mods = dict(model.named_modules())
    keep = {}

    def plant(layer, aim):
        conv, bn = mods[layer.name], mods[layer.bn_name]
        keep[layer.name] = (bn, bn.weight.detach().clone(), bn.running_var.detach().clone())
        with torch.no_grad():
            if aim > 1:
                bn.running_var.zero_()
            bn.weight.fill_(1.0)
            _, scale = rc.folded_bias(conv.weight.shape[0], None, (bn.weight.numpy(), bn.bias.numpy(), bn.running_mean.numpy(),
                                                                   bn.running_var.numpy(), bn.eps))
            median = float(np.median(np.abs(conv.weight.numpy() * scale[:, None, None, None])))
            bn.weight.fill_(2.0 ** round(np.log2(aim / median)))
        return conv, bn
    try:
        pairs = {big.name: plant(big, 65520.0), small.name: plant(small, 2.0 ** -25)}
        engine.refresh()
        report = {e['name']: e for e in engine.weight_report()}
        want = {name: _folded_words(conv, bn, torch.float16) for name, (conv, bn) in pairs.items()}
    finally:
        with torch.no_grad():
            for bn, gamma, var in keep.values():
                bn.weight.copy_(gamma)
                bn.running_var.copy_(var)
        engine.refresh()
    assert len(report) == len(list(engine._layers._convs()))
    for name, ref in want.items():
        assert {k: report[name]['folded'][k] for k in rg.NAMES[:7]} == {k: int(ref[k]) for k in rg.NAMES[:7]}, name
    n_big = want[big.name]['n']
    assert 0 < want[big.name]['over'] < n_big and 0 < want[small.name]['flush'] < want[small.name]['n']
    for name, e in report.items():
        s, f = e['stored'], e['folded']
        assert s['n'] == f['n'] == int(np.prod(e['shape'])) and s['over'] == s['flush'] == 0
        assert s['inf'] == f['over'] + f['inf'] and s['zero'] == f['zero'] + f['flush'] and s['sub'] == f['sub'] and s['nan'] == f['nan']
        assert (f['over'] > 0) == (name == big.name) and f['inf'] == 0
    clean = {e['name']: e for e in engine.weight_report()}
    assert all(e['folded']['over'] == 0 and e['stored']['inf'] == 0 for e in clean.values())
    for name, (conv, bn) in pairs.items():
        assert clean[name]['folded']['flush'] == _folded_words(conv, bn, torch.float16)['flush'] < 0.01 * n_big
    with pytest.raises(_lib.OgError, match='16-bit'):
        models.InferenceEngine(model, 1, 128, 128, dtype=torch.float32, device='cpu', use_graph=False).weight_report()


ARGV = ['--no-pretrain', '--initialize-whole', 'False', '--topk', '32', '--thre-hmp', '0.04', '--person-thre', '0.04', '--dist-max', '40',
        '--long-edge', '128', '--batch-size', '2', '--print-freq', '1000000', '--dump-name', 'run']


def test_run_images_range_report(dev, tmp_path, monkeypatch):
    """Four synthetic bs2 batches at long edge 128 on two lanes: the file is written, every probe's n is images x its elements per
    image, and the results are those of a run without the flag."""
    monkeypatch.setattr(evaluate, 'IN_FLIGHT', 2)
    torch.manual_seed(0)
    net, _ = models.model_factory(evaluate.evaluate_cli(ARGV))
    plain_stats = {}
    plain = evaluate.run_images(evaluate.evaluate_cli(ARGV), model=net, n_synthetic_batches=4, stats=plain_stats)
    assert 'range' not in plain_stats
    path = tmp_path / 'range.json'
    stats = {}
    probed = evaluate.run_images(evaluate.evaluate_cli(ARGV + ['--range-report', str(path)]), model=net, n_synthetic_batches=4, stats=stats)
    assert probed == plain and stats['engines_built'] == plain_stats['engines_built'] == 2
    report = json.loads(path.read_text())
    assert report == json.loads(json.dumps(stats['range'])) and report['dtype'] == 'float16' and report['images'] == 8
    assert len(report['activations']) > 100 and len(report['weights']) > 100
    for a in report['activations']:
        assert len(a['shapes']) == 1 and a['n'] == 8 * int(np.prod(a['shapes'][0][1:])), a['name']
    summary = report['summary']
    assert summary['first_nonfinite_activation'] is None and summary['weights_over'] == [] and 'no non-finite' in summary['verdict']
    assert summary['max_activation']['value'] == max(a['max'] for a in report['activations']) > 0
