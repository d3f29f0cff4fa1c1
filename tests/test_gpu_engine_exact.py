"""models/engine.py's layer glue on the GPU, bit for bit: real ConvBlock / Residual / HourglassLevel / head modules with exactly
representable parameters (tests/engine_exact.py) turned into the engine's own _Conv / _Residual / _Level objects (or run inside a
real InferenceEngine), fused=True, bf16 and fp16, against the staged fp64 reference.  Every comparison is torch.equal; every case
records its conv launches (conv_exact.record_launches) and asserts which entry point served it, so a route cannot go untested
silently after a threshold moves.

Routes and why the shapes are what they are (N <= 2, the smallest plane that selects the route):
  * og_conv3x3s2_tiled only serves layers with more than CONV_S2_MAX_PIXELS = 8192 output pixels (below, the split-K kernel comes
    first), so the stride-2 case runs 256 -> 256 from 224 x 160 (112 x 80 = 8960 outputs, a plane
    the stride-1 tiled kernel serves for conv2) and not 256 -> 384 from 80 x 80;
  * _Conv._hip launches og_conv2d (ksize 3) for the split-K route: the engine never calls og_conv3x3_*, which cannot be reached
    from it at any shape and is left to tests/test_gpu_conv_exact.py;
  * og_conv3x3_tiled_up2 with a projection block needs more than 8192 pixels (w_cat comes first): the merge cases use the identity
    block the network has there (low3[-1] of the 256-channel levels)."""
from collections import Counter

import pytest
import torch

import conv_exact as cx
import engine_exact as ex
from offsetguided_amd import models
from offsetguided_amd.models import engine as E
from offsetguided_amd.models.hourglass_104 import BLOCKS, DIMS, ConvBlock, HourglassLevel

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
RELU, SKIP_RELU, SKIP = (False, 1), (True, 1), (True, 0)          # (residual operand, ReLU) of a 3x3 launch

# case -> the launches it must make, in order: (family, shape as in test_gpu_conv_exact.CASES, epilogue)
ROUTES = {
    'cnvs-tiled': [('conv3x3_tiled', (1, 80, 48, 256, 256), RELU)],
    'cnvs-splitk': [('conv2d', (1, 40, 40, 256, 256, 3, 1), RELU)],
    'res384-band': [('conv_band', (2, 10, 10, 384, 384, 1, None), RELU), ('conv_band', (2, 10, 10, 384, 384, 1, None), SKIP_RELU)],
    'res512-band': [('conv_band', (2, 5, 5, 512, 512, 1, None), RELU), ('conv_band', (2, 5, 5, 512, 512, 1, None), SKIP_RELU)],
    'res384-512-s2-band': [('conv_band', (2, 10, 10, 384, 512, 2, None), RELU),
                           ('conv_band', (2, 5, 5, 512, 512, 1, (10, 10, 384, 2)), RELU)],
    'res384-256-wcat': [('conv2d', (1, 40, 40, 384, 256, 3, 1), RELU), ('conv2d_proj', (1, 40, 40, 256, 256, 40, 40, 384, 1), RELU)],
    'res256-tiled': [('conv3x3_tiled', (1, 80, 48, 256, 256), RELU), ('conv3x3_tiled', (1, 80, 48, 256, 256), SKIP_RELU)],
    'res256-s2-tiled': [('conv3x3s2_tiled', (1, 224, 160, 256, 256), RELU),
                        ('conv1x1_tiled', (1, 224, 160, 256, 256, 2, False), (False, False, 0)),
                        ('conv3x3_tiled', (1, 112, 80, 256, 256), SKIP_RELU)],
    'res256-up2': [('conv3x3_tiled', (1, 80, 48, 256, 256), RELU), ('conv3x3_tiled_up2', (1, 80, 48, 256, 256), SKIP_RELU)],
}
assert set(ROUTES) == set(ex.DENSE_CASES)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    return torch.device("cuda:0")


def _cl(t, dev, dtype):
    assert torch.equal(t.to(dtype).float(), t.float())                 # the operand is exact in the 16-bit type
    return t.to(dev).to(dtype).contiguous(memory_format=torch.channels_last)


def _assert_equal(got, exp64, dtype, what):
    exp = exp64.float() if dtype == torch.float32 else exp64.float().to(dtype)
    assert torch.equal(exp.double(), exp64) and got.dtype == dtype
    got = got.cpu()
    assert torch.equal(got, exp), f'{what}: {cx.describe_mismatch(got, exp)}'


def _recorder(monkeypatch, extra=()):
    records = []
    cx.record_launches(monkeypatch, records.append, extra)
    return records


def _block(m, dtype, relu=True):
    if isinstance(m, ConvBlock):
        return E._Conv(m.conv, m.bn, relu, dtype, True)
    return (E._Level if isinstance(m, HourglassLevel) else E._Residual)(m, dtype, True)


@pytest.mark.parametrize("dtype", DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize("name", list(ROUTES))
def test_dense_block(dev, name, dtype, monkeypatch):
    """One ConvBlock or Residual with dense exact parameters (negative gammas, a dead channel per layer) through the route its shape
    selects."""
    m, x, opts = ex.dense_case(name)
    exp = ex.case_reference(m, x, opts, dtype)
    records = _recorder(monkeypatch)
    with ex.issuing(dev), torch.no_grad():
        blk = _block(m, dtype)
        xd = _cl(x, dev, dtype)
        if 'merge_up' in opts:
            up = _cl(opts['merge_up'], dev, dtype)
            assert blk(xd, merge_up=up) is None                       # the output only ever exists inside the merge
            got = up
        else:
            got = blk(xd)
        torch.cuda.synchronize(dev)
        assert records == ROUTES[name], records
        _assert_equal(got, exp, dtype, name)
        if isinstance(m, ConvBlock):          # the same layer as the engine builds cnvs_ / a projection: ReLU off, residual operand
            skip = ex.grid8(ex.case_seed(name) + 3, tuple(exp.shape), cx.RES_MAX)
            del records[:]
            got = _block(m, dtype, relu=False)(xd, skip=_cl(skip, dev, dtype))
            assert records == [ROUTES[name][0][:2] + (SKIP,)], records
            mm = ex.as_double(m)
            _assert_equal(got, ex.ref_conv(mm.conv, mm.bn, x.double(), dtype, relu=False, skip=skip.double()), dtype, f'{name}, relu off')


# ----------------------------------------------------------------------------------------------------------------- the merge
def _small_level():
    torch.manual_seed(0)
    return ex.fill_exact(HourglassLevel(1, (256, 256), (1, 1)), 71, sparse=True), ex.ints(72, (2, 256, 64, 64))


_level_refs = {}


def _level_ref(key, make, dtype):
    if (key, dtype) not in _level_refs:
        m, x = make()
        _level_refs[key, dtype] = (m, x, ex.staged_reference(m, x, dtype=dtype))
    return _level_refs[key, dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize("conv_up2", [1, 0])
def test_level_merge_on_the_epilogue_and_as_a_pass(dev, conv_up2, dtype, monkeypatch):
    """The smallest level whose low3[-1] is large enough for og_conv3x3_tiled_up2 (2 x 32 x 32 = 2048 pixels), routing-mode
    weights: the merge on conv2's epilogue (CONV_UP2 = 1) and as og_upsample2_add after a plain tiled launch (0) give the same
    bits, those of the reference."""
    m, x, exp = _level_ref('small', _small_level, dtype)
    monkeypatch.setattr(E, 'CONV_UP2', conv_up2)
    records = _recorder(monkeypatch, extra=('og_upsample2_add',))
    with ex.issuing(dev), torch.no_grad():
        got = _block(m, dtype)(_cl(x, dev, dtype))
        torch.cuda.synchronize(dev)
    fam = Counter(r[0] for r in records)
    tiled = [r for r in records if r[0] == 'conv3x3_tiled']
    assert fam['conv2d'] == 1 and fam['conv2d_proj'] == 1 and {r[1] for r in tiled} == {(2, 64, 64, 256, 256), (2, 32, 32, 256, 256)}
    if conv_up2:
        assert fam['conv3x3_tiled_up2'] == 1 and fam['conv3x3_tiled'] == 5 and fam['og_upsample2_add'] == 0, fam
        assert ('conv3x3_tiled_up2', (2, 32, 32, 256, 256), SKIP_RELU) in records
    else:
        assert fam['conv3x3_tiled_up2'] == 0 and fam['conv3x3_tiled'] == 6 and fam['og_upsample2_add'] == 1, fam
    _assert_equal(got, exp, dtype, f'level merge, CONV_UP2={conv_up2}')


# ------------------------------------------------------------------------------------------------------------------ the level
def _level():
    torch.manual_seed(0)
    return ex.fill_exact(HourglassLevel(2, DIMS[2:], BLOCKS[2:]), 21, sparse=True), ex.ints(22, (1, DIMS[2], 40, 40))


# (BRANCHES, TRUNK_FIRST, DEEP_SHARED, CONV_BAND_MAX_PIXELS); an order-2 level has depths 0 and 1, so TRUNK_FIRST = 2 (the default)
# forks branch-first everywhere and 1 is the setting that queues the inner branch behind the trunk's first kernel
LEVEL_SETTINGS = [(1, 2, 3, 1024), (0, 2, 3, 1024), (1, 0, 3, 1024), (1, 1, 3, 1024), (1, 1, 1, 1024), (1, 2, 3, 0), (0, 0, 3, 0)]


@pytest.mark.parametrize("dtype", DTYPES, ids=['bf16', 'fp16'])
def test_level_every_setting_gives_the_same_bits(dev, dtype, monkeypatch):
    """HourglassLevel(2, DIMS[2:], BLOCKS[2:]) at 40 x 40, routing-mode weights (14 residuals in a chain: one product + bias + skip
    per stage).  The up1 forks and joins, the capture-order switch, the shared side stream and the band kernel on or off: every
    setting equals the reference, hence every other setting."""
    m, x, exp = _level_ref('order2', _level, dtype)
    assert exp.abs().max() > 4 and (exp != 0).double().mean() > 0.3
    records = _recorder(monkeypatch, extra=('og_upsample2_add',))
    xd = _cl(x, dev, dtype)
    for branches, trunk_first, deep_shared, band in LEVEL_SETTINGS:
        for k, v in (('BRANCHES', branches), ('TRUNK_FIRST', trunk_first), ('DEEP_SHARED', deep_shared), ('CONV_BAND_MAX_PIXELS', band)):
            monkeypatch.setattr(E, k, v)
        del records[:]
        with ex.issuing(dev), torch.no_grad():
            got = _block(m, dtype)(xd)             # built afresh: a layer is packed for one route
            torch.cuda.synchronize(dev)
        fam = Counter(r[0] for r in records)
        # both branches of both levels launch: up1 of the outer level at 40 x 40, of the inner one at 20 x 20
        assert sum(1 for r in records if r[0] == 'conv2d' and r[1] == (1, 40, 40, 384, 384, 3, 1)) == 4, records
        if band:
            assert fam == {'conv2d': 5, 'conv_band': 23, 'og_upsample2_add': 2}, fam
            assert sum(1 for r in records if r[1] == (1, 20, 20, 384, 384, 1, None)) == 10, records
        else:
            assert fam == {'conv2d': 26, 'conv2d_proj': 2, 'og_upsample2_add': 2}, fam
        _assert_equal(got, exp, dtype, f'level, BRANCHES={branches} TRUNK_FIRST={trunk_first} DEEP_SHARED={deep_shared} band={band}')


# ---------------------------------------------------------------------------------------------- stem, pre, junction and heads
_models = {}


def _model(flags):
    if flags not in _models:
        _models[flags] = ex.exact_model(flags)
    return _models[flags]


@pytest.mark.parametrize("dtype", DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize("flags", [(), ('--include-scale', '--include-jitter-offset')], ids=['2heads', '4heads'])
def test_engine_stem_pre_junction_heads(dev, flags, dtype, monkeypatch):
    """A strict InferenceEngine on a model_factory model with exact parameters in pre, the junction and the heads; forward_raw with
    the hourglasses taken out (engine_exact.drive_engine).  The stem pack, pre[1], the junction's summed biases and concatenated
    weights, the heads' concatenation, padding, pack and output slices: every recorded stage against the fp64 modules."""
    model = _model(flags)
    net, heads = model.basenet, ex.head_convs(model)
    chans = tuple(h.out_channels for h in heads)
    assert chans == ((17, 38, 17, 2) if flags else (17, 38))
    image, feat0, feat1, inter = ex.engine_inputs()
    records = _recorder(monkeypatch, extra=('og_bias_act', 'og_nhwc_bf16_to_nchw_f32', 'og_nhwc_f16_to_nchw_f32'))
    eng = models.InferenceEngine(model, 1, 128, 128, device=dev, dtype=dtype, use_graph=False)
    assert eng.strict and eng.fused
    f0, f1, it = (_cl(t, dev, dtype) for t in (feat0, feat1, inter))
    stem, j1x1 = ('stem7x7', (1, 128, 128), (1,)), ('conv1x1_tiled', (1, 32, 32, 256, 256, 1, True), (True, False, 1))
    hd = ('conv1x1_heads', (1, 32, 32, 256, chans), ())
    # the real pre
    outs, seen = ex.drive_engine(eng, image.to(dev), f0, f1)
    torch.cuda.synchronize(dev)
    assert records == [stem, ('conv2d', (1, 64, 64, 128, 256, 3, 2), RELU), ('conv_band', (1, 32, 32, 256, 256, 1, (64, 64, 128, 2)), RELU),
                       j1x1, hd], records
    _assert_equal(seen['pre'], ex.staged_reference(net.pre, image, dtype=dtype), dtype, 'pre')
    exp_heads = ex.staged_reference(heads, feat1)
    assert len(outs) == len(heads)
    for i, (got, exp) in enumerate(zip(outs, exp_heads)):
        assert got.is_contiguous()
        _assert_equal(got, exp, torch.float32, f'head {i}')
    # the junction on exact inputs
    del records[:]
    outs, seen = ex.drive_engine(eng, image.to(dev), f0, f1, inter=it)
    torch.cuda.synchronize(dev)
    assert records == [stem, j1x1, hd], records
    _assert_equal(seen['junction'], ex.staged_reference((net.inters_[0], net.cnvs_[0]), inter, feat0, dtype=dtype), dtype, 'junction')
    assert eng.torch_conv_calls == []
    # the two-pass branches: pointwise kernels off, torch's convolution allowed
    monkeypatch.setattr(E, 'CONV_TILED', 3)
    loose = models.InferenceEngine(model, 1, 128, 128, device=dev, dtype=dtype, use_graph=False, like=eng, strict=False)
    assert loose._layers is eng._layers
    del records[:]
    outs, seen = ex.drive_engine(loose, image.to(dev), f0, f1, inter=it)
    torch.cuda.synchronize(dev)
    nhwc = 'og_nhwc_f16_to_nchw_f32' if dtype == torch.float16 else 'og_nhwc_bf16_to_nchw_f32'
    assert records == [stem, ('og_bias_act', (), ())] + [(nhwc, (), ())] * len(heads), records
    assert len(loose.torch_conv_calls) == 3, loose.torch_conv_calls
    _assert_equal(seen['junction'], ex.staged_reference((net.inters_[0], net.cnvs_[0]), inter, feat0, dtype=dtype, fallback=True), dtype,
                  'junction, two passes')
    for i, (got, exp) in enumerate(zip(outs, ex.staged_reference(heads, feat1, dtype=dtype, conv_rounded=True), strict=True)):
        _assert_equal(got, exp, torch.float32, f'head {i}, two passes')
