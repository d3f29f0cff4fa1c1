"""models/engine.py's layer glue -- the BatchNorm fold, _Conv / _Residual / _Level, the junction's summed biases, the heads -- on its
fp32 CPU checking path against the fp64 modules themselves, bit for bit, on exactly representable parameters (tests/engine_exact.py);
and that file held honest: the staged reference against the plain module, its precondition, what the comparison can see, and how
much of the expected output the 16-bit roundings really change."""
import pytest
import torch

import conv_exact as cx
import engine_exact as ex
from offsetguided_amd import models
from offsetguided_amd.models import engine as E
from offsetguided_amd.models.hourglass_104 import BLOCKS, DIMS, ConvBlock, HourglassLevel, Residual

DTYPES = [torch.bfloat16, torch.float16]
F32 = dict(dtype=torch.float32, fused=False)


def _equal(got, exp64, what):
    assert got.dtype == torch.float32
    assert torch.equal(got.double(), exp64), f'{what}: {cx.describe_mismatch(got.double(), exp64)}'


def _engine_block(m, relu=True):
    if isinstance(m, ConvBlock):
        return E._Conv(m.conv, m.bn, relu, **F32)
    return (E._Residual if isinstance(m, Residual) else E._Level)(m, **F32)


# ------------------------------------------------------------------------------------------------------------------ parameters
def test_var_plus_eps_is_a_power_of_four_in_fp32():
    for k in ex.VAR_EXPONENTS:
        v = ex.exact_var(k)
        assert v.dtype == torch.float32 and torch.equal(torch.sqrt(v + ex.EPS), torch.tensor(2.0 ** k))
        assert not torch.equal(torch.sqrt(v + 1e-5), torch.tensor(2.0 ** k))          # the eps matters at every k


@pytest.mark.parametrize("sparse", [False, True], ids=['dense', 'routing'])
def test_fill_exact_parameters_fold_exactly(sparse):
    m = ex.fill_exact(Residual(128, 256, stride=2), 5, sparse=sparse)
    for conv, bn in ((m.conv1, m.bn1), (m.conv2, m.bn2), (m.skip[0], m.skip[1])):
        assert bn.eps == ex.EPS
        gamma = bn.weight.detach()
        live = gamma != 0
        assert 1 <= int((~live).sum()) <= 32 and bool((gamma < 0).any()) and bool((gamma > 0).any())
        assert torch.equal(torch.log2(gamma[live].abs()), torch.log2(gamma[live].abs()).round())      # signed powers of two
        scale = ex.bn_scale(ex.as_double(bn), bn.num_features).flatten()
        s = -torch.log2(scale[live].abs())
        assert torch.equal(s, s.round()) and set(s.tolist()) <= (set((0.0,)) if sparse else set(map(float, ex.DENSE_S)))
        assert torch.equal(torch.sign(scale), torch.sign(gamma.double()))
        w, b = E._fold(conv, bn)                                                     # what the engine makes of them
        assert torch.equal(w.double(), conv.weight.detach().double() * scale.view(-1, 1, 1, 1))
        k = b * 64
        assert torch.equal(k, k.round()) and bool((k % 2 == 1).all()) and b.abs().max() <= 4
        assert bool((w[~live] == 0).all())
        for dtype in DTYPES:
            assert torch.equal(w.to(dtype).float(), w) and torch.equal(b.to(dtype).float(), b)
        wt = conv.weight.detach()
        if sparse:
            assert bool(((wt != 0).sum((1, 2, 3)) == 1).all()) and bool((wt.abs().sum((1, 2, 3)) == 1).all())
        else:
            assert wt.abs().max() == 2 and torch.equal(wt, wt.round())


# --------------------------------------------------------------------------------------- the engine's blocks on the CPU path
@pytest.mark.parametrize("name", list(ex.DENSE_CASES))
def test_dense_block_equals_the_fp64_module(name):
    """_Conv / _Residual built from the module, fp32 on the CPU, against the module in fp64 (no 16-bit rounding on this path), and
    the staged reference with rounding off against the same: all three bit for bit."""
    m, x, opts = ex.dense_case(name, small=True)
    up = opts.get('merge_up')
    plain = ex.plain_fp64(m, x)
    if up is not None:
        plain = up.double() + plain.repeat_interleave(2, 2).repeat_interleave(2, 3)
    assert torch.equal(ex.case_reference(m, x, opts, None), plain)
    with torch.no_grad():
        got = _engine_block(m)(x.clone())
        if up is not None:      # the CPU path has no fused merge: _Level's own line
            got = up + torch.nn.functional.interpolate(got, scale_factor=2, mode='nearest')
    _equal(got, plain, name)
    if isinstance(m, ConvBlock):                    # the same layer built with ReLU off, and with a residual operand
        skip = ex.grid8(3, tuple(plain.shape), cx.RES_MAX)
        mm = ex.as_double(m)
        with torch.no_grad():
            lin = mm.bn(mm.conv(x.double()))
            _equal(_engine_block(m, relu=False)(x.clone()), lin, f'{name}, relu off')
            _equal(_engine_block(m, relu=False)(x.clone(), skip=skip.clone()), lin + skip.double(), f'{name}, relu off, skip')
            _equal(_engine_block(m)(x.clone(), skip=skip.clone()), torch.relu(lin + skip.double()), f'{name}, skip')
        assert bool((lin < 0).any())


def _routing_level():
    torch.manual_seed(0)
    m = ex.fill_exact(HourglassLevel(2, DIMS[2:], BLOCKS[2:]), 21, sparse=True)
    return m, ex.ints(22, (1, DIMS[2], 20, 20))


def test_level_equals_the_fp64_module():
    m, x = _routing_level()
    plain = ex.plain_fp64(m, x)
    assert torch.equal(ex.staged_reference(m, x, dtype=None), plain) and plain.abs().max() > 4
    with torch.no_grad():
        _equal(_engine_block(m)(x.clone()), plain, 'level')


# ------------------------------------------------------------------------------------------------------- a whole engine, CPU
@pytest.mark.parametrize("flags", [(), ('--include-scale', '--include-jitter-offset')], ids=['2heads', '4heads'])
def test_whole_engine_stage_by_stage(flags):
    """InferenceEngine(dtype=float32, device='cpu') on a model_factory model whose pre, junction and head modules hold exact
    parameters: forward_raw with the hourglasses taken out (engine_exact.drive_engine), every recorded stage against the fp64
    modules."""
    model = ex.exact_model(flags)
    net = model.basenet
    eng = models.InferenceEngine(model, 1, 128, 128, dtype=torch.float32, device='cpu', use_graph=False)
    image, feat0, feat1, inter = ex.engine_inputs()
    heads = ex.head_convs(model)
    assert [h.out_channels for h in heads] == ([17, 38, 17, 2] if flags else [17, 38])
    outs, seen = ex.drive_engine(eng, image, feat0, feat1)
    _equal(seen['pre'], ex.plain_fp64(net.pre, image), 'pre')
    assert torch.equal(ex.staged_reference(net.pre, image, dtype=None), ex.plain_fp64(net.pre, image))
    exp_heads = [ex.plain_fp64(h, feat1) for h in heads]
    for got, exp, ref in zip(outs, exp_heads, ex.staged_reference(heads, feat1), strict=True):
        _equal(got, exp, 'head')
        assert torch.equal(ref, exp) and got.is_contiguous()
    outs, seen = ex.drive_engine(eng, image, feat0, feat1, inter=inter)
    with torch.no_grad():
        j = torch.relu(ex.as_double(net.inters_[0])(inter.double()) + ex.as_double(net.cnvs_[0])(feat0.double()))
    _equal(seen['junction'], j, 'junction')
    assert torch.equal(ex.staged_reference((net.inters_[0], net.cnvs_[0]), inter, feat0, dtype=None), j)
    assert torch.equal(ex.staged_reference((net.inters_[0], net.cnvs_[0]), inter, feat0, dtype=None, fallback=True), j)


# ------------------------------------------------------------------------------------------------------------- the precondition
def test_precondition_rejects_fold_scale_one_on_a_dense_block():
    """s = 0 on a dense two-stage block: conv1's outputs are integers up to thousands, conv2's sum of them next to a 2^-6 bias no
    longer fits fp32's 24 bits."""
    torch.manual_seed(0)
    m = ex.fill_exact(Residual(512, 512), 3, s_choices=(0,))
    x = ex.ints(4, (2, 512, 5, 5))
    with pytest.raises(ex.PreconditionError, match='2\\^24'):
        ex.staged_reference(m, x, dtype=torch.float16)
    with pytest.raises(ex.PreconditionError, match='2\\^24'):
        ex.staged_reference(m, x, dtype=None)
    ex.staged_reference(ex.fill_exact(m, 3), x, dtype=torch.float16)            # the same block with s in 3..6 passes
    assert issubclass(ex.PreconditionError, AssertionError)


def test_grid_exp():
    assert ex.grid_exp(torch.tensor([0.0, 3.0, -4096.0])) == 0 and ex.grid_exp(torch.tensor([0.5, 3.0])) == 1
    assert ex.grid_exp(torch.tensor([1.0 + 2.0 ** -20, -2.0 ** -7])) == 20 and ex.grid_exp(torch.zeros(3)) == 0


# ------------------------------------------------------------------------------------------------------------------ sensitivity
def _wrong(m, edit):
    mm = ex.as_double(m)
    with torch.no_grad():
        edit(mm)
    return mm


@pytest.mark.parametrize("dtype", [torch.float32] + DTYPES, ids=['fp32', 'bf16', 'fp16'])
def test_wrong_expectations_differ(dtype):
    """Each kind of glue mistake, written as a wrong expectation on the operands of the 'res384-256-wcat' case (and of the heads),
    differs from the right one in at least one element after the final rounding to `dtype`: the operands can see it."""
    m, x, _ = ex.dense_case('res384-256-wcat', small=True)
    x64 = x.double()
    fin = lambda v: v.float() if dtype == torch.float32 else v.float().to(dtype)          # noqa: E731
    right = ex.plain_fp64(m, x)

    def no_proj_bias(mm):
        mm.skip[1].bias.zero_()
        mm.skip[1].running_mean.zero_()

    def no_eps(mm):
        for bn in (mm.bn1, mm.bn2, mm.skip[1]):
            bn.eps = 1e-5

    def no_sign(mm):
        for bn in (mm.bn1, mm.bn2, mm.skip[1]):
            bn.weight.abs_()

    def twice_proj_bias(mm):
        c = mm.skip[1](torch.zeros(1, 256, 1, 1, dtype=torch.float64)).flatten()
        mm.bn2.bias.add_(c)
    wrong = {name: _wrong(m, edit)(x64) for name, edit in (('projection bias dropped', no_proj_bias), ('eps ignored', no_eps),
                                                            ('gamma sign ignored', no_sign),
                                                            ('projection bias counted twice', twice_proj_bias))}
    # w_cat with the projection first, read by a kernel that expects [conv2 | projection] along K
    mm = ex.as_double(m)
    with torch.no_grad():
        y = torch.relu(mm.bn1(mm.conv1(x64)))
        w2 = mm.conv2.weight * ex.bn_scale(mm.bn2, 256).view(-1, 1, 1, 1)
        wp = mm.skip[0].weight * ex.bn_scale(mm.skip[1], 256).view(-1, 1, 1, 1)
        bias = (mm.bn2(torch.zeros(1, 256, 1, 1, dtype=torch.float64)) + mm.skip[1](torch.zeros(1, 256, 1, 1, dtype=torch.float64))).flatten()
        cat = torch.cat([w2.permute(0, 2, 3, 1).reshape(256, -1), wp.reshape(256, -1)], 1)
        assert torch.equal(torch.relu(cx.exact_sum(y, cat[:, :2304].reshape(256, 3, 3, 256).permute(0, 3, 1, 2), bias, x2=x64,
                                                   w2=cat[:, 2304:])), right)
        swapped = torch.cat([wp.reshape(256, -1), w2.permute(0, 2, 3, 1).reshape(256, -1)], 1)
        wrong['w_cat with the projection first'] = torch.relu(cx.exact_sum(
            y, swapped[:, :2304].reshape(256, 3, 3, 256).permute(0, 3, 1, 2), bias, x2=x64, w2=swapped[:, 2304:]))
    for name, out in wrong.items():
        differ = int((fin(out) != fin(right)).sum())
        print(f'{name}, {dtype}: {differ} of {right.numel()} elements differ')
        assert differ >= 1, f'{name}: the operands cannot see it'
    # a head slice shifted by one channel of the concatenated output
    torch.manual_seed(2)
    heads = [ex.fill_exact(torch.nn.Conv2d(256, c, 1), 60 + c) for c in (17, 38, 17, 2)]
    feat = ex.ints(61, (1, 256, 6, 5))
    outs = ex.staged_reference(heads, feat)
    full = torch.cat(outs + [torch.zeros(1, 6, 6, 5, dtype=torch.float64)], 1)        # padded to a multiple of 8
    c0 = 0
    for o in outs:
        assert torch.equal(full[:, c0:c0 + o.shape[1]], o) and not torch.equal(full[:, c0 + 1:c0 + 1 + o.shape[1]], o)
        c0 += o.shape[1]


# ------------------------------------------------------------------------------------------------------------ rounding coverage
@pytest.mark.parametrize("name", list(ex.DENSE_CASES))
def test_rounding_is_exercised_in_every_dense_case(name):
    """From the reference alone, at the shapes the GPU file runs: per (case, 16-bit type) at least 5 % of the nonzero expected
    outputs differ from their unrounded value, so a rounding in the wrong place or of the wrong kind moves the expectation.

    Measured shares (bf16 / fp16) are listed in EXPERIMENTS.md."""
    m, x, opts = ex.dense_case(name)
    for dtype in DTYPES:
        trace = []
        exp = ex.case_reference(m, x, opts, dtype, trace)
        assert torch.equal(exp.float().to(dtype).double(), exp)                      # 16-bit numbers
        share = ex.changed_share(trace)
        print(f'{name} {dtype}: {share:.1%} of the nonzero expected outputs rounded; stages {[t[0] for t in trace]}')
        assert share >= 0.05, (name, dtype, share)
