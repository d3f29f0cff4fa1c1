"""Exactly representable PARAMETERS for the modules of models/hourglass_104.py and the staged fp64 reference of what the engine
(models/engine.py) must compute from them (tests/test_engine_exact_cpu.py, tests/test_gpu_engine_exact.py).

tests/conv_exact.py pins each conv entry point on operands the test packs itself.  This file is one level up: the weights sit in a
real ConvBlock / Residual / HourglassLevel / head Conv2d, the engine folds, casts, sums, concatenates, packs and routes them, and the
expectation is the module's own forward in fp64 with one round_once wherever the engine stores a 16-bit activation.

fill_exact: integer conv weights; BatchNorm with eps = 2^-10 and running_var = 4^k - 2^-10 (var + eps is 4^k exactly, in fp32 and
fp64), gamma a signed power of two, so the fold scale is +-2^-s; about one channel in 32 dead (gamma = 0); the folded bias
-mean * scale + beta an odd multiple of 2^-6.  Every folded weight and bias is then exact in fp32, bf16 and fp16.

The reference never calls the engine, its fold or a packer.  Every stage asserts (sum |x w| + |bias| + |skip|) 2^g < 2^24 per output
element, g the finest grid exponent among the stage's terms: the fp32 result is then the same in every summation order and the
expected tensor is unique.  A breach raises PreconditionError: an error in the test's operands, never a skip."""
import contextlib
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_exact as cx
from offsetguided_amd.models.hourglass_104 import ConvBlock, HourglassLevel, Residual

EPS = 2.0 ** -10
DENSE_S = (3, 4, 5, 6)                  # fold scale 2^-s per channel, dense mode
GAMMA_EXP = (-1, 0, 1)                  # |gamma| = 2^j
VAR_EXPONENTS = range(min(GAMMA_EXP), max(DENSE_S) + max(GAMMA_EXP) + 1)      # every k = s + j that fill_exact can draw
DEAD_SHARE = 1.0 / 32


class PreconditionError(AssertionError):
    pass


# ------------------------------------------------------------------------------------------------------------------ parameters
def exact_var(k):
    """fp32 running_var = 4^k - 2^-10 with var + eps == 4^k exactly (asserted here, for every k used)."""
    v = torch.tensor(4.0 ** k - EPS, dtype=torch.float32)
    assert v.double().item() == 4.0 ** k - EPS, f'k = {k}: 4^k - 2^-10 is not an fp32 number'
    assert (v + EPS).item() == 4.0 ** k and (v.double() + EPS).item() == 4.0 ** k, f'k = {k}: var + eps != 4^k'
    return v


def _fill_conv(m, g, sparse):
    cout, cin, kh, kw = m.weight.shape
    if sparse:      # routing mode: one tap (ci, ky, kx) per output channel, weight +-1
        w = torch.zeros(cout, cin, kh, kw)
        sign = torch.randint(0, 2, (cout,), generator=g).float() * 2 - 1
        w[torch.arange(cout), torch.randint(0, cin, (cout,), generator=g), torch.randint(0, kh, (cout,), generator=g),
          torch.randint(0, kw, (cout,), generator=g)] = sign
    else:
        w = cx._ints(g, (cout, cin, kh, kw), cx.W_MAX)
    m.weight.copy_(w)
    if m.bias is not None:
        m.bias.copy_(cx._odd_grid(g, (cout,), cx.BIAS_GRID, cx.BIAS_MAX))


def _fill_bn(bn, g, s_choices):
    c = bn.num_features
    s = torch.tensor(s_choices)[torch.randint(0, len(s_choices), (c,), generator=g)]
    j = torch.tensor(GAMMA_EXP)[torch.randint(0, len(GAMMA_EXP), (c,), generator=g)]
    sign = torch.randint(0, 2, (c,), generator=g).float() * 2 - 1
    dead = torch.rand(c, generator=g) < DEAD_SHARE
    a, b = (int(i) for i in torch.randperm(c, generator=g)[:2])
    dead[a], dead[b], sign[b] = True, False, -1.0          # every layer has a dead channel and a negative gamma
    bn.eps = EPS
    bn.running_var.copy_(torch.stack([exact_var(int(k)) for k in s + j]))
    bn.weight.copy_(torch.where(dead, torch.zeros(c), sign * 2.0 ** j))
    target = cx._odd_grid(g, (c,), cx.BIAS_GRID, cx.BIAS_MAX)          # -mean * scale + beta
    q = cx._grid(g, (c,), cx.RES_GRID, 2)                               # mean * scale
    bn.running_mean.copy_(q * sign * 2.0 ** s)
    bn.bias.copy_(target + torch.where(dead, torch.zeros(c), q))


def fill_exact(module, seed, sparse=False, s_choices=None):
    """Exactly representable parameters for every Conv2d and BatchNorm2d under `module` (in place, fp32).  sparse = routing mode:
    one +-1 tap per output channel and fold scale +-1 (s = 0).  s_choices overrides the set the per-channel s is drawn from."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    s_choices = tuple(s_choices) if s_choices is not None else ((0,) if sparse else DENSE_S)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.Conv2d):
                _fill_conv(m, g, sparse)
            elif isinstance(m, nn.BatchNorm2d):
                _fill_bn(m, g, s_choices)
    return module


def as_double(module):
    """An fp64 eval-mode CPU copy: what the reference runs; the caller's module stays as it is."""
    return copy.deepcopy(module).double().eval()


# ------------------------------------------------------------------------------------------------------------- staged reference
def _low_bit(t):
    """Per element: the exponent of the lowest set bit of its fp64 value (zeros: a large number)."""
    t = t.detach().double()
    m, e = torch.frexp(t)
    mi = (m.abs() * 2.0 ** 53).to(torch.int64)
    low = torch.log2((mi & -mi).clamp(min=1).double()).to(torch.int64)
    return torch.where(t == 0, torch.full_like(low, 1 << 20), e.to(torch.int64) - 53 + low)


def grid_exp(t):
    """Smallest e >= 0 with t * 2^e integer in every element."""
    return max(0, -int(_low_bit(t).min())) if t.numel() else 0


def grid_exp_channels(t):
    """grid_exp per leading index (output channel) -> (1, C, 1, 1): an output element only ever sums its own channel's weights."""
    return (-_low_bit(t).reshape(t.shape[0], -1).min(1).values).clamp(min=0).view(1, -1, 1, 1)


def _bn(bn, z):
    return bn(z) if bn is not None else z


def bn_scale(bn, c):
    """The per-channel multiplier of a BatchNorm, read off its own forward: bn(1) - bn(0)."""
    z = torch.zeros((1, c, 1, 1), dtype=torch.float64)
    return _bn(bn, z + 1) - _bn(bn, z)


def _term(conv, bn, x):
    """One conv (+ BN) of a stage, from the module's own forward: (linear part, constant (1,C,1,1), sum |x w| per output, grid)."""
    const = _bn(bn, conv(torch.zeros((1, conv.in_channels, 1, 1), dtype=torch.float64)))
    assert tuple(const.shape[2:]) == (1, 1)
    lin = _bn(bn, conv(x)) - const
    alpha = bn_scale(bn, conv.out_channels)
    mass = F.conv2d(x.abs(), conv.weight.abs(), None, conv.stride, conv.padding) * alpha.abs()
    return lin, const, mass, grid_exp(x) + grid_exp_channels(conv.weight * alpha.view(-1, 1, 1, 1))


def _finish(v, bound, g, dtype, what, trace):
    """g: the grid exponent, a number or per output channel (1, C, 1, 1)."""
    worst = float((bound * 2.0 ** torch.as_tensor(g, dtype=torch.float64)).max())
    if not worst < 2.0 ** 24:
        raise PreconditionError(f'{what}: (sum|x w| + |bias| + |skip|) * 2^g = {worst:.4g} >= 2^24: the fp32 sum depends on its order')
    out = v if dtype is None else cx.round_once(v, dtype).double()
    if trace is not None:
        trace.append((what, v, out))
    return out


def _stage(terms, skip, relu, dtype, what, trace, with_const=True):
    lin = sum(t[0] for t in terms)
    bound = sum(t[2] for t in terms)
    grids = [t[3] for t in terms]
    if with_const:
        lin = lin + sum(t[1] for t in terms)
        bound = bound + sum(t[1].abs() for t in terms)
        grids += [grid_exp_channels(t[1].flatten()) for t in terms]
    if skip is not None:
        lin, bound = lin + skip, bound + skip.abs()
        grids.append(grid_exp(skip))
    g = torch.stack([torch.as_tensor(g).expand(1, lin.shape[1], 1, 1) for g in grids]).max(0).values
    return _finish(torch.relu(lin) if relu else lin, bound, g, dtype, what, trace)


def _merge(up, low, dtype, trace):
    """round(up + nearest2x(low)), low already stored in 16 bits: the up2 contract of conv_exact.exact_reference."""
    low2 = low.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    return _finish(up + low2, up.abs() + low2.abs(), max(grid_exp(up), grid_exp(low)), dtype, 'merge', trace)


def ref_conv(conv, bn, x, dtype, relu=True, skip=None, trace=None):
    """act(bn(conv(x)) (+ skip)), stored once: a ConvBlock (relu) or a bare conv + BN (_Conv built with relu off)."""
    return _stage([_term(conv, bn, x)], skip, relu, dtype, 'conv', trace)


def ref_residual(m, x, dtype, proj_rounded=False, merge_up=None, trace=None):
    """Residual.forward with the engine's stores: after conv1 + bn1 + relu, after the sum + relu; proj_rounded: the pointwise route
    writes the projection (without its bias, which rides on conv2's) out in 16 bits first; merge_up: then the level merge."""
    y = _stage([_term(m.conv1, m.bn1, x)], None, True, dtype, 'conv1', trace)
    terms, skip = [_term(m.conv2, m.bn2, y)], x
    if len(m.skip):
        p = _term(m.skip[0], m.skip[1], x)
        if proj_rounded:
            skip = _stage([p], None, False, dtype, 'projection', trace, with_const=False)
            terms.append((torch.zeros_like(p[1]), p[1], torch.zeros_like(p[1]), torch.zeros_like(p[1], dtype=torch.int64)))
        else:
            terms.append(p)
            skip = None
    out = _stage(terms, skip, True, dtype, 'conv2', trace)
    return out if merge_up is None else _merge(merge_up, out, dtype, trace)


def ref_level(m, x, dtype, trace=None):
    """HourglassLevel.forward: up1(x) + nearest2x(low3(low2(low1(x)))), every residual staged, the merge stored once."""
    up, low = x, x
    for r in m.up1:
        up = ref_residual(r, up, dtype, trace=trace)
    for r in m.low1:
        low = ref_residual(r, low, dtype, trace=trace)
    if isinstance(m.low2, HourglassLevel):
        low = ref_level(m.low2, low, dtype, trace)
    else:
        for r in m.low2:
            low = ref_residual(r, low, dtype, trace=trace)
    for r in m.low3:
        low = ref_residual(r, low, dtype, trace=trace)
    return _merge(up, low, dtype, trace)


def ref_junction(inters_, cnvs_, inter, feat, dtype, fallback=False, trace=None):
    """relu(inters_(inter) + cnvs_(feat)): one stage over both inputs.  fallback: the engine's two-pass branch writes each raw
    convolution out in 16 bits, then adds the summed biases and the second one as the residual operand."""
    a, b = _term(inters_[0], inters_[1], inter), _term(cnvs_[0], cnvs_[1], feat)
    if not fallback:
        return _stage([a, b], None, True, dtype, 'junction', trace)
    ra = _stage([a], None, False, dtype, 'inters_ raw', trace, with_const=False)
    rb = _stage([b], None, False, dtype, 'cnvs_ raw', trace, with_const=False)
    const = a[1] + b[1]
    v = ra + const + rb
    return _finish(torch.relu(v), ra.abs() + a[1].abs() + b[1].abs() + rb.abs(), max(grid_exp(ra), grid_exp(rb), grid_exp(const)), dtype,
                   'junction, two passes', trace)


def ref_pre(pre, image, dtype, trace=None):
    """Hourglass104.pre: the stem ConvBlock, then its stride-2 residual."""
    return ref_residual(pre[1], ref_conv(pre[0].conv, pre[0].bn, image, dtype, trace=trace), dtype, trace=trace)


def ref_heads(convs, feat, dtype=None, conv_rounded=False, trace=None):
    """One fp64 tensor per head Conv2d (bias, no BN).  The heads kernel writes fp32 from its accumulators: the exact value.
    conv_rounded: the two-pass branch stores the raw convolution in 16 bits and adds the bias in fp32 afterwards."""
    outs = []
    for conv in convs:
        t = _term(conv, None, feat)
        if conv_rounded:
            raw = _stage([t], None, False, dtype, 'head raw', trace, with_const=False)
            outs.append(_finish(raw + t[1], raw.abs() + t[1].abs(), max(grid_exp(raw), grid_exp(t[1])), torch.float32, 'head', trace))
        else:
            outs.append(_stage([t], None, False, torch.float32, 'head', trace))
    return outs


def staged_reference(module, *inputs, dtype=None, **kw):
    """The expected output (fp64 values of the 16-bit numbers) of the engine object built from `module` for fp32 CPU inputs.
    module: ConvBlock | Residual | HourglassLevel | Sequential(ConvBlock, Residual) (pre) | (inters_, cnvs_) | [head Conv2d, ...].
    dtype None: no rounding anywhere, i.e. the plain fp64 module."""
    m = [as_double(p) for p in module] if isinstance(module, (tuple, list)) else as_double(module)
    xs = [None if x is None else x.detach().double().cpu() for x in inputs]
    with torch.no_grad():
        if isinstance(m, ConvBlock):
            return ref_conv(m.conv, m.bn, xs[0], dtype, skip=xs[1] if len(xs) > 1 else None, **kw)
        if isinstance(m, Residual):
            return ref_residual(m, xs[0], dtype, **kw)
        if isinstance(m, HourglassLevel):
            return ref_level(m, xs[0], dtype, **kw)
        if isinstance(m, nn.Sequential):
            return ref_pre(m, xs[0], dtype, **kw)
        if isinstance(module, tuple):
            return ref_junction(m[0], m[1], xs[0], xs[1], dtype, **kw)
        return ref_heads(m, xs[0], dtype, **kw)


def plain_fp64(module, *inputs):
    """The module's forward in fp64, untouched: what staged_reference(dtype=None) must equal bit for bit."""
    with torch.no_grad():
        return as_double(module)(*[x.detach().double().cpu() for x in inputs])


def changed_share(trace):
    """Share of the nonzero expected outputs of the LAST stage that differ from their unrounded value; for a merge the unrounded
    value is up + nearest2x(the never-rounded sum of the convolution below): either rounding point may have moved it."""
    what, v, out = trace[-1]
    if what == 'merge':
        _, pv, pout = trace[-2]
        v = v + (pv - pout).repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    nz = out != 0
    return float((out != v)[nz].double().mean())


# ------------------------------------------------------------------------------------------------------------- inputs, engine
def ints(seed, shape):
    """Integer activations in [-3, 3] (conv_exact's ends-weighted draw), fp32 NCHW."""
    return cx._ints(torch.Generator(device='cpu').manual_seed(seed), shape, cx.X_MAX)


def grid8(seed, shape, lim=cx.X_MAX):
    """Skip / second-input / up operands on the 2^-3 grid, fp32 NCHW: exact in bf16 and fp16."""
    return cx._grid(torch.Generator(device='cpu').manual_seed(seed), shape, cx.RES_GRID, lim)


@contextlib.contextmanager
def issuing(device=None):
    """The issuer state InferenceEngine sets while it builds and runs layers, for blocks used outside an engine: folded weights go
    to `device`, scratch comes from a dictionary of this context's own."""
    from offsetguided_amd.models import engine as E
    E._issuer.build_device, E._issuer.ws = device, {}
    try:
        yield
    finally:
        E._issuer.build_device, E._issuer.ws = None, None


def drive_engine(eng, image, feat0, feat1, inter=None):
    """eng.forward_raw(image) of a two-stack engine with both hourglasses, their 3x3 feature convs and the bridge residual taken
    out: kps[0] sees the output of pre and hands on feat0, the junction runs on (that output | `inter`, feat0), kps[1] sees the
    junction's result and hands feat1 to the heads.  -> (head outputs, {'pre': ..., 'junction': ...}); the engine's own stem launch,
    junction call and head code run as they are."""
    seen = {}

    def kps0(x):
        seen['pre'] = x
        return feat0

    def kps1(x):
        seen['junction'] = x
        return feat1
    assert eng.stage == 1
    saved = {k: eng.__dict__[k] for k in ('pre', 'kps', 'cnvs', 'inters')}
    eng.kps, eng.cnvs, eng.inters = [kps0, kps1], [lambda x: x] * 2, [lambda x: x]
    if inter is not None:
        eng.pre = [eng.pre[0], lambda x: inter]
    try:
        outs = eng.forward_raw(image)
    finally:
        eng.__dict__.update(saved)
    return outs, seen


# ----------------------------------------------------------------------------------------------------------------- dense cases
# name -> (module constructor, input (n, c, h, w) at which the GPU engine takes the route under test, reference options).
# Shapes: the smallest planes at network channel counts that select each route (tests/test_gpu_engine_exact.py asserts the route).
DENSE_CASES = {
    # (one stage on integer inputs stays on the bias grid 2^-6, where fp16 only rounds from 32 on: s in {3, 4} keeps the sums that large)
    'cnvs-tiled': (lambda: ConvBlock(3, 256, 256), (1, 256, 80, 48), {'s_choices': (3, 4)}),
    'cnvs-splitk': (lambda: ConvBlock(3, 256, 256), (1, 256, 40, 40), {'s_choices': (3, 4)}),
    'res384-band': (lambda: Residual(384, 384), (2, 384, 10, 10), {}),
    'res512-band': (lambda: Residual(512, 512), (2, 512, 5, 5), {}),
    'res384-512-s2-band': (lambda: Residual(384, 512, stride=2), (2, 384, 10, 10), {}),
    'res384-256-wcat': (lambda: Residual(384, 256), (1, 384, 40, 40), {}),
    'res256-tiled': (lambda: Residual(256, 256), (1, 256, 80, 48), {}),
    'res256-s2-tiled': (lambda: Residual(256, 256, stride=2), (1, 256, 224, 160), {'proj_rounded': True}),
    'res256-up2': (lambda: Residual(256, 256), (1, 256, 80, 48), {'merge_up': True}),
}


def case_seed(name):
    import zlib
    return zlib.crc32(name.encode())


def dense_case(name, small=False):
    """-> (module with exact parameters, x fp32 NCHW integers, reference options; 'merge_up' holds the up tensor on the 2^-3 grid).
    small: the same block on a plane of at most 12 x 10 (the CPU path has no routes to select)."""
    make, (n, c, h, w), opts = DENSE_CASES[name]
    if small:
        h, w = min(h, 12), min(w, 10)
    seed = case_seed(name)
    torch.manual_seed(seed)
    opts = dict(opts)
    m = fill_exact(make(), seed, s_choices=opts.pop('s_choices', None))
    if opts.get('merge_up'):
        opts['merge_up'] = grid8(seed + 1, (n, m.conv2.out_channels, 2 * h, 2 * w), cx.RES_MAX)
    return m, ints(seed + 2, (n, c, h, w)), opts


def case_reference(m, x, opts, dtype, trace=None):
    kw = {k: (v.double() if torch.is_tensor(v) else v) for k, v in opts.items()}
    return staged_reference(m, x, dtype=dtype, trace=trace, **kw)


# pre is three dense stages.  Each bias is up to 4 on the 2^-6 grid, i.e. 2^(8 + s) units of the next stage's grid 2^-(6 + s): with
# s = 6 the third stage's sum of |x w| passes 2^24 units, with s = 3 it stays near 2^22.
PRE_S = (3,)


def exact_model(flags=()):
    """model_factory(['--no-pretrain'] + flags) with exact parameters in pre, the first junction and the decoded stack's heads
    (everything else keeps its random initialisation: drive_engine takes it out of the forward)."""
    import argparse
    from offsetguided_amd import models
    p = argparse.ArgumentParser()
    models.net_cli(p)
    torch.manual_seed(1)
    model, _ = models.model_factory(p.parse_args(['--no-pretrain'] + list(flags)))
    hm, off = model.headnets[0], model.headnets[1]
    hm.include_jitter_offset, off.include_scale = '--include-jitter-offset' in flags, '--include-scale' in flags    # per instance
    net = model.basenet
    for i, part in enumerate((net.pre, net.inters_[0], net.cnvs_[0])):
        fill_exact(part, 31 + i, s_choices=PRE_S if part is net.pre else None)
    for i, head in enumerate(head_convs(model)):
        fill_exact(head, 41 + i)
    return model.eval()


def head_convs(model, stage=1):
    hm, off = model.headnets[0], model.headnets[1]
    heads = [hm.hp_convs[stage], off.reg_convs[stage]]
    heads += [off.scale_convs[stage]] if off.include_scale else []
    return heads + ([hm.jitter_convs[stage]] if hm.include_jitter_offset else [])


def engine_inputs():
    """image (integers in [-1, 1]: pre is THREE dense stages in a row, the stem's sums have to stay small for the third to keep the
    precondition), feat0 / inter (2^-3 grid) for the junction, feat1 (integers in [-3, 3]) for the heads: fp32 NCHW."""
    image = torch.randint(-1, 2, (1, 3, 128, 128), generator=torch.Generator(device='cpu').manual_seed(51)).float()
    return (image, grid8(52, (1, 256, 32, 32)), ints(53, (1, 256, 32, 32)), grid8(54, (1, 256, 32, 32)))
