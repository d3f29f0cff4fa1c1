"""Shared by the engine-refresh tests: the fold rule of include/og_decoder.h ("weight refresh") restated in numpy, a seeded
perturbation of every weight of a model, and the list of a weight bundle's persistent tensors."""
import argparse

import numpy as np
import torch


def to_lp(x, dtype):
    """fp32 array -> the bit patterns (uint16) of the values rounded to nearest even in fp16 / bf16."""
    x = np.ascontiguousarray(x, np.float32)
    if dtype == torch.float16:
        with np.errstate(over='ignore'):
            return x.astype(np.float16).view(np.uint16)         # IEEE conversion: beyond the range -> inf, subnormals kept
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7fc0), r)


def folded_bias(cout, bias, bn):
    """b' and the scale (None without BN): every operation one rounded fp32 operation.  bn = (gamma, beta, mean, var, eps) or None."""
    f = np.float32
    b = np.zeros(cout, f) if bias is None else np.asarray(bias, f)
    if bn is None:
        return b, None
    gamma, beta, mean, var, eps = bn
    with np.errstate(divide='ignore', invalid='ignore', over='ignore', under='ignore'):
        s = np.asarray(var, f) + f(eps)
        r = np.sqrt(s)
        scale = np.asarray(gamma, f) / r
        d = b - np.asarray(mean, f)
        m = d * scale
        return m + np.asarray(beta, f), scale


def fold_reference(w, bias, bn, dtype, partner=None):
    """The rule for one layer.  w: (Cout, Cin, kh, kw) fp32 (logical order, whatever its memory); partner = (bias, bn) of the layer
    whose folded bias is added.  -> (w16 (Cout, kh, kw, Cin) uint16, b32 (Cout,) fp32, b16 (Cout,) uint16)."""
    w = np.asarray(w, np.float32)
    b, scale = folded_bias(w.shape[0], bias, bn)
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        if scale is not None:
            w = w * scale[:, None, None, None]
        if partner is not None:
            b = b + folded_bias(w.shape[0], *partner)[0]
    return to_lp(w.transpose(0, 2, 3, 1), dtype), b, to_lp(b, dtype)


def bits16(t):
    """A 16-bit torch tensor's bit patterns as a numpy uint16 array (bf16 has no numpy type)."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def make_model():
    from offsetguided_amd import models
    p = argparse.ArgumentParser()
    models.net_cli(p)
    torch.manual_seed(0)
    model, _ = models.model_factory(p.parse_args(['--no-pretrain']))
    return model


def perturb(model, seed):
    """Change every conv weight, conv bias and BatchNorm tensor in place (seeded; the values do not depend on the device).  Per
    channel: sigma^2 log-uniform over 1e-4 .. 1e2 with a few exact zeros, gamma = g * sqrt(sigma^2 + eps) with g log-uniform over
    1e-2 .. 0.7 (gamma itself then spans five decades) and a few exact zeros, means and betas of both signs; conv weights
    N(0, 1 / fan_in): a forward through the 104 layers stays finite in fp16."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda n: torch.rand(n, generator=g)            # noqa: E731
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.Conv2d):
                fan_in = m.weight[0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / fan_in ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                n = m.num_features
                var = 10.0 ** (rnd(n) * 6 - 4)
                var[rnd(n) < 0.03] = 0.0
                gamma = 10.0 ** (rnd(n) * 1.85 - 2) * torch.sqrt(var + m.eps)
                gamma[rnd(n) < 0.03] = 0.0
                m.running_var.copy_(var)
                m.weight.copy_(gamma)
                m.running_mean.copy_(0.1 * torch.randn(n, generator=g))
                m.bias.copy_(0.1 * torch.randn(n, generator=g))
    return model


def persistent(layers):
    """{name: tensor} of every persistent weight buffer of a bundle (models/engine.py:_Layers) that exists right now."""
    out = {}
    for i, (c, _) in enumerate(layers._convs()):
        for field in ('w', 'b32', 'b', 'w_tiled', 'w_band', 'w_alt'):
            t = getattr(c, field)
            if t is not None:
                out[f'{i}:{c.name}.{field}'] = t
    for field in ('stem_w', 'heads_w', 'heads_b'):
        if getattr(layers, field) is not None:
            out[field] = getattr(layers, field)
    if layers.heads_tiled is not None:
        out['heads_tiled.w'], out['heads_tiled.b'] = layers.heads_tiled[:2]
    return out
