"""Numpy restatement of the optimizer kernels (include/og_decoder.h, "training step without a host wait"; csrc/optim.hip), dtype
generic: every line is one numpy operation, so one rounding in the arrays' dtype.  In float32 it is what the GPU tests compare with
bit for bit; in float64 the CPU tests hold it against torch.optim.Adam / AdamW / SGD.  The scalars are computed in Python doubles and
rounded to the dtype once, as the host side of the kernels does."""
import math

import numpy as np


def adam_scalars(dtype, lr, betas, eps, wd, t):
    b1, b2 = betas
    return [dtype(x) for x in (lr, b1, b2, 1.0 - b1, 1.0 - b2, eps, wd, 1.0 - b1 ** t, 1.0 - b2 ** t)]


def scaled_gradient(g, scale):
    """ge = (scale == 0) ? 0 : g * scale -- a dropped batch contributes exactly zero, even where g is inf / NaN."""
    if scale == 0:
        return np.zeros_like(g)
    return g * g.dtype.type(scale)


def adam_step(p, g, m, v, *, lr, betas=(0.9, 0.999), eps=1e-8, wd=0.0, t, adam_w_mode, scale=1.0):
    """One Adam step at step count t (1 for the first) -> (p', m', v')."""
    dtype = p.dtype.type
    lr, b1, b2, omb1, omb2, eps, wd, bc1, bc2 = adam_scalars(dtype, lr, betas, eps, wd, t)
    ge = scaled_gradient(g, scale)
    if wd != 0 and not adam_w_mode:
        t_ = wd * p
        ge = ge + t_
    a = b1 * m
    b = omb1 * ge
    m2 = a + b
    c = b2 * v
    d = omb2 * ge
    e = d * ge
    v2 = c + e
    mh = m2 / bc1
    q = v2 / bc2
    r = np.sqrt(q)
    den = r + eps
    u = mh / den
    if wd != 0 and adam_w_mode:
        t_ = wd * p
        u = u + t_
    s = lr * u
    return p - s, m2, v2


def sgd_step(p, g, buf, *, lr, mom=0.0, wd=0.0, first, scale=1.0):
    """One SGD step (dampening 0, no Nesterov) -> (p', buf'); buf is None and stays None with mom == 0."""
    dtype = p.dtype.type
    lr, mom, wd = dtype(lr), dtype(mom), dtype(wd)
    ge = scaled_gradient(g, scale)
    if wd != 0:
        t_ = wd * p
        ge = ge + t_
    if mom != 0:
        if first:
            buf = ge
        else:
            t_ = mom * buf
            buf = t_ + ge
        step = buf
    else:
        step, buf = ge, None
    s = lr * step
    return p - s, buf


def sum_of_squares(grads):
    """The exactly rounded sum of the squares (each fp32 square is exact in double; math.fsum rounds the exact sum once)."""
    return math.fsum(float(x) * float(x) for g in grads for x in np.asarray(g, dtype=np.float64).ravel())


def step_scale(n2, loss=None, loss_limit=1e8, max_norm=math.inf):
    """The scale block from the double sum of squares -> (scale fp32, norm fp32, dropped bool)."""
    with np.errstate(invalid='ignore'):
        norm = np.float32(np.sqrt(np.float64(n2)))
    drop = (loss is not None and np.float32(loss) > np.float32(loss_limit)) or not math.isfinite(n2)
    if drop:
        return np.float32(0), norm, True
    if math.isfinite(max_norm):
        den = norm + np.float32(1e-6)
        c = np.float32(max_norm) / den
        return (c if c < 1 else np.float32(1)), norm, False
    return np.float32(1), norm, False


def magnitudes(rs, n, lo=1e-6, hi=1e3):
    """n fp32 values with random signs, magnitudes log-uniform in lo .. hi: no intermediate of an update is subnormal."""
    return (np.exp(rs.uniform(np.log(lo), np.log(hi), n)) * rs.choice([-1.0, 1.0], n)).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)
