"""Numpy restatement of the weight average (include/og_decoder.h, "weight average"; csrc/optim.hip, offsetguided_amd.optim.ModelEma),
dtype generic like optim_common: every line is one numpy operation, so one rounding in the arrays' dtype.  In float32 it is what the
GPU tests compare with bit for bit.  omd = 1 - decay is computed in Python doubles and rounded to the dtype once, as the host does."""
import numpy as np

import optim_common as oc


def decay_at(decay, warmup, t):
    """The decay of the update after t updates (double): min(decay, (1 + t) / (10 + t)) with warm-up, else decay."""
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def omd_at(decay, warmup, t, dtype=np.float32):
    return dtype(1.0 - decay_at(decay, warmup, t))


def ema_step(e, x, omd):
    """d = x - e;  t = omd * d;  e' = e + t"""
    omd = e.dtype.type(omd)
    d = x - e
    t = omd * d
    return e + t


def adam_step_ema(p, g, m, v, e, omd, **kw):
    """optim_common.adam_step, then the average of the p' it returns -> (p', m', v', e')."""
    p2, m2, v2 = oc.adam_step(p, g, m, v, **kw)
    return p2, m2, v2, ema_step(e, p2, omd)


def sgd_step_ema(p, g, buf, e, omd, **kw):
    """optim_common.sgd_step, then the average of the p' it returns -> (p', buf', e')."""
    p2, buf2 = oc.sgd_step(p, g, buf, **kw)
    return p2, buf2, ema_step(e, p2, omd)
