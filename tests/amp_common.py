"""Numpy restatement of the loss-scaler scale block (include/og_decoder.h, og_step_scale_amp_f32; csrc/optim.hip): every line is one
rounded operation, fp32 unless it says double, as the header writes them.  The clip coefficient is optim_common.step_scale's."""
import math

import numpy as np

import optim_common as oc

F = np.float32


def amp_step_scale(n2, S, unskipped, *, dynamic=True, scale_factor=2.0, scale_window=2000, min_scale=1.0, max_scale=2.0 ** 24,
                   loss=None, loss_limit=1e8, max_norm=math.inf):
    """One step of the block from the double sum of squares of the SCALED gradients, the loss scale S and the count of unskipped
    steps -> (scale fp32, norm fp32, S' fp32, unskipped', overflow bool, dropped bool).  dropped: the dropped-batch counter moves
    (a loss above the limit, or an overflow under a static scale); a dynamic overflow is counted by `overflow` alone."""
    S, factor, lo, hi = F(S), F(scale_factor), F(min_scale), F(max_scale)
    overflow = not math.isfinite(n2)
    with np.errstate(invalid='ignore'):
        r = np.sqrt(np.float64(n2))
        q = r / np.float64(S)
    norm = F(q)
    if overflow:
        if not dynamic:
            return F(0), norm, S, unskipped, True, True
        t = S / factor
        return F(0), norm, (lo if t < lo else t), 0, True, False
    dropped = loss is not None and F(loss) > F(loss_limit)
    if dropped:
        scale = F(0)
    else:
        inv = F(1) / S
        # step_scale takes a sum of squares: an fp32 norm's square is exact in double and its root is the norm again
        c, _, _ = oc.step_scale(float(norm) * float(norm), max_norm=max_norm)
        scale = c * inv
    if not dynamic:
        return scale, norm, S, unskipped, False, dropped
    u = unskipped + 1
    if u == scale_window:
        t = S * factor
        S = hi if t > hi else t
        u = 0
    return scale, norm, S, u, False, dropped
