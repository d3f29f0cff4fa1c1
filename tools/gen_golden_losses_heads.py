#!/usr/bin/env python3
"""Golden values for the training losses with every head present (background, jitter offsets, spread, keypoint scale) from the
imported reference models/losses.py (build container only): the 32 combinations of heatmap loss x jitter loss x offset loss x
sqrt_re of tests/losses_heads_common.py.  Asserts that the torch formulation of offsetguided_amd/models/losses.py equals the
reference bit for bit (the five loss values and every gradient, the spread head's included), then stores the values and a strided
slice of every gradient in tests/golden/losses_heads.npz.  torch.sqrt is tests/test_losses.py:IeeeSqrt and torch.exp is
losses_heads_common.PortableExp on both sides (the processor's vector routines differ in the last bit between processors).

Where an offset target is not finite the vector / laplace formulations leave NaN in the gradient (0 * inf in the backward of
norm), in the reference and here alike; the fixture stores them as they are."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
from offsetguided_amd.models import losses as mine  # noqa: E402
from tools.gen_golden_losses import load_reference_losses  # noqa: E402


def main():
    ref = load_reference_losses()
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import losses_heads_common as common
    from test_losses import IeeeSqrt
    torch.sqrt = IeeeSqrt.apply          # the reference and ours alike
    torch.exp = common.PortableExp.apply
    inp = common.inputs()
    out, n_nan = {}, 0
    for combo in common.COMBOS:
        r_val, r_grad = common.run(ref, inp, *combo)
        m_val, m_grad = common.run(mine, inp, *combo)
        assert np.array_equal(r_val, m_val) and np.isfinite(r_val).all(), (combo, r_val, m_val)
        assert sorted(r_grad) == sorted(m_grad)
        t = common.tag(*combo)
        out[t + '/losses'] = r_val
        for k, g in r_grad.items():
            assert np.array_equal(g, m_grad[k], equal_nan=True), (combo, k)
            assert np.any(g != 0), (combo, k)
            out[f'{t}/g_{k}'] = common.grad_slice(g)
            n_nan += int(np.isnan(out[f'{t}/g_{k}']).sum())
        print(t, r_val)
    np.savez_compressed(os.path.join(ROOT, 'tests', 'golden', 'losses_heads.npz'), **out)
    print(f'losses with all heads: torch formulation bit-identical to the reference on CPU for {len(common.COMBOS)} combinations; '
          f'fixture written ({n_nan} NaN gradient entries next to non-finite offset targets)')


if __name__ == '__main__':
    main()
