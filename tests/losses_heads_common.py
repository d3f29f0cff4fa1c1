"""Inputs and the criterion run shared by the all-heads loss tests (CPU golden, GPU fused vs torch) and by
tools/gen_golden_losses_heads.py: every head present (heatmap, background, jitter, guiding offsets, spread, keypoint scale), two
stacks, the 32 combinations of heatmap loss x jitter loss x offset loss x sqrt_re."""
import itertools

import numpy as np
import torch

from offsetguided_amd import synth

LAMBDAS = [1.0, 1.0, 100.0, 100.0, 0.01]        # the CLI's defaults: hmp, background, jitter, offset, scale
STACK_WEIGHTS = [1, 3]
HEADS = ('hm', 'bg', 'jit', 'off', 'spread', 'scale')
COMBOS = list(itertools.product(('l2_loss', 'focal_l2_loss'), ('offset_l1_loss', 'vector_l1_loss'),
                                ('offset_l1_loss', 'offset_instance_l1_loss', 'vector_l1_loss', 'offset_laplace_loss'),
                                (False, True)))


def tag(hmp, jit, off, sqrt_re):
    return f'{hmp}-{jit}-{off}-{int(sqrt_re)}'


class PortableExp(torch.autograd.Function):
    """torch.exp on the CPU with a forward that does not depend on the processor: exp in float64, rounded to float32 (torch's own
    float32 exp is a vector routine with different last bits per instruction set, like the sqrt tests/test_losses.py:IeeeSqrt
    replaces), and torch's own backward, grad * result.  The golden cases use it on both sides."""

    @staticmethod
    def forward(ctx, x):
        r = torch.from_numpy(np.exp(x.detach().numpy().astype(np.float64)).astype(np.float32))
        ctx.save_for_backward(r)
        return r

    @staticmethod
    def backward(ctx, g):
        (r,) = ctx.saved_tensors
        return g * r


def vector_holes(rng, n, pairs, h, w, undefined=0.7, single=0.01):
    """bool (n, 2 * pairs, h, w): where an (x, y) target is undefined.  Both components of a vector (as the encoder writes
    them) in `undefined` of the cells; in a few cells (`single`) one component only."""
    both = rng.uniform(n * pairs * h * w).reshape(n, pairs, 1, h, w) < undefined
    one = rng.uniform(n * pairs * 2 * h * w).reshape(n, pairs, 2, h, w) < single
    return torch.from_numpy((both | one).reshape(n, 2 * pairs, h, w))


def inputs(seed=11, n=2, h=24, w=24, limbs=19, n_kp=17, masked_image=None, no_targets=False):
    """dict of CPU tensors: predictions are lists over the two stacks.  Offset predictions equal their target in some cells
    (error 0: below the margin; laplace value = logb there, negative in part), scale predictions lie within MARGIN2 of it in
    some.  masked_image: that image of the batch is all unlabelled; no_targets: no finite jitter / offset / scale target."""
    rng = synth.HashRng(seed)
    t = lambda c, lo, hi: torch.from_numpy(rng.uniform(n * c * h * w, lo, hi).reshape(n, c, h, w).astype(np.float32))  # noqa: E731
    d = {}
    d['hm_gt'] = t(n_kp, 0, 1) * (t(n_kp, 0, 1) > 0.8)                       # sparse: most targets are background (< tau)
    d['hm'] = [t(n_kp, -0.2, 1.1), t(n_kp, -0.2, 1.1)]
    d['bg_gt'] = 1.0 - d['hm_gt'].max(dim=1, keepdim=True)[0]
    d['bg'] = [t(1, -0.2, 1.1), t(1, -0.2, 1.1)]
    d['jit_gt'] = t(2, -0.5, 0.5)
    d['jit_gt'][vector_holes(rng, n, 1, h, w)] = float('inf')
    d['jit'] = [t(2, -1, 1), t(2, -1, 1)]
    d['off_gt'] = t(2 * limbs, -60, 60)
    d['off_gt'][vector_holes(rng, n, limbs, h, w)] = float('inf')
    d['off'] = []
    for _ in range(2):
        p, same = t(2 * limbs, -60, 60), vector_holes(rng, n, limbs, h, w, undefined=0.1, single=0.0)
        same &= torch.isfinite(d['off_gt'])
        p[same] = d['off_gt'][same]
        d['off'].append(p)
    d['spread'] = [t(limbs, -2, 3), t(limbs, -2, 3)]
    d['scale_gt'] = t(n_kp, 1, 12)
    d['scale_gt'][t(n_kp, 0, 1) > 0.3] = float('nan')
    d['scale'] = []
    for _ in range(2):
        p, near = t(n_kp, 0, 13), t(n_kp, 0, 1) < 0.1
        near &= torch.isfinite(d['scale_gt'])
        p[near] = d['scale_gt'][near] + 0.05
        d['scale'].append(p)
    d['ps'] = t(1, 20, 300)
    d['mask'] = t(1, 0, 1) > 0.15
    if masked_image is not None:
        d['mask'][masked_image] = False
    if no_targets:
        d['jit_gt'][:] = float('inf')
        d['off_gt'][:] = float('inf')
        d['scale_gt'][:] = float('nan')
    return d


def run(mod, d, hmp, jit, off, sqrt_re, fused=False, device='cpu'):
    """Both criteria of `mod` (a models/losses.py) on the inputs, weighted like train_step, backward.
    -> (five losses as float32, {head: gradients stacked over the stacks})."""
    dev = lambda x: [v.to(device) for v in x] if isinstance(x, list) else x.to(device)  # noqa: E731
    d = {k: dev(v) for k, v in d.items()}
    pred = {k: [p.clone().requires_grad_(True) for p in d[k]] for k in HEADS}
    choice = lambda name: getattr(mod.LossChoice, name)  # noqa: E731
    extra = (fused,) if fused else ()                    # the reference's classes have no such argument
    hl = mod.HeatMapsLoss('hmp', 2, STACK_WEIGHTS, choice(hmp), choice(jit), sqrt_re, *extra)
    ol = mod.OffsetMapsLoss('omp', 2, STACK_WEIGHTS, choice(off), choice('scale_l1_loss'), sqrt_re, *extra)
    parts = list(hl((pred['hm'], pred['bg'], pred['jit']), d['hm_gt'], d['bg_gt'], d['jit_gt'], d['mask']))
    parts += list(ol((pred['off'], pred['spread'], pred['scale']), d['off_gt'], d['scale_gt'], d['ps'], d['mask']))
    sum(lam * l for lam, l in zip(LAMBDAS, parts)).backward()
    grads = {}
    for k in HEADS:
        if k == 'spread' and off != 'offset_laplace_loss':       # only the laplace loss reads the spread head
            assert all(p.grad is None for p in pred[k])
            continue
        grads[k] = np.stack([p.grad.cpu().numpy() for p in pred[k]])
    return np.array([float(l.detach()) for l in parts], np.float32), grads


def grad_slice(g):
    """The part of a stacked gradient (stacks, n, c, h, w) the fixture stores."""
    return g[:, :, ::(3 if g.shape[2] > 3 else 1), ::4, ::4]
