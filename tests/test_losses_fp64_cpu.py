"""tests/losses_fp64.py, the float64 restatement the GPU loss tests measure the HIP kernels against, held to models/losses.py
itself: the torch formulation run in float64 on the CPU with autograd, all six loss choices, both sqrt_re settings, gamma in
{1, 2, 0.5}, every shape of the GPU tests but the two largest.  Values and gradients agree to 1e-12 relative (_close) wherever torch's
gradient is finite; where torch leaves NaN (the norm backward next to an undefined target, |x|^gamma at x = 0 for gamma < 1)
the restatement has the exact 0 the kernels write.  (tests/golden/losses.npz and losses_heads.npz tie that formulation to the
reference bit for bit in float32.)

The second half checks the input conditions the GPU tests rely on, for every generated case including the largest: at most 4
borderline elements, counts below 2^24, the exact-sum cases below 2^24 quanta, and kept, dropped and masked elements present."""
import numpy as np
import pytest
import torch

import losses_fp64 as ref64
from offsetguided_amd.models import losses


def _torch_run(case):
    """models/losses.py in float64 -> (value, count-scaled gradient of pred, of logb or None)."""
    k = case['kernel']
    n, c, hw = case['pred'].shape
    t64 = lambda a: torch.from_numpy(a.astype(np.float64)).reshape(a.shape[0], a.shape[1], hw, 1)  # noqa: E731
    pred, gt = t64(case['pred']).requires_grad_(True), t64(case['gt'])
    mask = torch.from_numpy(case['mask'] != 0).reshape(n, 1, hw, 1)
    logb = None
    if k == 'focal':
        tau, gamma = float(case['tau']), float(case['gamma'])
        val = losses.tensor_loss(pred, gt, mask, lambda s, t: losses.focal_l2(s, t, tau, gamma)).sum()
    elif k == 'l2':
        val = losses.LossChoice.l2_loss(pred, gt, mask).sum()
    else:
        if k == 'ml1':
            err = losses.LossChoice.scale_l1_loss(pred, gt, mask)
        elif k == 'offset':
            err = losses.LossChoice.offset_instance_l1_loss(pred, gt, t64(case['ps']), None, mask)
        elif k == 'vector':
            err = losses.LossChoice.vector_l1_loss(pred, gt, None, None, mask)
        else:
            logb = t64(case['logb']).requires_grad_(True)
            err = losses.LossChoice.offset_laplace_loss(pred, gt, None, logb, mask)
        val = losses._margin_mean(err, float(case['margin']), bool(case['sqrt_re']))
    val.backward()
    g = lambda x: None if x is None else x.grad.numpy().reshape(x.shape[:3])  # noqa: E731
    return float(val.detach()), g(pred), g(logb)


def _close(got, want, scale, what):
    """1e-12 relative to the gradient, plus 8 float64 roundings (2^-53 each) of the magnitude of the terms it is made of where
    those cancel (focal: |A| + |B|; grad_logb: 1 + r exp(-logb); under a root: (|p/ps| + |g/ps|) / e, (|logb| + r inv) / v)."""
    fin = np.isfinite(got)
    assert np.all(want[~fin] == 0.0), f'{what}: not 0 where torch has NaN'
    assert np.all(np.isfinite(want)), what
    err = np.abs(got[fin] - want[fin])
    assert np.all(err <= (1e-12 * np.abs(want) + 8 * 2.0 ** -53 * scale)[fin]), (what, float(err.max(initial=0.0)))
    return int((~fin).sum())


CPU_CASES = [c for k in ref64.KERNELS for c in ref64.case_list(k) if c[1][0] not in ref64.LARGEST]


@pytest.mark.parametrize("cid,shape,variant,seed,flags", CPU_CASES, ids=[c[0] for c in CPU_CASES])
def test_restatement_matches_torch_float64(cid, shape, variant, seed, flags):
    case = ref64.make_case(cid.split('-')[0], shape, variant, seed, **flags)
    ref = ref64.reference(case)
    ref64.check_conditions(case, ref)
    val, grad, grad_b = _torch_run(case)
    denom = 1.0 if case['kernel'] in ('focal', 'l2') else 1.0 + ref.count
    assert abs(val - ref.sum / denom) <= 1e-12 * abs(ref.sum / denom), (val, ref.sum, ref.count)
    nans = _close(grad * denom, ref.grad, ref.scale64, 'grad')
    if grad_b is not None:
        nans += _close(grad_b * denom, ref.grad_logb, ref.scale64_logb, 'grad_logb')
    if case['kernel'] in ('focal', 'l2', 'ml1', 'offset') and float(case.get('gamma', 1)) >= 1:
        assert nans == 0                        # the element-wise formulations have the 0 themselves
    # dropped and masked elements have the exact 0
    kept = ref.kept if ref.grad.shape == ref.kept.shape else np.repeat(ref.kept, 2, axis=1)
    assert np.all(ref.grad[~kept] == 0.0) and np.all(ref.gbound[~kept] == 0.0) and np.all(ref.chk[~kept] == 0.0)
    # the float32 continuation differs from the exact gradient by no more than the conditioning it removes
    assert np.all(np.abs(ref.chk - ref.grad) <= ref.gbound) and not (ref.cont & ~ref.kept).any()


REST = [c for k in ref64.KERNELS for c in ref64.case_list(k) if c[1][0] in ref64.LARGEST]
REST += [c for k in ref64.EXACT for c in ref64.exact_case_list(k)]


@pytest.mark.parametrize("cid,shape,variant,seed,flags", REST, ids=[c[0] for c in REST])
def test_input_conditions_of_the_largest_and_exact_cases(cid, shape, variant, seed, flags):
    case = ref64.make_case(cid.split('-')[0], shape, variant, seed, **flags)
    ref = ref64.reference(case)
    ref64.check_conditions(case, ref)
    if case['exact']:
        # every term is a multiple of the quantum, and float32 arithmetic on these inputs is exact: sum and gradient are float32
        assert np.all(ref.grad.astype(np.float32).astype(np.float64) == ref.grad)
        assert np.float64(np.float32(ref.sum)) == ref.sum


def test_planted_edges_follow_the_rules():
    """e == float32(margin) is kept, one float32 below is dropped, neither is borderline; t == float32(tau) is foreground;
    s in {0, 1} gives |1 - st| = 0 with a finite (zero) focal derivative; d == 0 is dropped and norm'(0) = 0."""
    m = ref64.MARGIN2
    below = np.nextafter(m, np.float32(0))
    pred = np.array([m, -m, below, 2 * m, 0, 5], np.float32).reshape(1, 1, 6)
    gt = np.array([0, 0, 0, m, m, 5], np.float32).reshape(1, 1, 6)
    mask = np.ones((1, 6), np.uint8)
    for fn in (lambda: ref64.masked_l1(pred, gt, mask, m, 0), lambda: ref64.offset_l1(pred, gt, np.ones_like(pred), mask, m, 0)):
        r = fn()
        assert r.kept.ravel().tolist() == [True, True, False, True, True, False] and not r.borderline.any()
        assert r.grad.ravel().tolist() == [1, -1, 0, 1, -1, 0] and r.count == 4
    tau = ref64.TAU
    for gamma in (1, 2, 0.5):
        s = np.array([0.3, 0.3, 1.0, 0.0, 1.0], np.float32).reshape(1, 1, 5)
        t = np.array([tau, np.nextafter(tau, np.float32(0)), 0.5, 0.0, 1.0], np.float32).reshape(1, 1, 5)
        r = ref64.focal_l2(s, t, mask[:, :5], tau, np.float32(gamma))
        s64, t64 = s.astype(np.float64).ravel(), t.astype(np.float64).ravel()
        fg_term = 0.5 * (s64[0] - t64[0]) ** 2 * (1 - s64[0]) ** gamma
        bg_term = 0.5 * (s64[1] - t64[1]) ** 2 * s64[1] ** gamma
        assert abs(r.sum - fg_term - bg_term) <= 1e-15 and np.all(np.isfinite(r.grad))
        assert np.all(r.grad.ravel()[2:] == 0.0)
    # vector: p == g gives r = 0: dropped by a positive margin; kept by the laplace value logb with gradient 0 to pred, k to logb
    p = np.array([1.5, -2.0], np.float32).reshape(1, 2, 1)
    r = ref64.vector_l1(p, p.copy(), mask[:, :1], ref64.MARGIN, 1)
    assert r.count == 0 and np.all(r.grad == 0)
    for lb, kept in ((0.25, True), (-0.25, False), (np.nan, False), (-np.inf, False)):
        r = ref64.laplace(p, p.copy(), np.full((1, 1, 1), lb, np.float32), mask[:, :1], ref64.MARGIN, 0)
        assert bool(r.kept.all()) == kept and np.all(r.grad == 0) and float(r.grad_logb.ravel()[0]) == (1.0 if kept else 0.0)
        assert r.sum == (0.25 if kept else 0.0)
    # non-finite targets are dropped
    g = np.array([np.inf, -np.inf, np.nan], np.float32).reshape(1, 1, 3)
    r = ref64.l2(np.zeros_like(g), g, mask[:, :3])
    assert r.count == 0 and r.sum == 0 and np.all(r.grad == 0)


def test_geometry_of_the_cases():
    """The shapes reach what their names say: units on either side of the grid cap on both paths, the small unit counts."""
    for k in ref64.KERNELS:
        for name, n, cp, hw in ref64.CAP_SHAPES + ref64.SMALL_V1 + ref64.SMALL_V4:
            v, units, blocks, m, w = ref64.geometry(k, n, cp, hw)
            if k not in ref64.HAS_V:
                assert v == 1
                continue
            assert v == (4 if name.startswith('v4') else 1), (k, name)
            want = {'cap-1': ref64.CAP - 1, 'cap': ref64.CAP, 'cap+1': ref64.CAP + 1}.get(name[3:]) or int(name[4:])
            assert units == want, (k, name, units)
            assert blocks == min(2048, -(-units // 256)) and m == (2 if units > ref64.CAP else 1) * v
        v, units, blocks, m, w = ref64.geometry(k, *ref64.TRAIN[k][1:])
        assert blocks == 2048 and w == 8192 and m == {'focal': 5, 'offset': 10}.get(k, 8)
