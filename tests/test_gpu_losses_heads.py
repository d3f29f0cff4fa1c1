"""Training with every optional head on the GPU: the fused HIP losses of all loss choices against the torch formulation on
the same device, no host synchronisation inside the fused criterion, odd shapes, training steps through train_dist.main with
device-side targets for every head, and the default step still on the two original kernels.

Tolerances are tests/test_losses.py's for this comparison: loss values 1e-5 relative, gradients rtol 1e-5 / atol 1e-7.
Where a target is not finite (or the pixel unlabelled) the fused gradient must be exactly 0; the torch formulation has 0 there
too for the element-wise losses but NaN for vector_l1 / laplace (0 * inf in the backward of norm, the reference's behaviour,
pinned by tests/test_losses_heads_cpu.py), so there the fused result is held to the exact 0 and not to the NaN."""
import numpy as np
import pytest
import torch

import losses_heads_common as common
from offsetguided_amd import _lib
from offsetguided_amd.models import losses

pytestmark = pytest.mark.gpu

KERNEL = {'l2_loss': 'og_l2_loss_f32', 'focal_l2_loss': 'og_focal_l2_loss_f32', 'vector_l1_loss': 'og_vector_l1_loss_f32',
          'offset_laplace_loss': 'og_laplace_loss_f32', 'offset_instance_l1_loss': 'og_offset_l1_loss_f32'}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")


class _Recorder:
    """libog_decoder.so as _lib.load() returns it, noting which entry points are asked for."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._lib, name)


def _no_mask_gather(monkeypatch):
    """Boolean-mask gathers (the torch formulation) raise from here on."""
    plain = torch.Tensor.__getitem__

    def getitem(self, idx):
        if isinstance(idx, torch.Tensor) and idx.dtype == torch.bool:
            raise AssertionError('boolean-mask gather inside the fused criterion')
        return plain(self, idx)
    monkeypatch.setattr(torch.Tensor, '__getitem__', getitem)


def _pairwise(finite):
    """finite (n, 2L, h, w) -> the same shape, true where BOTH components of the (x, y) vector are."""
    n, c, h, w = finite.shape
    both = finite.reshape(n, c // 2, 2, h, w).all(axis=2, keepdims=True)
    return np.broadcast_to(both, (n, c // 2, 2, h, w)).reshape(n, c, h, w)


def _defined(d, hmp, jit, off):
    """{head: bool array (n, c, h, w)}: labelled pixel and a target the loss choice accepts."""
    mask = d['mask'].numpy()
    fin = lambda k: np.isfinite(d[k].numpy())  # noqa: E731
    vec = lambda k, name: _pairwise(fin(k)) if name in ('vector_l1_loss', 'offset_laplace_loss') else fin(k)  # noqa: E731
    out = {'hm': fin('hm_gt') & mask, 'bg': fin('bg_gt') & mask, 'jit': vec('jit_gt', jit) & mask, 'off': vec('off_gt', off) & mask,
           'scale': fin('scale_gt') & mask}
    out['spread'] = out['off'][:, ::2]
    return out


def _compare(d, combo, monkeypatch):
    hmp, jit, off, sqrt_re = combo
    ref_val, ref_grad = common.run(losses, d, *combo, fused=False, device='cuda:0')
    rec = _Recorder(_lib.load())
    with monkeypatch.context() as mp:
        mp.setattr(_lib, 'load', lambda: rec)
        _no_mask_gather(mp)
        got_val, got_grad = common.run(losses, d, *combo, fused=True, device='cuda:0')
    print(common.tag(*combo), 'torch', ref_val, 'fused', got_val)
    # the kernels ran: heatmap + background, jitter, offsets, scale, for each of the two stacks
    jit_k = KERNEL.get(jit, 'og_masked_l1_loss_f32')
    off_k = KERNEL.get(off, 'og_offset_l1_loss_f32')
    want = [KERNEL[hmp]] * 4 + [jit_k] * 2 + [off_k] * 2 + ['og_masked_l1_loss_f32'] * 2
    assert sorted(n for n in rec.names if n.endswith('_loss_f32')) == sorted(want)
    assert np.all(np.abs(got_val - ref_val) <= 1e-5 * np.abs(ref_val)), (ref_val, got_val)
    assert sorted(got_grad) == sorted(ref_grad)
    defined = _defined(d, hmp, jit, off)
    for k, g in got_grad.items():
        ok = np.broadcast_to(defined[k], g.shape)
        assert np.isfinite(g).all(), k
        assert np.all(g[~ok] == 0.0), f'{k}: gradient on an unlabelled / undefined element'
        err = np.abs(g[ok] - ref_grad[k][ok])
        print(' ', k, 'elements', int(ok.sum()), 'max abs err', float(err.max(initial=0.0)))
        assert np.allclose(ref_grad[k][ok], g[ok], rtol=1e-5, atol=1e-7), k
        if {'jit': jit, 'off': off}.get(k) not in ('vector_l1_loss', 'offset_laplace_loss') or k == 'spread':
            assert np.array_equal(ref_grad[k][~ok], g[~ok]), k          # the element-wise formulations have the 0 there too
    return got_val, got_grad


@pytest.mark.parametrize("hmp,jit,off,sqrt_re", common.COMBOS, ids=[common.tag(*c) for c in common.COMBOS])
def test_fused_losses_match_torch_all_heads(hmp, jit, off, sqrt_re, monkeypatch):
    _need_gpu()
    d = common.inputs()
    _, grad = _compare(d, (hmp, jit, off, sqrt_re), monkeypatch)
    # below the margin: offset predictions that equal their target, scale predictions within MARGIN2 of theirs
    if off in ('offset_l1_loss', 'offset_instance_l1_loss', 'vector_l1_loss'):
        for s, p in enumerate(d['off']):
            same = (p == d['off_gt']).numpy()
            if off == 'vector_l1_loss':
                same = _pairwise(same)
            assert same.any() and np.all(grad['off'][s][same] == 0.0)
    for s, p in enumerate(d['scale']):
        near = ((p - d['scale_gt']).abs() < losses.MARGIN2).numpy()
        assert near.any() and np.all(grad['scale'][s][near] == 0.0)


def test_fused_criterion_never_waits_for_the_device():
    """Criterion forward + backward with every head, fused, under torch's sync debug mode: an operation that makes the host
    wait for the GPU (a boolean-mask gather's output size, .item()) raises."""
    _need_gpu()
    dev = 'cuda:0'
    d = {k: ([v.to(dev) for v in x] if isinstance(x, list) else x.to(dev)) for k, x in common.inputs().items()}
    _lib.load()

    def step(hmp, jit, off, sqrt_re):
        pred = {k: [p.clone().requires_grad_(True) for p in d[k]] for k in common.HEADS}
        crit = losses.lossfuncs_factory(['hmp', 'omp'], 2, common.STACK_WEIGHTS, hmp, jit, off, 'scale_l1_loss', sqrt_re, fused=True)
        parts = list(crit[0]((pred['hm'], pred['bg'], pred['jit']), d['hm_gt'], d['bg_gt'], d['jit_gt'], d['mask']))
        parts += list(crit[1]((pred['off'], pred['spread'], pred['scale']), d['off_gt'], d['scale_gt'], d['ps'], d['mask']))
        loss = sum(lam * l for lam, l in zip(common.LAMBDAS, parts))
        loss.backward()
        return loss.detach(), pred

    step(*common.COMBOS[0])                      # allocator and library warm-up outside the guarded region
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    results = []
    try:
        torch.cuda.set_sync_debug_mode('error')
        for combo in common.COMBOS:
            results.append(step(*combo))
    finally:
        torch.cuda.set_sync_debug_mode(before)
    for loss, pred in results:
        assert np.isfinite(float(loss))
        assert all(p.grad is not None for k in ('hm', 'bg', 'jit', 'off', 'scale') for p in pred[k])


ODD = {'hw_not_multiple_of_4': dict(h=5, w=7), 'one_image': dict(n=1, h=8, w=6), 'one_image_odd': dict(n=1, h=3, w=3),
       'masked_image': dict(masked_image=1), 'no_finite_target': dict(no_targets=True)}
ODD_COMBOS = [('l2_loss', 'vector_l1_loss', 'offset_laplace_loss', True), ('focal_l2_loss', 'offset_l1_loss', 'vector_l1_loss', False),
              ('l2_loss', 'offset_l1_loss', 'offset_instance_l1_loss', True)]


@pytest.mark.parametrize("case", sorted(ODD))
def test_fused_losses_odd_shapes(case, monkeypatch):
    _need_gpu()
    d = common.inputs(seed=23, **ODD[case])
    for combo in ODD_COMBOS:
        val, grad = _compare(d, combo, monkeypatch)
        if case == 'masked_image':
            assert all(np.all(g[:, 1] == 0.0) for g in grad.values())
        if case == 'no_finite_target':          # sum 0, count 0: 0 / (1 + 0)
            assert val[2] == 0.0 and val[3] == 0.0 and val[4] == 0.0
            assert all(np.all(grad[k] == 0.0) for k in grad if k not in ('hm', 'bg'))


def test_gpu_train_steps_all_heads_device_encoder(tmp_path, monkeypatch):
    """train_dist.main on the GPU with every optional head and the laplace offset loss: annotations -> HIP encoder (heatmaps,
    background, jitter, offsets, keypoint scales) -> fused HIP losses -> optimizer, three steps."""
    _need_gpu()
    from offsetguided_amd import encoder, models, train_dist
    from offsetguided_amd.models import networks
    saved, initial = [], {}
    monkeypatch.setattr(networks.torch, 'save', lambda data, path: saved.append((data, str(path))))
    factory = models.model_factory

    def recording_factory(args):
        model, crit = factory(args)
        initial.update({k: v.detach().clone() for k, v in model.state_dict().items()})
        return model, crit
    monkeypatch.setattr(models, 'model_factory', recording_factory)
    for cls, name in ((encoder.HeatMaps, 'include_jitter_offset'), (encoder.HeatMaps, 'include_background'),
                      (encoder.OffsetMaps, 'include_scale')):
        monkeypatch.setattr(cls, name, getattr(cls, name))          # main() sets them from the flags: put them back afterwards
    from offsetguided_amd.models import heads
    for cls in (heads.HeatMapsHead, heads.OffsetMapsHead):
        for name in ('include_spread', 'include_background', 'include_jitter_offset', 'include_scale'):
            if hasattr(cls, name):
                monkeypatch.setattr(cls, name, getattr(cls, name))
    _no_mask_gather(monkeypatch)
    train_dist.main(['--no-pretrain', '--square-length', '256', '--batch-size', '2', '--epochs', '1', '--steps-per-epoch', '3',
                     '--print-freq', '1', '--checkpoint-path', str(tmp_path), '--include-scale', '--include-jitter-offset',
                     '--include-background', '--include-spread', '--offset-loss', 'offset_laplace_loss'])
    assert encoder.HeatMaps.include_jitter_offset and encoder.HeatMaps.include_background and encoder.OffsetMaps.include_scale
    (data, path), = saved
    assert data['epoch'] == 0 and np.isfinite(data['train_loss'])
    state = data['model_state_dict']
    assert all(bool(torch.isfinite(v).all()) for v in state.values() if v.is_floating_point())
    for part in ('hp_convs', 'bghp_convs', 'jitter_convs', 'reg_convs', 'spread_convs', 'scale_convs'):
        keys = [k for k in state if ('.' + part + '.') in ('.' + k) and k.endswith('weight')]
        assert len(keys) == 2, (part, keys)
        for k in keys:
            assert not torch.equal(state[k].cpu(), initial[k].cpu()), f'{k} was not trained'

    # the targets the step trained on, in the layout the criteria expect
    joints, n_persons = train_dist.synthetic_annotations(3, 2, 256)
    encs = encoder.factory_heads(['hmp', 'omp'], 256, [4, 4], 'cuda:0')
    (hm, bg, jit, mask), (off, sc, ps, _) = train_dist.encode_targets(encs, torch.from_numpy(joints).cuda(),
                                                                       torch.from_numpy(n_persons).cuda())
    assert bg.shape == (2, 1, 64, 64) and jit.shape == (2, 2, 64, 64) and sc.shape == hm.shape == (2, 17, 64, 64)
    assert bool(torch.isfinite(jit).any()) and bool(torch.isinf(jit).any())
    assert bool(torch.isfinite(sc).any()) and bool(torch.isnan(sc).any())
    assert torch.allclose(bg, 1.0 - hm.max(dim=1, keepdim=True)[0])


def test_default_step_stays_on_the_two_original_kernels(monkeypatch):
    """Default loss choices, fused: only og_focal_l2_loss_f32 and og_offset_l1_loss_f32 are called, and the loss values equal
    those entry points called directly.  (One wave of elements per map, so each sum is a single atomic and exact equality
    does not depend on the order of the others.)"""
    _need_gpu()
    from offsetguided_amd import synth
    dev = torch.device('cuda:0')
    rng = synth.HashRng(31)
    n, c, h, w = 2, 2, 4, 4
    t = lambda lo, hi, ch=c: torch.from_numpy(rng.uniform(n * ch * h * w, lo, hi).reshape(n, ch, h, w).astype(np.float32)).to(dev)  # noqa: E731
    hm_gt, hm = t(0, 1) * (t(0, 1) > 0.5), [t(-0.2, 1.1), t(-0.2, 1.1)]
    off_gt, off = t(-60, 60), [t(-60, 60), t(-60, 60)]
    off_gt[t(0, 1) > 0.5] = float('inf')
    mask = t(0, 1, 1) > 0.2
    lib = _lib.load()
    rec = _Recorder(lib)
    monkeypatch.setattr(_lib, 'load', lambda: rec)
    crit = losses.lossfuncs_factory(['hmp', 'omp'], 2, [1, 1], 'focal_l2_loss', 'offset_l1_loss', 'offset_l1_loss', 'scale_l1_loss',
                                    False, fused=True)
    l_hm = crit[0](([p.clone().requires_grad_(True) for p in hm], [[], []], [[], []]), hm_gt, None, None, mask)
    l_off = crit[1](([p.clone().requires_grad_(True) for p in off], [[], []], [[], []]), off_gt, None, None, mask)
    assert sorted(x for x in rec.names if x.endswith('_loss_f32')) == ['og_focal_l2_loss_f32'] * 2 + ['og_offset_l1_loss_f32'] * 2
    assert l_hm[1] == 0 and l_hm[2] == 0 and l_off[1] == 0

    m8 = mask.to(torch.uint8).contiguous()
    stream = _lib.stream_ptr(dev)
    want_hm, want_off = [], []
    for p in hm:
        acc, grad = torch.zeros(1, device=dev), torch.empty_like(p)
        _lib.check(lib.og_focal_l2_loss_f32(_lib.ptr(p), _lib.ptr(hm_gt), _lib.ptr(m8), n, c, h * w, losses.TAU, losses.GAMMA,
                                            _lib.ptr(acc), _lib.ptr(grad), stream), lib)
        want_hm.append(acc[0] * 0.5)
    ones = torch.ones_like(off_gt)
    for p in off:
        acc, grad = torch.zeros(2, device=dev), torch.empty_like(p)
        _lib.check(lib.og_offset_l1_loss_f32(_lib.ptr(p), _lib.ptr(off_gt), _lib.ptr(ones), _lib.ptr(m8), n, c, h * w,
                                             losses.MARGIN, 0, _lib.ptr(acc), _lib.ptr(grad), stream), lib)
        want_off.append(acc[0] / (1.0 + acc[1]) * 0.5)
    assert float(l_hm[0]) == float(sum(want_hm) / n) and float(l_hm[0]) > 0
    assert float(l_off[0]) == float(sum(want_off) / n) and float(l_off[0]) > 0
