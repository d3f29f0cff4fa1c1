"""Training with every optional head, the part that needs no GPU: the torch formulation of all loss choices against the
reference's values and gradients (golden), a CPU training step with all heads, and the argument checks of the four fused
loss entry points."""
import numpy as np
import pytest
import torch

import losses_heads_common as common
from helpers import GOLDEN
from offsetguided_amd import _lib
from offsetguided_amd.models import losses
from test_losses import IeeeSqrt


@pytest.mark.parametrize("hmp,jit,off,sqrt_re", common.COMBOS, ids=[common.tag(*c) for c in common.COMBOS])
def test_torch_formulation_matches_reference_golden_all_heads(hmp, jit, off, sqrt_re, monkeypatch):
    """Bit for bit (a NaN equals a NaN: next to a non-finite offset target the vector / laplace formulations leave 0 * inf in
    the gradient, in the reference too -- tools/gen_golden_losses_heads.py)."""
    g = np.load(f"{GOLDEN}/losses_heads.npz")
    monkeypatch.setattr(torch, "sqrt", IeeeSqrt.apply)              # as the fixture was computed
    monkeypatch.setattr(torch, "exp", common.PortableExp.apply)
    values, grads = common.run(losses, common.inputs(), hmp, jit, off, sqrt_re)
    t = common.tag(hmp, jit, off, sqrt_re)
    assert np.array_equal(values, g[t + "/losses"])
    stored = sorted(k.split("/g_")[1] for k in g.files if k.startswith(t + "/g_"))
    assert stored == sorted(grads) and ("spread" in grads) == (off == "offset_laplace_loss")
    for k in grads:
        assert np.array_equal(common.grad_slice(grads[k]), g[f"{t}/g_{k}"], equal_nan=True), k


class TinyHeadsNet(torch.nn.Module):
    """Stand-in with the NetworkWrapper output nesting and every optional head."""
    channels = dict(hm=17, bg=1, jit=2, off=38, spread=19, scale=17)

    def __init__(self):
        super().__init__()
        self.body = torch.nn.Conv2d(3, 8, 3, stride=4, padding=1)
        self.heads = torch.nn.ModuleDict({k: torch.nn.ModuleList([torch.nn.Conv2d(8, c, 1) for _ in range(2)])
                                          for k, c in self.channels.items()})

    def forward(self, x):
        f = torch.relu(self.body(x))
        o = {k: [conv(f) for conv in convs] for k, convs in self.heads.items()}
        return [(o['hm'], o['bg'], o['jit']), (o['off'], o['spread'], o['scale'])]


def test_train_step_all_heads_cpu(tmp_path, monkeypatch):
    """train_dist's CPU step with --include-scale --include-jitter-offset --include-background --include-spread and the laplace
    offset loss: the synthetic targets carry every map, five finite per-head losses, every head is trained."""
    from offsetguided_amd import models, train_dist
    torch.manual_seed(0)
    flags = ['--no-pretrain', '--include-scale', '--include-jitter-offset', '--include-background', '--include-spread',
             '--offset-loss', 'offset_laplace_loss', '--square-length', '64', '--batch-size', '2']
    args = train_dist.train_cli(flags)
    crit = losses.lossfuncs_factory(args.headnets, 2, args.stack_weights, args.hmp_loss, args.jitter_offset_loss,
                                    args.offset_loss, args.scale_loss, args.sqrt_re, fused=args.fused_losses)
    annos = train_dist.synthetic_targets(3, 2, 64, torch.device('cpu'), background=args.include_background,
                                         jitter=args.include_jitter_offset, scale=args.include_scale)
    (hm, bg, jit, mask), (off, sc, ps, _) = annos
    assert bg.shape == (2, 1, 16, 16) and jit.shape == (2, 2, 16, 16) and sc.shape == hm.shape == (2, 17, 16, 16)
    assert torch.isinf(jit).any() and torch.isfinite(jit).any() and torch.isnan(sc).any() and torch.isfinite(sc).any()
    assert torch.equal(torch.isfinite(jit[:, 0]), torch.isfinite(jit[:, 1]))
    net = TinyHeadsNet()
    seen = {}
    opt = torch.optim.SGD(net.parameters(), lr=0.0)     # the step itself is not the subject: keep the gradients to look at
    loss, parts = train_dist.train_step(net, crit, opt, torch.randn(2, 3, 64, 64), annos, args.lambdas, autocast_dtype=None)
    assert len(parts) == 5 and all(np.isfinite(p) and p > 0 for p in parts) and np.isfinite(float(loss))
    for k, convs in net.heads.items():
        for conv in convs:
            seen[k] = conv.weight.grad
            assert conv.weight.grad is not None and bool((conv.weight.grad != 0).any()), k
            if k != 'off':      # the laplace formulation's backward leaves NaN next to inf targets (see the golden test)
                assert bool(torch.isfinite(conv.weight.grad).all()), k

    # the same flags through main() (the criterion and the pool are built from them there), model replaced by the stand-in
    monkeypatch.setattr(models, 'model_factory', lambda a: (TinyHeadsNet(), crit))
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    train_dist.main(flags + ['--epochs', '1', '--steps-per-epoch', '2', '--print-freq', '1', '--checkpoint-path', str(tmp_path)])
    ck = torch.load(tmp_path / 'PoseNet_0_epoch.pth', map_location='cpu')
    assert ck['epoch'] == 0 and any('heads.scale' in k for k in ck['model_state_dict'])


def test_jitter_laplace_is_refused_at_factory_time():
    with pytest.raises(ValueError, match='spread'):
        losses.lossfuncs_factory(['hmp', 'omp'], 2, [1, 1], 'focal_l2_loss', 'offset_laplace_loss', 'offset_l1_loss',
                                 'scale_l1_loss', False)


def test_new_loss_entry_points_validate_arguments_without_gpu():
    lib = _lib.load()
    x = torch.zeros(64)
    m = torch.zeros(64, dtype=torch.uint8)
    p, mp = _lib.ptr(x), _lib.ptr(m)
    # null pointers
    assert lib.og_l2_loss_f32(None, p, mp, 1, 2, 8, p, p, None) == _lib.OG_EINVAL
    assert b"og_l2_loss_f32: null pointer" in lib.og_last_error()
    assert lib.og_masked_l1_loss_f32(p, p, mp, 1, 2, 8, 0.1, 0, None, p, None) == _lib.OG_EINVAL
    assert b"og_masked_l1_loss_f32: null pointer" in lib.og_last_error()
    assert lib.og_vector_l1_loss_f32(p, p, None, 1, 2, 8, 1e-5, 0, p, p, None) == _lib.OG_EINVAL
    assert b"og_vector_l1_loss_f32: null pointer" in lib.og_last_error()
    assert lib.og_laplace_loss_f32(p, p, p, mp, 1, 2, 8, 1e-5, 0, p, p, None, None) == _lib.OG_EINVAL   # no grad_logb
    assert b"og_laplace_loss_f32: null pointer" in lib.og_last_error()
    # shapes
    assert lib.og_l2_loss_f32(p, p, mp, 0, 2, 8, p, p, None) == _lib.OG_EINVAL and b"bad shape" in lib.og_last_error()
    assert lib.og_masked_l1_loss_f32(p, p, mp, 1, 2, 0, 0.1, 0, p, p, None) == _lib.OG_EINVAL
    assert b"bad shape" in lib.og_last_error()
    assert lib.og_vector_l1_loss_f32(p, p, mp, 1, 3, 8, 1e-5, 0, p, p, None) == _lib.OG_EINVAL          # odd channel count
    assert b"pairs" in lib.og_last_error()
    assert lib.og_laplace_loss_f32(p, p, p, mp, 1, 3, 8, 1e-5, 0, p, p, p, None) == _lib.OG_EINVAL
    assert b"pairs" in lib.og_last_error()
    assert lib.og_laplace_loss_f32(p, p, p, mp, 1, -2, 8, 1e-5, 0, p, p, p, None) == _lib.OG_EINVAL
    assert b"bad shape" in lib.og_last_error()
