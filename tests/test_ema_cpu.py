"""CPU: the weight average's restatement (tests/ema_common.py) against torch.lerp in float64, the decay schedule, the flags of
train_dist and evaluate, the checkpoint entry, and optim.ModelEma on a CPU module (everything but an update works)."""
import numpy as np
import pytest
import torch

import ema_common as ec
import optim_common as oc
from offsetguided_amd import _lib, evaluate, models, optim, train_dist


def test_restatement_against_float64_lerp():
    """Three roundings: d = (x - e)(1 + a), t = omd d (1 + b), e' = (e + t)(1 + c), each of |a|, |b|, |c| <= 2^-24.  With omd <= 1 and
    |x - e| <= 2 M, M = max(|e|, |x|): |t| errs by at most 2 M (2 * 2^-24) (second order dropped: below 2^-47 M), and |e + t| <= M up
    to that error, so the last rounding adds at most 2^-24 M: 5 * 2^-24 M in all, below the 2^-21 M = 8 * 2^-24 M asserted.  The
    weight is the fp32-rounded omd in both, as the host rounds it once.  No intermediate is subnormal at these magnitudes."""
    rs = np.random.RandomState(41)
    e, x = oc.magnitudes(rs, 10000, 1e-6, 1e3), oc.magnitudes(rs, 10000, 1e-6, 1e3)
    x[::7] = e[::7] * np.float32(1.0001)              # neighbours too: the difference cancels
    for omd in (np.float32(1.0 - 0.9998), np.float32(0.9), np.float32(1.0), np.float32(0.0), np.float32(1e-7)):
        got = ec.ema_step(e, x, omd)
        assert got.dtype == np.float32
        ref = torch.lerp(torch.from_numpy(e.astype(np.float64)), torch.from_numpy(x.astype(np.float64)), float(omd)).numpy()
        bound = 2.0 ** -21 * np.maximum(np.abs(e), np.abs(x)).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - ref) <= bound).all()
    assert np.array_equal(oc.bits(ec.ema_step(e, x, np.float32(0.0))), oc.bits(e))


def _tiny():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4))


@pytest.mark.parametrize('t, expected', [(0, 0.1), (1, 2.0 / 11.0), (9, 10.0 / 19.0), (10 ** 6, 0.9998)])
def test_decay_at(t, expected):
    ema = optim.ModelEma(_tiny(), decay=0.9998, warmup=True)
    assert ema.decay_at(t) == expected == ec.decay_at(0.9998, True, t)
    assert optim.ModelEma(_tiny(), decay=0.9998, warmup=False).decay_at(t) == 0.9998 == ec.decay_at(0.9998, False, t)
    with pytest.raises(ValueError):
        optim.ModelEma(_tiny(), decay=1.0)


def _error(cli, argv, capsys):
    with pytest.raises(SystemExit):
        cli(argv)
    return capsys.readouterr().err


def test_parser_errors(capsys):
    assert '--device-step' in _error(train_dist.train_cli, ['--no-pretrain', '--ema-decay', '0.999'], capsys)
    assert '[0, 1)' in _error(train_dist.train_cli, ['--no-pretrain', '--device-step', '--ema-decay', '1'], capsys)
    assert '[0, 1)' in _error(train_dist.train_cli, ['--no-pretrain', '--device-step', '--ema-decay', '-0.1'], capsys)
    assert '--resume' in _error(evaluate.evaluate_cli, ['--no-pretrain', '--use-ema'], capsys)
    args = train_dist.train_cli(['--no-pretrain', '--device-step', '--ema-decay', '0.5', '--ema-warmup', 'False'])
    assert args.ema_decay == 0.5 and args.ema_warmup is False
    args = train_dist.train_cli(['--no-pretrain', '--device-step', '--ema-decay', '0'])
    assert args.ema_decay == 0.0 and args.ema_warmup is True
    args = train_dist.train_cli(['--no-pretrain'])
    assert args.ema_decay is None and train_dist.make_ema(args, _tiny()) is None


def test_shadow_module():
    net = _tiny().to(memory_format=torch.channels_last)
    net.train()
    ema = optim.ModelEma(net, decay=0.99)
    assert ema.module is not net and not ema.module.training and ema.updates == 0
    assert all(not p.requires_grad for p in ema.module.parameters()) and all(p.requires_grad for p in net.parameters())
    w, sw = net[0].weight, ema.module[0].weight
    assert sw.stride() == w.stride() and not sw.is_contiguous() and sw.data_ptr() != w.data_ptr()
    assert list(ema.tensors) == list(net.state_dict())
    for name, (x, e) in ema.tensors.items():
        assert torch.equal(x, e) and ema.shadow_of(x) is e, name
    assert ema.shadow_of(torch.zeros(1)) is None


def test_state_dict_round_trip_and_cpu_update_raises():
    net = _tiny()
    ema = optim.ModelEma(net, decay=0.9)
    with torch.no_grad():
        for p in ema.module.parameters():
            p.add_(1.0)
    ema.updates = 7
    state = ema.state_dict()
    assert set(state) == {'module', 'updates'} and state['updates'] == 7
    other = optim.ModelEma(_tiny(), decay=0.9)
    other.load_state_dict(state)
    assert other.updates == 7
    for (k, a), (_, b) in zip(ema.module.state_dict().items(), other.module.state_dict().items()):
        assert torch.equal(a, b), k
    with pytest.raises(_lib.OgError):
        ema.update()
    assert ema.updates == 7
    p = [q for q in net.parameters()]
    for q in p:
        q.grad = torch.ones_like(q)
    with pytest.raises(_lib.OgError):
        optim.DeviceAdam(p, lr=1e-3).step(ema=ema)


def test_checkpoint_carries_the_average(tmp_path):
    net = _tiny()
    ema = optim.ModelEma(net, decay=0.9)
    with torch.no_grad():
        for p in ema.module.parameters():
            p.mul_(0.5)
        ema.module[1].running_mean.fill_(0.25)
    ema.updates = 3
    path = str(tmp_path / 'ema.pth')
    models.save_model(path, 4, 0.5, net, ema_state=ema.state_dict())
    ckpt = torch.load(path, map_location='cpu')
    assert set(ckpt) == {'epoch', 'train_loss', 'model_state_dict', 'ema_state_dict'} and ckpt['ema_state_dict']['updates'] == 3
    raw, _, start_epoch, _, _ = models.load_model(_tiny().requires_grad_(False), path, drop_layers=False)
    avg, *_ = models.load_model(_tiny().requires_grad_(False), path, drop_layers=False, use_ema=True)
    assert start_epoch == 5
    assert torch.equal(raw[0].weight, net[0].weight) and torch.equal(avg[0].weight, ema.module[0].weight)
    assert not torch.equal(avg[0].weight, raw[0].weight)
    assert float(avg[1].running_mean[0]) == 0.25 and float(raw[1].running_mean[0]) == 0.0
    # an average resumes from the file; a file without one starts it at the loaded weights
    resumed = optim.ModelEma(_tiny(), decay=0.9)
    fresh_net = _tiny()
    resumed.bind(fresh_net)
    models.load_model(fresh_net, path, drop_layers=False, ema=resumed)
    assert resumed.updates == 3 and torch.equal(resumed.module[0].weight, ema.module[0].weight)
    plain = str(tmp_path / 'plain.pth')
    models.save_model(plain, 4, 0.5, net)                       # the old signature
    assert 'ema_state_dict' not in torch.load(plain, map_location='cpu')
    models.load_model(fresh_net, plain, drop_layers=False, ema=resumed)
    assert resumed.updates == 0 and torch.equal(resumed.module[0].weight, net[0].weight)


def test_checkpoint_without_the_average_raises(tmp_path):
    net = _tiny()
    path = str(tmp_path / 'hand_made.pth')
    torch.save({'epoch': 0, 'train_loss': 1.0, 'model_state_dict': net.state_dict()}, path)
    with pytest.raises(KeyError, match='hand_made.pth'):
        models.load_model(_tiny(), path, drop_layers=False, use_ema=True)
    model, optimizer, start_epoch, start_loss, amp = models.load_model(_tiny(), path, drop_layers=False)      # as every caller so far
    assert optimizer is None and start_epoch == 1 and start_loss == 1.0 and amp is False
