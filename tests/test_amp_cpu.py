"""CPU: the restatement of the loss-scaler scale block (tests/amp_common.py) on a written-out trace, its agreement with
optim_common.step_scale at S = 1, train_dist's apex flags, and the amp state through a checkpoint."""
import math

import numpy as np
import pytest
import torch

import amp_common as ac
import optim_common as oc
from offsetguided_amd import models, optim, train_dist

F = np.float32
INF, NAN = math.inf, math.nan

# window 3, factor 2, scales inside [1, 16], start S = 4.  Every n2 is (3 S)^2: an unscaled norm of exactly 3.
# (what happens, n2 as a multiple of S^2 or inf / nan, loss) -> (S', unskipped', overflow, dropped) written out by hand
TRACE = [
    ('clean', 9.0, 1.0, (4, 1, False, False)),
    ('clean', 9.0, 1.0, (4, 2, False, False)),
    ('grow at the window', 9.0, 1.0, (8, 0, False, False)),
    ('clean', 9.0, 1.0, (8, 1, False, False)),
    ('loss-limit drop: S stays, the step counts', 9.0, 2e8, (8, 2, False, True)),
    ('grow', 9.0, 1.0, (16, 0, False, False)),
    ('clean', 9.0, 1.0, (16, 1, False, False)),
    ('clean', 9.0, 1.0, (16, 2, False, False)),
    ('clamp at max_loss_scale', 9.0, 1.0, (16, 0, False, False)),
    ('clean', 9.0, 1.0, (16, 1, False, False)),
    ('inf: halve, unskipped back to 0', INF, 1.0, (8, 0, True, False)),
    ('clean', 9.0, 1.0, (8, 1, False, False)),
    ('nan: halve', NAN, 1.0, (4, 0, True, False)),
    ('inf', INF, 3e8, (2, 0, True, False)),
    ('inf', INF, 1.0, (1, 0, True, False)),
    ('clamp at min_loss_scale', INF, 1.0, (1, 0, True, False)),
    ('clean', 9.0, 1.0, (1, 1, False, False)),
]


@pytest.mark.parametrize("max_norm", [INF, 1.5], ids=['no_clip', 'clip'])
def test_written_out_trace(max_norm):
    S, u = F(4), 0
    for what, mult, loss, (S2, u2, overflow, dropped) in TRACE:
        n2 = mult * float(S) ** 2
        got = ac.amp_step_scale(n2, S, u, scale_factor=2.0, scale_window=3, min_scale=1.0, max_scale=16.0, loss=loss, max_norm=max_norm)
        scale, norm = got[:2]
        assert got[2:] == (F(S2), u2, overflow, dropped), f'{what}: {got}'
        assert got[2].dtype == np.float32 and scale.dtype == np.float32 and norm.dtype == np.float32
        if overflow or dropped:
            assert scale == 0
        else:                       # 1 / S is exact; the clip coefficient is the one of an unscaled norm of 3
            assert norm == 3 and scale == oc.step_scale(9.0, max_norm=max_norm)[0] / S
        if not overflow:
            assert norm == 3
        elif math.isinf(n2):
            assert norm == INF
        else:
            assert math.isnan(norm)
        S, u = got[2], got[3]


def test_static_scale():
    """A static scale never moves; an overflow counts a dropped batch, as a non-finite norm does without a scaler."""
    got = ac.amp_step_scale(INF, 1000.0, 7, dynamic=False, scale_window=3)
    assert got[0] == 0 and got[1] == INF and got[2:] == (F(1000), 7, True, True)
    got = ac.amp_step_scale(9e6, 1000.0, 7, dynamic=False, scale_window=3)
    inv = F(1) / F(1000)
    assert got == (inv, F(3), F(1000), 7, False, False)
    got = ac.amp_step_scale(9e6, 1000.0, 7, dynamic=False, max_norm=1.5)
    c = F(1.5) / (F(3) + F(1e-6))
    assert got[0] == c * inv and c < 1
    got = ac.amp_step_scale(9e6, 1000.0, 7, dynamic=False, loss=2e8)
    assert got == (F(0), F(3), F(1000), 7, False, True)


STEP_SCALE_CASES = [                    # the clip, loss, inf and NaN cases of tests/test_gpu_optim.py's scale block
    (1234.5625, None, 1e8, 1e4), (1234.5625, None, 1e8, 0.75), (1234.5625, 3.0, 1e8, INF), (1234.5625, 0.99e8, 1e8, 0.75),
    (1234.5625, 1.01e8, 1e8, 0.75), (1234.5625, 10.5, 10.0, INF), (INF, 1.0, 1e8, 0.75), (NAN, 1.0, 1e8, INF),
    (0.0, None, 1e8, 0.75), (3.0e-9, None, 1e8, 1.0), (7.0e30, 1.0, 1e8, 2.0),
]


@pytest.mark.parametrize("n2,loss,limit,max_norm", STEP_SCALE_CASES)
def test_unit_static_scale_is_step_scale(n2, loss, limit, max_norm):
    """S = 1 static: bit for bit optim_common.step_scale."""
    scale, norm, dropped = oc.step_scale(n2, loss=loss, loss_limit=limit, max_norm=max_norm)
    got = ac.amp_step_scale(n2, 1.0, 5, dynamic=False, loss=loss, loss_limit=limit, max_norm=max_norm)
    assert np.array_equal(oc.bits(got[0]), oc.bits(scale)) and got[5] == dropped and got[2:4] == (F(1), 5)
    assert got[4] == (not math.isfinite(n2))
    if math.isnan(n2):
        assert math.isnan(got[1]) and math.isnan(norm)
    else:
        assert np.array_equal(oc.bits(got[1]), oc.bits(norm))


# ---- the flags ------------------------------------------------------------------------------------------------------------------
def _error(argv, capsys):
    with pytest.raises(SystemExit):
        train_dist.train_cli(['--no-pretrain'] + argv)
    return capsys.readouterr().err


def test_parser(capsys):
    assert '--device-step' in _error(['--opt-level', 'O1'], capsys)
    assert 'master weights' in _error(['--opt-level', 'O2', '--device-step'], capsys)
    assert 'master weights' in _error(['--opt-level', 'O3', '--device-step'], capsys)
    assert 'O1' in _error(['--loss-scale', '128'], capsys)
    assert 'number' in _error(['--opt-level', 'O1', '--device-step', '--loss-scale', 'big'], capsys)
    cpu = torch.device('cpu')
    args = train_dist.train_cli(['--no-pretrain'])
    assert args.opt_level is None and args.loss_scale is None and args.load_amp is True
    assert train_dist.amp_setup(args, cpu, True) == (torch.bfloat16, None)          # what every run so far did
    assert train_dist.amp_setup(args, cpu, False) == (None, None)
    assert train_dist.amp_setup(train_dist.train_cli(['--no-pretrain', '--device-step']), cpu, True) == (torch.bfloat16, None)
    assert train_dist.amp_setup(train_dist.train_cli(['--no-pretrain', '--opt-level', 'O0']), cpu, True) == (None, None)
    args = train_dist.train_cli(['--no-pretrain', '--device-step', '--opt-level', 'O1', '--drop-amp-state'])
    dtype, scaler = train_dist.amp_setup(args, cpu, True)
    assert dtype == torch.float16 and scaler.dynamic and args.load_amp is False
    assert scaler.state_dict() == {'loss_scale': 65536.0, 'unskipped': 0}
    assert (scaler.scale_factor, scaler.scale_window, scaler.min_loss_scale, scaler.max_loss_scale) == (2.0, 2000, 1.0, 2.0 ** 24)
    for flag in ('dynamic', '128'):
        args = train_dist.train_cli(['--no-pretrain', '--device-step', '--opt-level', 'O1', '--loss-scale', flag])
        _, scaler = train_dist.amp_setup(args, cpu, True)
        assert scaler.dynamic == (flag == 'dynamic') and scaler.state_dict()['loss_scale'] == (65536.0 if scaler.dynamic else 128.0)


def test_scaler_arguments():
    for bad in (dict(scale_factor=1.0), dict(scale_window=0), dict(min_loss_scale=0.0), dict(min_loss_scale=4.0, max_loss_scale=2.0),
                dict(init_scale=NAN), dict(loss_scale=-2.0), dict(loss_scale=INF), dict(scale_factor=NAN)):
        with pytest.raises(ValueError):
            optim.DeviceLossScaler(device='cpu', **bad)
    scaler = optim.DeviceLossScaler(device='cpu')
    with pytest.raises(ValueError):
        scaler.load_state_dict({'loss_scale': 0.0, 'unskipped': 0})
    with pytest.raises(ValueError):
        optim.load_amp_state(scaler, {'loss_scaler1': {}})
    assert optim.load_amp_state(scaler, False) is False and scaler.state_dict() == {'loss_scale': 65536.0, 'unskipped': 0}


# ---- the checkpoint -------------------------------------------------------------------------------------------------------------
def test_amp_state_round_trip(tmp_path):
    """amp_state_dict -> save_model -> load_model(load_amp=True) -> load_amp_state on CPU tensors, and an amp entry written by hand
    in the layout of apex's amp.state_dict()."""
    net = torch.nn.Linear(3, 2)
    scaler = optim.DeviceLossScaler(device='cpu', scale_window=50)
    scaler.load_state_dict({'loss_scale': 4096.0, 'unskipped': 33})
    assert float(scaler.loss_scale) == 4096.0 and int(scaler.unskipped) == 33
    assert int(scaler.overflow_steps) == 0 and int(scaler.last_overflow) == 0
    loss = torch.tensor(0.5, requires_grad=True)
    scaler.scale(loss).backward()
    assert float(loss.grad) == 4096.0
    state = optim.amp_state_dict(scaler)
    assert state == {'loss_scaler0': {'loss_scale': 4096.0, 'unskipped': 33}}
    path = str(tmp_path / 'ck.pth')
    models.save_model(path, 3, 0.5, net, None, amp_state=state)
    *_, loaded = models.load_model(torch.nn.Linear(3, 2), path, drop_layers=False, resume_optimizer=False, load_amp=True)
    assert loaded == state
    fresh = optim.DeviceLossScaler(device='cpu')
    assert optim.load_amp_state(fresh, loaded) is True and fresh.state_dict() == state['loss_scaler0']
    *_, dropped = models.load_model(torch.nn.Linear(3, 2), path, drop_layers=False, resume_optimizer=False, load_amp=False)
    assert dropped is False
    written = {'loss_scaler0': {'loss_scale': 32768.0, 'unskipped': 17}}
    models.save_model(path, 3, 0.5, net, None, amp_state=written)
    *_, loaded = models.load_model(torch.nn.Linear(3, 2), path, drop_layers=False, resume_optimizer=False, load_amp=True)
    optim.load_amp_state(fresh, loaded)
    assert fresh.state_dict() == written['loss_scaler0'] and float(fresh.loss_scale) == 32768.0 and int(fresh.unskipped) == 17


def test_load_checkpoint_resumes_the_scaler(tmp_path):
    """train_dist.load_checkpoint: the amp entry reaches the scaler with --resume, and stays out with --drop-amp-state."""
    net = torch.nn.Linear(3, 2)
    path = str(tmp_path / 'ck.pth')
    models.save_model(path, 3, 0.5, net, None, amp_state={'loss_scaler0': {'loss_scale': 2048.0, 'unskipped': 5}})
    common = ['--no-pretrain', '--device-step', '--opt-level', 'O1', '--resume', '--drop-optim-state', '--checkpoint-whole', path]
    for extra, expect in (([], {'loss_scale': 2048.0, 'unskipped': 5}), (['--drop-amp-state'], {'loss_scale': 65536.0, 'unskipped': 0})):
        args = train_dist.train_cli(common + extra)
        _, scaler = train_dist.amp_setup(args, torch.device('cpu'), False)
        _, _, start_epoch, _ = train_dist.load_checkpoint(args, torch.nn.Linear(3, 2), None, False, scaler)
        assert start_epoch == 4 and scaler.state_dict() == expect
