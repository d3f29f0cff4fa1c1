"""GPU: fp16 training's device-side loss scaler (og_step_scale_amp_f32 in csrc/optim.hip, optim.DeviceLossScaler).  A step on S * g
with a power-of-two S equals the merged scaler-less step on g bit for bit; every word of the scaler block and of the state block
follows the numpy restatement (tests/amp_common.py) through overflows, growth, both clamps, a static scale and a loss-limit drop;
an overflow step is the zero-gradient update; a gradient that underflows in fp16 arrives exactly with the scaler; three fp16 training
steps never wait for the device; a scaler resumed from its state_dict goes on identically."""
import math

import numpy as np
import pytest
import torch

import amp_common as ac
import optim_common as oc
from offsetguided_amd import _lib, optim, train_dist
from offsetguided_amd.optim import DeviceLossScaler
from test_gpu_optim import Twin, _chunk, _eighths

pytestmark = pytest.mark.gpu
INF, NAN = math.inf, math.nan


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    _lib.load()
    return torch.device("cuda:0")


def _specs():
    """1, 5, chunk + 5 and 2 chunk + 5 elements, and a view whose parameter and gradient start 4 bytes off a 16-byte boundary."""
    c = _chunk()
    return [(1, 0, 0), (5, 0, 0), (c + 5, 0, 0), (2 * c + 5, 0, 0), (37, 1, 1)]


def _tensors(tw):
    """Bit patterns of every parameter and moment of a Twin's device optimizer."""
    out = []
    for i in tw.live:
        p = tw.params[i]
        out.append(oc.bits(p.detach().cpu().numpy()))
        for k in tw.opt.MOMENTS:
            if k in tw.opt.state[p]:
                out.append(oc.bits(tw.opt.state[p][k].cpu().numpy()))
    return out


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _block(scaler):
    """(loss_scale fp32, unskipped, overflows, last_overflow) read back."""
    host = scaler._block.cpu()
    return host[0:1].view(torch.float32).numpy()[0], int(host[1]), int(host[2]), int(host[3])


# ---- scaled == unscaled -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [INF, 0.75], ids=['no_clip', 'clip'])
@pytest.mark.parametrize("S", [2.0 ** 8, 2.0 ** 16, 2.0 ** 24])
@pytest.mark.parametrize("kind", ['adamw_wd', 'sgd_mom_wd'])
def test_scaled_equals_unscaled(dev, kind, S, clip):
    """Three steps on S g0 with a scaler against three steps on g0 without one.  S is a power of two: S^2 n2, its root, the division
    by S, 1 / S and c (1 / S) are exact, so the merged scaler-less path pins the new block independently of the new restatement.
    |g0| <= 1e3, so S g0 <= 1.7e10 stays finite in fp32 and its squares in double."""
    plain, scaled = Twin(dev, kind, _specs(), seed=41), Twin(dev, kind, _specs(), seed=41)
    scaler = DeviceLossScaler(init_scale=S, device=dev)
    loss = torch.tensor(2.5, device=dev)
    for step, lr in enumerate([1e-3, 2.5e-4, 7e-3]):
        g0 = plain.random_grads()
        plain.set_grads(g0)
        scaled.set_grads({i: g0[i] * np.float32(S) for i in g0})
        c, _, _ = oc.step_scale(oc.sum_of_squares(g0.values()), max_norm=clip)
        assert (c < 1) == (clip != INF)
        plain.step(lr, scale=c, loss=loss, max_grad_norm=clip)
        scaled.step(lr, scale=c / np.float32(S), loss=loss, max_grad_norm=clip, scaler=scaler)
        assert _same(_tensors(plain), _tensors(scaled)), f'step {step + 1}'
        assert np.array_equal(oc.bits(plain.opt.last_grad_norm.cpu().numpy()), oc.bits(scaled.opt.last_grad_norm.cpu().numpy()))
        assert int(plain.opt.dropped_steps) == int(scaled.opt.dropped_steps) == 0
        assert float(scaled.opt.last_scale) * S == float(plain.opt.last_scale)
    assert _block(scaler) == (np.float32(S), 3, 0, 0)


# ---- the scaler block, every word -------------------------------------------------------------------------------------------------
# an event: (poison (tensor index, element, value) or None, loss or None).  In _block_specs tensor 2 has chunk + 2 elements: its
# last two are the tail of its second chunk; tensor 3's gradient starts 8 bytes off a 16-byte boundary: its first two are a head.
CLEAN, TAIL_INF, HEAD_NAN = (None, 1.0), ((2, -1, INF), 1.0), ((3, 0, NAN), 1.0)
BLOCK_CASES = {
    # name: (scaler arguments, state loaded first or None, max_grad_norm, events)
    'inf_in_a_tail': (dict(scale_window=3), None, INF, [CLEAN, TAIL_INF, CLEAN]),
    'nan_in_a_head': (dict(scale_window=3), None, 0.75, [CLEAN, HEAD_NAN, HEAD_NAN]),
    'growth_after_window': (dict(scale_window=3, init_scale=2.0 ** 10), None, 0.75, [CLEAN, CLEAN, CLEAN, CLEAN]),
    'window_of_two': (dict(scale_window=2, init_scale=2.0 ** 4), None, INF, [CLEAN, CLEAN, TAIL_INF, CLEAN, CLEAN]),
    'clamp_max': (dict(scale_window=2, max_loss_scale=2.0 ** 17), dict(loss_scale=2.0 ** 16, unskipped=1), INF, [CLEAN, CLEAN, CLEAN]),
    'clamp_min': (dict(scale_window=3, init_scale=3.0, min_loss_scale=1.25), None, INF, [TAIL_INF, TAIL_INF, CLEAN]),
    'odd_factor': (dict(scale_window=2, init_scale=1000.0, scale_factor=1.5), None, 0.75, [CLEAN, CLEAN, HEAD_NAN, CLEAN]),
    'static_overflow': (dict(loss_scale=1000.0), None, 0.75, [CLEAN, TAIL_INF, CLEAN]),
    'static_1000': (dict(loss_scale=1000.0), None, INF, [CLEAN, CLEAN]),
    'loss_limit_drop': (dict(scale_window=3), dict(loss_scale=2.0 ** 12, unskipped=1), 0.75, [CLEAN, (None, 2e8), CLEAN]),
    'overflow_and_loss_limit': (dict(scale_window=3), None, INF, [(TAIL_INF[0], 2e8), CLEAN]),
}


def _block_specs():
    return [(3, 0, 0), (1025, 0, 0), (_chunk() + 2, 0, 0), (40, 1, 2)]


def _run_events(tw, scaler, events, clip, S, u, overflows=0, dropped=0, first_lr=1e-3):
    """Each event's step on the device and in the restatement; every word of both blocks and every tensor compared after it."""
    kw = dict(dynamic=scaler.dynamic, scale_factor=scaler.scale_factor, scale_window=scaler.scale_window,
              min_scale=scaler.min_loss_scale, max_scale=scaler.max_loss_scale)
    for n, (poison, loss) in enumerate(events):
        grads = {i: _eighths(tw.rs, tw.specs[i][0]) for i in tw.live}
        if poison is not None:
            grads[poison[0]][poison[1]] = poison[2]
        with np.errstate(invalid='ignore', over='ignore'):
            n2 = oc.sum_of_squares([grads[i] for i in tw.live])
        scale, norm, S, u, overflow, drop = ac.amp_step_scale(n2, S, u, loss=loss, max_norm=clip, **kw)
        overflows += int(overflow and scaler.dynamic)
        dropped += int(drop)
        tw.set_grads(grads)
        tw.step(first_lr * (n + 1), scale=scale, loss=torch.tensor(loss, dtype=torch.float32, device=tw.dev), max_grad_norm=clip,
                scaler=scaler)
        where = f'event {n}'
        got = _block(scaler)
        assert np.array_equal(oc.bits(got[0]), oc.bits(S)) and got[1:] == (u, overflows, int(overflow)), f'{where}: {got}'
        assert np.array_equal(oc.bits(tw.opt.last_scale.cpu().numpy()), oc.bits(scale)), where
        if math.isnan(n2):                                 # (a NaN has many encodings)
            assert math.isnan(float(tw.opt.last_grad_norm)), where
        else:
            assert np.array_equal(oc.bits(tw.opt.last_grad_norm.cpu().numpy()), oc.bits(norm)), where
        assert int(tw.opt.dropped_steps) == dropped, where
        if overflow or drop:
            assert scale == 0
        tw.check(where)                                    # p, m, v: the update with that scale -- for scale 0 a zero gradient's
        assert all(np.isfinite(tw.p[i]).all() for i in tw.live)
    return S, u, overflows, dropped


@pytest.mark.parametrize("kind", ['adamw_wd', 'sgd_mom_wd'])
@pytest.mark.parametrize("case", sorted(BLOCK_CASES))
def test_scaler_block(dev, kind, case):
    """The device's [scale, norm, dropped] and [loss_scale, unskipped, overflows, last_overflow] against amp_common after every
    step, and p, m, v against optim_common with that scale: on an overflow step exactly the update of a zero gradient (adam_step /
    sgd_step with scale=0), no inf or NaN reaching the state."""
    kw, state, clip, events = BLOCK_CASES[case]
    tw = Twin(dev, kind, _block_specs(), seed=43)
    scaler = DeviceLossScaler(device=dev, **kw)
    if state is not None:
        scaler.load_state_dict(state)
    S, u = (state['loss_scale'], state['unskipped']) if state else (kw.get('loss_scale', kw.get('init_scale', 2.0 ** 16)), 0)
    S, u, overflows, dropped = _run_events(tw, scaler, events, clip, np.float32(S), u)
    expect = {'inf_in_a_tail': (2.0 ** 15, 1, 1, 0), 'nan_in_a_head': (2.0 ** 14, 0, 2, 0), 'growth_after_window': (2.0 ** 11, 1, 0, 0),
              'window_of_two': (2.0 ** 5, 0, 1, 0), 'clamp_max': (2.0 ** 17, 0, 0, 0), 'clamp_min': (1.25, 1, 2, 0),
              'odd_factor': (1000.0, 1, 1, 0), 'static_overflow': (1000.0, 0, 0, 1), 'static_1000': (1000.0, 0, 0, 0),
              'loss_limit_drop': (2.0 ** 13, 1, 0, 1), 'overflow_and_loss_limit': (2.0 ** 15, 1, 1, 0)}[case]
    assert (float(S), u, overflows, dropped) == expect              # the restatement went where the case means it to go


def test_unit_static_scale_is_the_scalerless_path(dev):
    """S = 1 static: state block and tensors bit for bit those of step() without a scaler, through a clip, an inf and a loss drop."""
    plain, unit = Twin(dev, 'adamw_wd', _block_specs(), seed=47), Twin(dev, 'adamw_wd', _block_specs(), seed=47)
    scaler = DeviceLossScaler(loss_scale=1.0, device=dev)
    for n, (poison, loss) in enumerate([CLEAN, TAIL_INF, CLEAN, (None, 2e8), HEAD_NAN]):
        grads = {i: _eighths(plain.rs, plain.specs[i][0]) for i in plain.live}
        if poison is not None:
            grads[poison[0]][poison[1]] = poison[2]
        kw = dict(loss=torch.tensor(loss, dtype=torch.float32, device=dev), max_grad_norm=0.75)
        for tw, extra in ((plain, {}), (unit, dict(scaler=scaler))):
            tw.set_grads({i: g.copy() for i, g in grads.items()})
            for group in tw.opt.param_groups:
                group['lr'] = 1e-3
            tw.opt.step(**kw, **extra)
        assert _same(_tensors(plain), _tensors(unit)), f'step {n}'
        a, b = plain.opt._ws[:12].cpu().view(torch.int32).numpy(), unit.opt._ws[:12].cpu().view(torch.int32).numpy()
        if poison is not None and math.isnan(poison[2]):
            assert a[0] == b[0] == 0 and a[2] == b[2] and math.isnan(float(unit.opt.last_grad_norm))
        else:
            assert np.array_equal(a, b), f'step {n}: {a} {b}'
        assert _block(scaler) == (np.float32(1), 0, 0, int(poison is not None))
    assert int(unit.opt.dropped_steps) == 3


# ---- what the scaler is for -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled", [False, True], ids=['scale_1', 'scale_2^16'])
def test_fp16_underflow_is_recovered_exactly(dev, scaled):
    """loss = (w.half() * a.half()).float() * 2^-10 with a = 2^-20: the fp16 backward multiplies 2^-10 by 2^-20 = 2^-30, below fp16's
    smallest subnormal 2^-24, so w.grad is 0 and an SGD step does not move w.  Behind S = 2^16 the product is 2^6 * 2^-20 = 2^-14, a
    normal fp16 number; the step unscales it to 2^-30 exactly and moves w = 2^-12 by lr 2^-30 (representable: the spacing of fp32 at
    2^-12 is 2^-35)."""
    w = torch.nn.Parameter(torch.full((1,), 2.0 ** -12, device=dev))
    a = torch.full((1,), 2.0 ** -20, device=dev)
    opt = optim.DeviceSGD([w], lr=1.0)
    scaler = DeviceLossScaler(device=dev) if scaled else None
    loss = ((w.half() * a.half()).float() * 2.0 ** -10).sum()
    (scaler.scale(loss) if scaled else loss).backward()
    assert float(w.grad) == (2.0 ** -14 if scaled else 0.0)
    opt.step(loss=loss.detach(), **(dict(scaler=scaler) if scaled else {}))
    assert float(w.detach()) == (2.0 ** -12 - 2.0 ** -30 if scaled else 2.0 ** -12)
    assert float(opt.last_grad_norm) == (2.0 ** -30 if scaled else 0.0) and int(opt.dropped_steps) == 0
    if scaled:
        assert _block(scaler) == (np.float32(2.0 ** 16), 1, 0, 0)


class TwoConvsBN(torch.nn.Module):
    """Convolution + BatchNorm, then a convolution per output, in the NetworkWrapper output nesting (tests/test_train_step.py)."""

    def __init__(self):
        super().__init__()
        self.body = torch.nn.Conv2d(3, 8, 3, stride=4, padding=1)
        self.bn = torch.nn.BatchNorm2d(8)
        self.hm = torch.nn.ModuleList([torch.nn.Conv2d(8, 17, 1) for _ in range(2)])
        self.off = torch.nn.ModuleList([torch.nn.Conv2d(8, 38, 1) for _ in range(2)])

    def forward(self, x):
        f = torch.relu(self.bn(self.body(x)))
        return [([h(f) for h in self.hm], [[], []], [[], []]), ([o(f) for o in self.off], [[], []], [[], []])]


@pytest.mark.parametrize("optimizer", ['adam', 'sgd'])
def test_fp16_training_steps_never_wait_for_the_device(dev, optimizer, monkeypatch):
    """Three --device-step --opt-level O1 training steps (fp16 autocast, dynamic loss scaler) under torch's sync debug mode: anything
    that makes the host wait for the GPU raises.  Before them the scaler settles as it would in a run: with the offset loss weighted
    100 the fp16 gradients of this toy overflow at 2^16, every such step is skipped and halves the scale until one is taken (measured:
    eight overflows, the ninth step is taken at 2^8 with an unscaled gradient norm of 1.1e3).  Whatever the three steps meet, the scaler's words add up, a step that was taken moved
    every parameter, and nothing non-finite reached one."""
    from offsetguided_amd.models import losses
    monkeypatch.setattr(torch.backends.cudnn, 'benchmark', False)
    args = train_dist.train_cli(['--no-pretrain', '--device-step', '--opt-level', 'O1', '--max-grad-norm', '10', '--optimizer', optimizer])
    crit = losses.lossfuncs_factory(['hmp', 'omp'], 2, [1, 1], 'focal_l2_loss', 'offset_l1_loss', 'offset_instance_l1_loss',
                                    'scale_l1_loss', True, fused=True)
    torch.manual_seed(0)
    net = TwoConvsBN().to(dev)
    opt = train_dist.make_optimizer(args, net, 1, True)
    autocast_dtype, scaler = train_dist.amp_setup(args, dev, True)
    assert autocast_dtype == torch.float16 and isinstance(scaler, DeviceLossScaler) and scaler.dynamic
    images = torch.randn(2, 3, 64, 64, device=dev)
    annos = train_dist.synthetic_targets(3, 2, 64, dev)
    lambdas = [1, 0, 0, 100, 0.01]
    step = lambda: train_dist.train_step_device(net, crit, opt, images, annos, lambdas, autocast_dtype, args.max_grad_norm,  # noqa: E731
                                                scaler=scaler)
    settle = 0
    while True:                                         # warm-up outside the guarded region, until the scale lets a step through
        first, _ = step()
        settle += 1
        if int(scaler.last_overflow) == 0:
            break
        assert settle <= 16, 'the loss scale reached its minimum and the gradients still overflow'
    torch.cuda.synchronize()
    S0, u0, ov0, _ = _block(scaler)
    assert ov0 == settle - 1 and u0 == 1 and S0 == 2.0 ** (16 - ov0)
    start = [p.detach().clone() for p in net.parameters()]
    before = torch.cuda.get_sync_debug_mode()
    results = []
    try:
        torch.cuda.set_sync_debug_mode('error')
        for _ in range(3):
            results.append(step())
        norm, dropped = opt.last_grad_norm, opt.dropped_steps
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert all(torch.is_tensor(loss) and loss.is_cuda for loss, _ in results)
    assert np.isfinite(float(first)) and np.isfinite(float(results[-1][0])) and int(dropped) == 0
    S, unskipped, overflows, last = _block(scaler)
    print(f'settled after {settle} steps at {S0}; then loss scale {S} unskipped {unskipped} overflows {overflows} last_overflow {last} '
          f'norm {float(norm)}')
    assert ov0 <= overflows <= ov0 + 3 and S == S0 / 2.0 ** (overflows - ov0) and (unskipped == 0) == (last == 1)
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
    if overflows == ov0:
        assert unskipped == u0 + 3
    if last == 0:                                       # the last step was taken: it is inside the guarded region
        assert float(norm) > 0 and all(not torch.equal(a, b.detach()) for a, b in zip(start, net.parameters()))


# ---- checkpoints and errors -------------------------------------------------------------------------------------------------------
def test_resumed_scaler_continues_identically(dev):
    """Two events, state_dict(), a new scaler, load_state_dict(), three more events: scale, window position and every tensor equal
    the uninterrupted run's after each step."""
    events = [CLEAN, TAIL_INF, CLEAN, CLEAN, CLEAN, CLEAN]
    kw = dict(scale_window=3, init_scale=2.0 ** 9)
    whole, resumed = Twin(dev, 'adamw_wd', _block_specs(), seed=53), Twin(dev, 'adamw_wd', _block_specs(), seed=53)
    one, two = DeviceLossScaler(device=dev, **kw), DeviceLossScaler(device=dev, **kw)
    state = _run_events(whole, one, events[:2], 0.75, np.float32(2.0 ** 9), 0)
    state_r = _run_events(resumed, two, events[:2], 0.75, np.float32(2.0 ** 9), 0)
    saved = two.state_dict()
    assert saved == {'loss_scale': 256.0, 'unskipped': 0}
    three = DeviceLossScaler(device=dev, scale_window=3)             # made with the default scale: the state brings its own
    three.load_state_dict(saved)
    state_r = (np.float32(saved['loss_scale']), saved['unskipped'], 0, state_r[3])      # the overflow count is not part of the state
    for n, event in enumerate(events[2:]):
        state = _run_events(whole, one, [event], 0.75, *state)
        state_r = _run_events(resumed, three, [event], 0.75, *state_r)
        assert _block(one)[:2] == _block(three)[:2] and _block(one)[3] == _block(three)[3], f'event {n + 2}'
        assert _same(_tensors(whole), _tensors(resumed)), f'event {n + 2}'
    assert one.state_dict() == three.state_dict() == {'loss_scale': 512.0, 'unskipped': 1}


def test_scaler_on_another_device_raises(dev):
    p = torch.nn.Parameter(torch.ones(4, device=dev))
    p.grad = torch.ones(4, device=dev)
    opt = optim.DeviceAdam([p], lr=1e-3)
    with pytest.raises(_lib.OgError):
        opt.step(scaler=DeviceLossScaler(device='cpu'))
    assert bool((p == 1).all())


def test_entry_point_refuses_bad_arguments(dev):
    lib = _lib.load()
    ws = torch.zeros(lib.og_optim_workspace_bytes(1), dtype=torch.uint8, device=dev)
    block = torch.zeros(8, dtype=torch.int32, device=dev)
    good = dict(scaler=block.data_ptr(), factor=2.0, window=3, lo=1.0, hi=16.0)
    for bad in (dict(scaler=None), dict(scaler=block.data_ptr() + 4), dict(factor=1.0), dict(factor=NAN), dict(window=0), dict(lo=0.0),
                dict(lo=NAN), dict(hi=0.5), dict(hi=NAN)):
        a = dict(good, **bad)
        rc = lib.og_step_scale_amp_f32(1, None, 1e8, INF, a['scaler'], 1, a['factor'], a['window'], a['lo'], a['hi'], _lib.ptr(ws),
                                       ws.numel(), _lib.stream_ptr(dev))
        assert rc == _lib.OG_EINVAL, bad
    torch.cuda.synchronize()
    assert not bool(block.any()) and not bool(ws.any())               # nothing was launched
