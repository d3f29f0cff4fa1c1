"""GPU: the multi-tensor optimizer kernels (csrc/optim.hip) and offsetguided_amd.optim bit for bit against the fp32 numpy restatement
(tests/optim_common.py): p, m, v and g after each of three steps, over tensor lists that reach every path of a chunk (scalar head and
tail, 16-byte vectors, tensors that start off a 16-byte boundary, more than one chunk, more than one block of the table), the sum of
squares, the scale block, gradients that move between steps, a step that never waits for the device, and a torch checkpoint."""
import math

import numpy as np
import pytest
import torch

import optim_common as oc
from offsetguided_amd import _lib, optim, train_dist

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    _lib.load()
    return torch.device("cuda:0")


def _chunk():
    return _lib.load().og_optim_chunk_elems()


def _off16(values, off, dev):
    """A device tensor holding `values` whose first element sits `off` elements (4 bytes each) past a 16-byte boundary."""
    values = np.ascontiguousarray(values, dtype=np.float32)
    base = torch.zeros(values.size + off + 4, dtype=torch.float32, device=dev)
    view = base[off:off + values.size].view(values.shape)
    view.copy_(torch.from_numpy(values))
    assert view.data_ptr() % 16 == 4 * off
    return view


# (numel, parameter offset, gradient offset): offsets in elements from a 16-byte boundary; None = a parameter without a gradient
def _sizes_list():
    c = _chunk()
    specs = [(n, 0, 0) for n in (1, 3, 4, 5, 1023, 1024, 1025)]
    specs += [(37, 1, 0), (1030, 1, 0), None, (1030, 0, 1), (261, 2, 3), (c + 1, 0, 0), (c + 2, 0, 0), (c + 7, 3, 1), (2 * c + 5, 1, 1)]
    return specs


def _small_list():
    rs = np.random.RandomState(7)
    return [(int(n), 0, 0) for n in rs.randint(1, 10, 700)]      # 700 rows: more than one block of the table's prefix


LISTS = {'sizes': _sizes_list, 'small700': _small_list}

KINDS = {
    'adamw_wd': dict(opt='adam', adam_w_mode=True, wd=1e-2),
    'adam_l2_wd': dict(opt='adam', adam_w_mode=False, wd=1e-2),
    'adam_nowd': dict(opt='adam', adam_w_mode=True, wd=0.0),
    'sgd_plain': dict(opt='sgd', mom=0.0, wd=0.0),
    'sgd_wd': dict(opt='sgd', mom=0.0, wd=1e-2),
    'sgd_mom': dict(opt='sgd', mom=0.9, wd=0.0),
    'sgd_mom_wd': dict(opt='sgd', mom=0.9, wd=1e-2),
}
LRS = [1e-3, 2.5e-4, 7e-3]          # the schedule sets lr per step: it travels as a kernel argument


class Twin:
    """A device optimizer over a tensor list and the restatement's copy of the same state."""

    def __init__(self, dev, kind, specs, seed, state=None):
        self.dev, self.kind, self.specs = dev, dict(KINDS[kind]), specs
        rs = self.rs = np.random.RandomState(seed)
        self.live = [i for i, s in enumerate(specs) if s is not None]
        self.p = {i: oc.magnitudes(rs, specs[i][0], 1e-3, 1e1) for i in self.live}
        self.params = [torch.nn.Parameter(_off16(self.p[i], specs[i][1], dev) if s is not None else torch.ones(5, device=dev))
                       for i, s in enumerate(specs)]
        k = self.kind
        if k['opt'] == 'adam':
            self.opt = optim.DeviceAdam(self.params, lr=1.0, weight_decay=k['wd'], adam_w_mode=k['adam_w_mode'])
        else:
            self.opt = optim.DeviceSGD(self.params, lr=1.0, momentum=k['mom'], weight_decay=k['wd'])
        self.m = {i: np.zeros_like(self.p[i]) for i in self.live}
        self.v = {i: np.zeros_like(self.p[i]) for i in self.live}
        self.t = 0
        self.grads = {}

    def set_grads(self, grads, fresh=True):
        """grads: {index: fp32 array}.  fresh: new gradient tensors (their addresses move); else the old ones are overwritten."""
        self.g = grads
        for i in self.live:
            if fresh or i not in self.grads:
                self.grads[i] = _off16(grads[i], self.specs[i][2], self.dev)
                self.params[i].grad = self.grads[i]
            else:
                self.grads[i].copy_(torch.from_numpy(grads[i]))

    def random_grads(self):
        return {i: oc.magnitudes(self.rs, self.specs[i][0]) for i in self.live}

    def step(self, lr, scale=1.0, **kw):
        for group in self.opt.param_groups:
            group['lr'] = lr
        self.opt.step(**kw)
        self.t += 1
        k = self.kind
        for i in self.live:
            if k['opt'] == 'adam':
                self.p[i], self.m[i], self.v[i] = oc.adam_step(self.p[i], self.g[i], self.m[i], self.v[i], lr=lr, wd=k['wd'], t=self.t,
                                                               adam_w_mode=k['adam_w_mode'], scale=scale)
            else:
                self.p[i], self.m[i] = oc.sgd_step(self.p[i], self.g[i], self.m[i] if self.t > 1 else None, lr=lr, mom=k['mom'],
                                                   wd=k['wd'], first=self.t == 1, scale=scale)

    def _device(self, tensors):
        return torch.cat([t.detach().reshape(-1) for t in tensors]).cpu().numpy()

    def _host(self, arrays):
        return np.concatenate([np.asarray(arrays[i], np.float32).reshape(-1) for i in self.live])

    def check(self, where):
        live = [self.params[i] for i in self.live]
        assert np.array_equal(oc.bits(self._device(live)), oc.bits(self._host(self.p))), f'{where}: p'
        assert np.array_equal(oc.bits(self._device([p.grad for p in live])), oc.bits(self._host(self.g))), f'{where}: g'
        state = self.opt.state
        if self.kind['opt'] == 'adam':
            assert np.array_equal(oc.bits(self._device([state[p]['exp_avg'] for p in live])), oc.bits(self._host(self.m))), f'{where}: m'
            assert np.array_equal(oc.bits(self._device([state[p]['exp_avg_sq'] for p in live])), oc.bits(self._host(self.v))), f'{where}: v'
        elif self.kind['mom'] != 0:
            assert np.array_equal(oc.bits(self._device([state[p]['momentum_buffer'] for p in live])), oc.bits(self._host(self.m))), f'{where}: buf'
        else:
            assert all('momentum_buffer' not in state[p] for p in live)
        for i, s in enumerate(self.specs):                       # a parameter without a gradient has no row: untouched, no state
            if s is None:
                assert bool((self.params[i] == 1).all()) and len(state[self.params[i]]) == 0


@pytest.mark.parametrize("guard", [False, True], ids=['update_only', 'scale_path'])
@pytest.mark.parametrize("which", sorted(LISTS))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_three_steps_bit_for_bit(dev, kind, which, guard):
    """Fresh state, lr changed between steps; step 2 overwrites step 1's gradient tensors, step 3 gets new ones.  scale_path: with a
    small loss the sum of squares and the scale block run and the scale is exactly 1, so the same numbers must come out."""
    tw = Twin(dev, kind, LISTS[which](), seed=11)
    kw = dict(loss=torch.tensor(2.5, device=dev)) if guard else {}
    for step, lr in enumerate(LRS):
        tw.set_grads(tw.random_grads(), fresh=step != 1)
        tw.step(lr, **kw)
        tw.check(f'step {step + 1}')
    if guard:
        assert float(tw.opt.last_scale) == 1.0 and int(tw.opt.dropped_steps) == 0


def _torch_state(kind, params, steps=2):
    """A state_dict written by torch.optim on CPU tensors after `steps` steps, and the numpy copy of parameters and moments."""
    k = KINDS[kind]
    tp = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in params]
    if k['opt'] == 'adam':
        opt = torch.optim.Adam(tp, lr=1e-3, weight_decay=0.0)
    else:
        opt = torch.optim.SGD(tp, lr=1e-3, momentum=k['mom'], weight_decay=0.0)
    rs = np.random.RandomState(5)
    for _ in range(steps):
        for p in tp:
            p.grad = torch.from_numpy(oc.magnitudes(rs, p.numel(), 1e-3, 1e1).reshape(p.shape))
        opt.step()
    return opt, tp


@pytest.mark.parametrize("kind", ['adamw_wd', 'adam_l2_wd', 'sgd_mom_wd'])
def test_resumed_from_a_torch_checkpoint(dev, kind, tmp_path):
    """torch.optim.Adam / SGD state through models.save_model / load_model into the device optimizer; three more steps equal the
    restatement continued from that state (Adam's step count goes on from 2)."""
    from offsetguided_amd import models
    specs = [(n, 0, 0) for n in (5, 1025, _chunk() + 3)]
    tw = Twin(dev, kind, specs, seed=13)
    t_opt, tp = _torch_state(kind, [tw.p[i] for i in tw.live])

    class Holder(torch.nn.Module):
        def __init__(self, ps):
            super().__init__()
            self.ps = torch.nn.ParameterList(ps)

    path = str(tmp_path / 'ck.pth')
    models.save_model(path, 1, 0.25, Holder(tp), t_opt)
    holder = Holder(tw.params)
    _, opt, start_epoch, _, _ = models.load_model(holder, path, optimizer=tw.opt, resume_optimizer=True, drop_layers=False)
    assert opt is tw.opt and start_epoch == 2
    for group in tw.opt.param_groups:                 # the hyper-parameters came from the file: set this case's again
        group['weight_decay'] = KINDS[kind]['wd']
        if KINDS[kind]['opt'] == 'sgd':
            group['momentum'] = KINDS[kind]['mom']
    for n, i in enumerate(tw.live):
        tw.p[i] = tp[n].detach().numpy().copy()
        st = t_opt.state[tp[n]]
        if KINDS[kind]['opt'] == 'adam':
            tw.m[i], tw.v[i] = st['exp_avg'].numpy().copy(), st['exp_avg_sq'].numpy().copy()
        else:
            tw.m[i] = st['momentum_buffer'].numpy().copy()
    tw.t = 2
    for step, lr in enumerate(LRS):
        tw.set_grads(tw.random_grads())
        tw.step(lr)
        tw.check(f'resumed step {step + 1}')
    if KINDS[kind]['opt'] == 'adam':
        assert all(float(st['step']) == 5.0 for st in tw.opt.state_dict()['state'].values())


@pytest.mark.parametrize("kind", ['adamw_wd', 'adam_nowd'])
def test_all_zero_gradient_and_moments(dev, kind):
    """g = 0, m = 0, v = 0: den = eps, u = 0 / eps = 0; only the decoupled decay moves p."""
    tw = Twin(dev, kind, [(n, 0, 0) for n in (1, 6, 1025)], seed=17)
    tw.set_grads({i: np.zeros(tw.specs[i][0], np.float32) for i in tw.live})
    before = {i: tw.p[i].copy() for i in tw.live}
    tw.step(1e-3)
    tw.check('zero step')
    if KINDS[kind]['wd'] == 0:
        assert all(np.array_equal(tw.p[i], before[i]) for i in tw.live)


# ---- sum of squares -------------------------------------------------------------------------------------------------------------
def _sumsq(dev, grads, offsets):
    """og_grad_sumsq_f32 + og_step_scale_f32 on a hand-built table -> (partials float64, norm fp32)."""
    lib, chunk = _lib.load(), _chunk()
    tensors = [_off16(g, off, dev) for g, off in zip(grads, offsets)]
    rows = np.array([[0, t.data_ptr(), 0, 0, t.numel()] for t in tensors], np.int64)
    prefix = np.zeros(len(tensors) + 1, np.int32)
    np.cumsum(-(-rows[:, 4] // chunk), out=prefix[1:])
    n_chunks = int(prefix[-1])
    d_rows, d_prefix = torch.from_numpy(rows).to(dev), torch.from_numpy(prefix).to(dev)
    nbytes = lib.og_optim_workspace_bytes(n_chunks)
    assert nbytes == 16 + 8 * n_chunks
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    stream = _lib.stream_ptr(dev)
    _lib.check(lib.og_grad_sumsq_f32(_lib.ptr(d_rows), _lib.ptr(d_prefix), len(tensors), n_chunks, _lib.ptr(ws), nbytes, stream), lib)
    _lib.check(lib.og_step_scale_f32(n_chunks, None, 1e8, math.inf, _lib.ptr(ws), nbytes, stream), lib)
    host = ws.cpu()
    with pytest.raises(_lib.OgError):
        _lib.check(lib.og_grad_sumsq_f32(_lib.ptr(d_rows), _lib.ptr(d_prefix), len(tensors), n_chunks, _lib.ptr(ws), nbytes - 8, stream), lib)
    return host[16:].view(torch.float64).numpy(), host[:8].view(torch.float32).numpy()[1], host[:4].view(torch.float32).numpy()[0]


def _split(values, chunk):
    cuts = np.cumsum([1, 5, chunk + 3, 2 * chunk, 1023])
    return np.split(values, cuts), [0, 1, 3, 2, 0, 1]


def test_sum_of_squares_exact_on_integers(dev):
    """Integer gradients, |g| <= 64, 100 000 elements: every partial sum is an integer below 2^53, exact in double, so the order of
    the additions cannot matter and the result is THE value."""
    rs = np.random.RandomState(19)
    values = rs.randint(-64, 65, 100000).astype(np.float32)
    grads, offsets = _split(values, _chunk())
    partials, norm, scale = _sumsq(dev, grads, offsets)
    n2 = int((values.astype(np.int64) ** 2).sum())
    assert len(partials) == sum(-(-len(g) // _chunk()) for g in grads)
    assert all(float(x).is_integer() for x in partials) and int(sum(int(x) for x in partials)) == n2
    assert norm == np.float32(np.sqrt(np.float64(n2))) and scale == 1.0


def test_sum_of_squares_random(dev):
    """Random gradients: within n 2^-53 relative of math.fsum, the worst-case bound of any summation order of non-negative terms.
    The fp32 norm is the square root of a number that close to the exact one: the exactly rounded norm or its neighbour."""
    rs = np.random.RandomState(23)
    values = oc.magnitudes(rs, 100000)
    grads, offsets = _split(values, _chunk())
    partials, norm, _ = _sumsq(dev, grads, offsets)
    exact = oc.sum_of_squares(grads)
    bound = len(values) * 2.0 ** -53
    assert abs(math.fsum(partials) - exact) <= bound * exact
    at = 0
    for g in grads:                                    # and chunk by chunk, in table order
        for lo in range(0, len(g), _chunk()):
            part = oc.sum_of_squares([g[lo:lo + _chunk()]])
            assert abs(partials[at] - part) <= bound * part
            at += 1
    ref = np.float32(np.sqrt(exact))
    assert abs(float(norm) - float(ref)) <= float(np.spacing(ref))


# ---- the scale block ------------------------------------------------------------------------------------------------------------
def _eighths(rs, n):
    """Multiples of 1/8 up to 8 in magnitude: squares and their sums are exact in double, so the norm is one known fp32 number."""
    return (rs.randint(-64, 65, n) / 8.0).astype(np.float32)


SCALE_CASES = {
    # name: (step keywords without the loss, loss or None, poison)
    'clip_above_norm': (dict(max_grad_norm=1e4), None, None),
    'clip_below_norm': (dict(max_grad_norm=0.75), None, None),
    'no_clip_with_loss': (dict(max_grad_norm=math.inf), 3.0, None),
    'loss_just_under_limit': (dict(max_grad_norm=0.75), 0.99e8, None),
    'loss_just_over_limit': (dict(max_grad_norm=0.75), 1.01e8, None),
    'custom_limit_over': (dict(loss_limit=10.0), 10.5, None),
    'inf_gradient': (dict(max_grad_norm=0.75), 1.0, np.inf),
    'nan_gradient': (dict(), 1.0, np.nan),
}


@pytest.mark.parametrize("kind", ['adamw_wd', 'sgd_mom_wd'])
@pytest.mark.parametrize("case", sorted(SCALE_CASES))
def test_scale_block(dev, kind, case):
    """One ordinary step, then the case's step: scale, norm and the dropped count are the restatement's, and every parameter and
    moment takes exactly the update with that scale -- for a dropped batch the ge = 0 update, with no NaN reaching p."""
    kw, loss, poison = SCALE_CASES[case]
    specs = [(n, 0, 0) for n in (3, 1025, _chunk() + 2)] + [(40, 1, 2)]
    tw = Twin(dev, kind, specs, seed=29)
    tw.set_grads({i: _eighths(tw.rs, specs[i][0]) for i in tw.live})
    tw.step(1e-3, max_grad_norm=1e6)
    tw.check('first step')
    assert int(tw.opt.dropped_steps) == 0
    grads = {i: _eighths(tw.rs, specs[i][0]) for i in tw.live}
    if poison is not None:
        grads[1][777] = poison
    with np.errstate(invalid='ignore', over='ignore'):
        n2 = oc.sum_of_squares([grads[i] for i in tw.live])
    scale, norm, dropped = oc.step_scale(n2, loss=loss, loss_limit=kw.get('loss_limit', 1e8), max_norm=kw.get('max_grad_norm', math.inf))
    assert dropped == (case in ('loss_just_over_limit', 'custom_limit_over', 'inf_gradient', 'nan_gradient'))
    assert (scale < 1) == (dropped or case in ('clip_below_norm', 'loss_just_under_limit'))
    tw.set_grads(grads)
    if loss is not None:
        kw = dict(kw, loss=torch.tensor(loss, dtype=torch.float32, device=dev))
    tw.step(2e-3, scale=scale, **kw)
    assert np.array_equal(oc.bits(tw.opt.last_scale.cpu().numpy()), oc.bits(scale))
    if math.isnan(n2):                                 # (a NaN has many encodings)
        assert math.isnan(float(tw.opt.last_grad_norm))
    else:
        assert np.array_equal(oc.bits(tw.opt.last_grad_norm.cpu().numpy()), oc.bits(norm))
    assert int(tw.opt.dropped_steps) == int(dropped)
    tw.check(case)
    assert all(np.isfinite(tw.p[i]).all() for i in tw.live)
    assert bool(torch.isfinite(torch.cat([tw.params[i].detach().reshape(-1) for i in tw.live])).all())
    if dropped:                                        # and the count goes on
        tw.step(2e-3, scale=scale, **kw)
        tw.check(case + ', again')
        assert int(tw.opt.dropped_steps) == 2


# ---- gradients that move, steps that never wait ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ['adamw_wd', 'sgd_mom'])
def test_gradients_move_between_steps(dev, kind):
    """step, zero_grad(set_to_none=True), a new backward (autograd allocates new gradients, behind an allocation that takes their old
    place), step: the table follows the pointers."""
    specs = [(n, 0, 0) for n in (5, 1030, _chunk() + 9)]
    tw = Twin(dev, kind, specs, seed=31)
    keep = []
    for step, lr in enumerate(LRS[:2]):
        weights = [torch.from_numpy(oc.magnitudes(tw.rs, s[0], 1e-3, 1e1)).to(dev) for s in specs]
        sum((p * w).sum() for p, w in zip(tw.params, weights)).backward()
        tw.g = {i: tw.params[i].grad.cpu().numpy() for i in tw.live}
        tw.step(lr, max_grad_norm=1e9)
        tw.check(f'step {step + 1}')
        tw.opt.zero_grad(set_to_none=True)
        assert all(p.grad is None for p in tw.params)
        keep.append([torch.empty(s[0], device=dev) for s in specs])      # held to the end: the next gradients land elsewhere


class TwoConvs(torch.nn.Module):
    """Two convolutions per output in the NetworkWrapper output nesting (tests/test_train_step.py)."""

    def __init__(self):
        super().__init__()
        self.body = torch.nn.Conv2d(3, 8, 3, stride=4, padding=1)
        self.hm = torch.nn.ModuleList([torch.nn.Conv2d(8, 17, 1) for _ in range(2)])
        self.off = torch.nn.ModuleList([torch.nn.Conv2d(8, 38, 1) for _ in range(2)])

    def forward(self, x):
        f = torch.relu(self.body(x))
        return [([h(f) for h in self.hm], [[], []], [[], []]), ([o(f) for o in self.off], [[], []], [[], []])]


@pytest.mark.parametrize("optimizer", ['adam', 'sgd'])
def test_device_step_never_waits_for_the_device(dev, optimizer, monkeypatch):
    """Three --device-step training steps with the fused criterion under torch's sync debug mode: anything that makes the host wait
    for the GPU (.item(), float(), a blocking copy) raises."""
    from offsetguided_amd.models import losses
    monkeypatch.setattr(torch.backends.cudnn, 'benchmark', False)     # train_dist.main leaves it on: no exhaustive search for two convs
    args = train_dist.train_cli(['--no-pretrain', '--device-step', '--max-grad-norm', '10', '--optimizer', optimizer])
    crit = losses.lossfuncs_factory(['hmp', 'omp'], 2, [1, 1], 'focal_l2_loss', 'offset_l1_loss', 'offset_instance_l1_loss',
                                    'scale_l1_loss', True, fused=True)
    torch.manual_seed(0)
    net = TwoConvs().to(dev)
    opt = train_dist.make_optimizer(args, net, 1, True)
    assert isinstance(opt, optim.DeviceAdam if optimizer == 'adam' else optim.DeviceSGD)
    images = torch.randn(2, 3, 64, 64, device=dev)
    annos = train_dist.synthetic_targets(3, 2, 64, dev)
    lambdas = [1, 0, 0, 100, 0.01]
    step = lambda: train_dist.train_step_device(net, crit, opt, images, annos, lambdas, None, args.max_grad_norm)  # noqa: E731
    first, _ = step()                                   # allocator, pinned table slot and library warm-up outside the guarded region
    torch.cuda.synchronize()
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
    assert all(torch.is_tensor(part) and part.is_cuda for _, parts in results for part in parts if torch.is_tensor(part))
    assert len(results[0][1]) == 5 and np.isfinite(float(results[-1][0])) and float(norm) > 0 and int(dropped) == 0
    assert np.isfinite(float(first))
    assert all(not torch.equal(a, b.detach()) for a, b in zip(start, net.parameters()))


def test_cpu_tensors_raise(dev):
    p = torch.nn.Parameter(torch.ones(4))
    p.grad = torch.ones(4)
    with pytest.raises(_lib.OgError):
        optim.DeviceAdam([p], lr=1e-3).step()
