"""GPU: the weight average (include/og_decoder.h, "weight average"; csrc/optim.hip; optim.ModelEma) bit for bit against the numpy
restatement (tests/ema_common.py over tests/optim_common.py): the fused update entry points and og_ema_lerp_f32 through the C ABI on
hand-built tables -- every length round a chunk, p and e independently off a 16-byte boundary, a row without an average, NaN guards
round every average -- their error cases, ModelEma with DeviceAdam.step(ema=) on a small channels-last module without a host wait,
the loss scaler beside it, and an engine refreshed from the shadow module."""
import copy
import math

import numpy as np
import pytest
import torch

import ema_common as ec
import engine_refresh_common as rc
import optim_common as oc
from offsetguided_amd import _lib, models, optim
from offsetguided_amd.models import engine as eng_mod

pytestmark = pytest.mark.gpu

GUARD = 0x7fc0dead            # a NaN bit pattern: an average that read it would be poisoned, one that wrote it would change it
LRS = [1e-3, 2.5e-4, 7e-3]
OMDS = [0.9, 1.0 - 0.9998, 0.37]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests selected but no HIP device is visible')
    _lib.load()
    return torch.device('cuda:0')


def _chunk():
    return _lib.load().og_optim_chunk_elems()


class Placed:
    """Tensors of given lengths, each `off` elements past a 16-byte boundary inside a buffer of its own filled with GUARD."""

    def __init__(self, dev, arrays, offs):
        self.bases, self.views, masks = [], [], []
        for a, off in zip(arrays, offs):
            base = torch.full((a.size + off + 8,), GUARD, dtype=torch.int32, device=dev)
            view = base[4 + off:4 + off + a.size].view(torch.float32)
            view.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
            assert view.data_ptr() % 16 == 4 * off
            mask = np.ones(base.numel(), bool)
            mask[4 + off:4 + off + a.size] = False
            self.bases.append(base)
            self.views.append(view)
            masks.append(mask)
        self.mask = torch.from_numpy(np.concatenate(masks)).to(dev)

    def ptrs(self):
        return [v.data_ptr() for v in self.views]

    def values(self):
        return torch.cat(self.views).cpu().numpy()

    def guards_intact(self):
        return bool((torch.cat(self.bases)[self.mask] == GUARD).all())


def _sizes():
    c = _chunk()
    return [1, 3, 4, 5, c - 1, c, c + 1, 2 * c + 5]


def _grid_specs():
    """(numel, p offset, e offset, has an average): every length with p and e independently 0, 4, 8, 12 bytes off, and one row more
    whose average is withheld."""
    specs = [(n, po, eo, True) for n in _sizes() for po in range(4) for eo in range(4)]
    return specs[:40] + [(_chunk() + 7, 1, 2, False)] + specs[40:]


def _tiny_specs():
    rs = np.random.RandomState(7)
    return [(int(n), int(po), int(eo), True) for n, po, eo in zip(rs.randint(1, 10, 700), rs.randint(0, 4, 700), rs.randint(0, 4, 700))]


def _table(dev, rows, counts, extra=None):
    """Device bytes of rows (+ extra int64 words) + prefix -> (tensor, rows ptr, extra ptr, prefix ptr, n_chunks)."""
    rows = np.ascontiguousarray(rows, np.int64)
    prefix = np.zeros(rows.shape[0] + 1, np.int32)
    np.cumsum(counts, out=prefix[1:])
    parts = [rows.reshape(-1).view(np.uint8)] + ([np.asarray(extra, np.int64).view(np.uint8)] if extra is not None else [])
    at_extra = rows.size * 8
    at_prefix = sum(p.size for p in parts)
    raw = torch.from_numpy(np.concatenate(parts + [prefix.view(np.uint8)])).to(dev)
    return raw, raw.data_ptr(), raw.data_ptr() + at_extra, raw.data_ptr() + at_prefix, int(prefix[-1])


KINDS = {
    'adamw_wd': dict(opt='adam', adam_w_mode=True, wd=1e-2),
    'adam_l2_wd': dict(opt='adam', adam_w_mode=False, wd=1e-2),
    'sgd_plain': dict(opt='sgd', mom=0.0, wd=1e-2),
    'sgd_mom': dict(opt='sgd', mom=0.9, wd=0.0),
}


class Fused:
    """One table of tensors for the update entry points and the flat restatement of it (the rules are per element: the tensors'
    values are kept concatenated).  `plain` is a second copy of p, m, v that takes the existing entry point on the same inputs."""

    def __init__(self, dev, kind, specs, seed):
        self.dev, self.k, self.specs = dev, KINDS[kind], specs
        rs = self.rs = np.random.RandomState(seed)
        ns = [s[0] for s in specs]
        self.cuts = np.cumsum(ns)[:-1]
        total = sum(ns)
        self.p, self.e = oc.magnitudes(rs, total, 1e-3, 1e1), oc.magnitudes(rs, total, 1e-3, 1e1)
        self.m, self.v = np.zeros(total, np.float32), np.zeros(total, np.float32)
        self.has = np.concatenate([np.full(s[0], s[3]) for s in specs])
        split = lambda a: np.split(a, self.cuts)                                  # noqa: E731
        po, eo = [s[1] for s in specs], [s[2] for s in specs]
        self.dp, self.de = Placed(dev, split(self.p), po), Placed(dev, split(self.e), eo)
        self.dm = Placed(dev, split(self.m), [(o + 2) % 4 for o in po])
        self.dv = Placed(dev, split(self.v), [(o + 3) % 4 for o in eo])
        self.plain = [Placed(dev, split(a), offs) for a, offs in ((self.p, po), (self.m, [0] * len(po)), (self.v, [1] * len(po)))]
        self.go = [(o + 1) % 4 for o in po]
        self.t = 0

    def _tables(self, dg):
        chunk = _chunk()
        counts = [-(-s[0] // chunk) for s in self.specs]
        ns = [s[0] for s in self.specs]
        ema = [e if s[3] else 0 for e, s in zip(self.de.ptrs(), self.specs)]
        fused = _table(self.dev, list(zip(self.dp.ptrs(), dg.ptrs(), self.dm.ptrs(), self.dv.ptrs(), ns)), counts, ema)
        plain = _table(self.dev, list(zip(self.plain[0].ptrs(), dg.ptrs(), self.plain[1].ptrs(), self.plain[2].ptrs(), ns)), counts)
        return fused, plain

    def step(self, lr, omd, scale=None, grads=None):
        """One call of the _ema entry point and one of the existing one; scale: None = no state block, else its first word."""
        lib, k, n_rows = _lib.load(), self.k, len(self.specs)
        self.t += 1
        g = oc.magnitudes(self.rs, self.p.size) if grads is None else grads
        dg = Placed(self.dev, np.split(g, self.cuts), self.go)
        (keep_f, rows, ema, prefix, n_chunks), (keep_p, prows, _, pprefix, _) = self._tables(dg)
        state = None
        if scale is not None:
            block = torch.tensor([scale, 0, 0, 0], dtype=torch.float32, device=self.dev)
            state = _lib.ptr(block)
        stream = _lib.stream_ptr(self.dev)
        if k['opt'] == 'adam':
            b1, b2 = 0.9, 0.999
            common = (lr, b1, b2, 1.0 - b1, 1.0 - b2, 1e-8, k['wd'], 1.0 - b1 ** self.t, 1.0 - b2 ** self.t, int(k['adam_w_mode']))
            _lib.check(lib.og_adam_step_ema_f32(rows, prefix, n_rows, 0, n_chunks, state, *common, ema, omd, stream), lib)
            _lib.check(lib.og_adam_step_f32(prows, pprefix, n_rows, 0, n_chunks, state, *common, stream), lib)
            p2, self.m, self.v = oc.adam_step(self.p, g, self.m, self.v, lr=lr, wd=k['wd'], t=self.t, adam_w_mode=k['adam_w_mode'],
                                              scale=1.0 if scale is None else scale)
        else:
            common = (lr, k['mom'], k['wd'], int(self.t == 1))
            _lib.check(lib.og_sgd_step_ema_f32(rows, prefix, n_rows, 0, n_chunks, state, *common, ema, omd, stream), lib)
            _lib.check(lib.og_sgd_step_f32(prows, pprefix, n_rows, 0, n_chunks, state, *common, stream), lib)
            p2, buf = oc.sgd_step(self.p, g, self.m if self.t > 1 else None, lr=lr, mom=k['mom'], wd=k['wd'], first=self.t == 1,
                                  scale=1.0 if scale is None else scale)
            self.m = buf if buf is not None else self.m
        torch.cuda.synchronize(self.dev)
        self.p = p2
        self.e = np.where(self.has, ec.ema_step(self.e, p2, np.float32(omd)), self.e)
        self.g, self.dg = g, dg

    def check(self, where):
        assert np.array_equal(oc.bits(self.dp.values()), oc.bits(self.p)), f'{where}: p'
        assert np.array_equal(oc.bits(self.de.values()), oc.bits(self.e)), f'{where}: e'
        assert np.array_equal(oc.bits(self.dg.values()), oc.bits(self.g)), f'{where}: g'
        moments = [(self.dm, self.plain[1], self.m, 'm')] if self.k['opt'] == 'adam' or self.k['mom'] != 0 else []
        moments += [(self.dv, self.plain[2], self.v, 'v')] if self.k['opt'] == 'adam' else []
        for mine, theirs, host, name in moments:
            assert np.array_equal(oc.bits(mine.values()), oc.bits(host)), f'{where}: {name}'
            assert np.array_equal(oc.bits(theirs.values()), oc.bits(host)), f'{where}: {name} of the existing entry point'
        assert np.array_equal(oc.bits(self.plain[0].values()), oc.bits(self.p)), f'{where}: p of the existing entry point'
        for placed in (self.dp, self.de, self.dm, self.dv, self.dg, *self.plain):
            assert placed.guards_intact(), f'{where}: a guard element changed'


# ---- the fused entry points -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', sorted(KINDS))
def test_fused_three_steps_bit_for_bit(dev, kind):
    """Every length x p offset x e offset in ONE table, and the row whose average is withheld: p, m, v equal the restatement AND the
    existing entry point's; e the three-line rule of the p' just stored; the withheld average and every guard element unchanged."""
    tw = Fused(dev, kind, _grid_specs(), seed=43)
    withheld = [i for i, s in enumerate(tw.specs) if not s[3]]
    assert len(withheld) == 1
    before = tw.de.views[withheld[0]].clone()
    for step, (lr, omd) in enumerate(zip(LRS, OMDS)):
        tw.step(lr, omd)
        tw.check(f'step {step + 1}')
    assert torch.equal(tw.de.views[withheld[0]].view(torch.int32), before.view(torch.int32))


def test_fused_700_tiny_tensors(dev):
    tw = Fused(dev, 'adamw_wd', _tiny_specs(), seed=47)
    for step, (lr, omd) in enumerate(zip(LRS, OMDS)):
        tw.step(lr, omd)
        tw.check(f'step {step + 1}')


@pytest.mark.parametrize('kind', ['adamw_wd', 'sgd_mom'])
def test_fused_omd_ends_and_dropped_step(dev, kind):
    """omd = 0 leaves e as it is; omd = 1 gives e + (p' - e) as restated (NOT asserted to be p'); a scale == 0 step still moves the
    weights (decay, moments) and e moves to the restated average of that zero-gradient update, with an inf and a NaN in g."""
    c = _chunk()
    specs = [(5, 1, 3, True), (c + 3, 2, 1, True), (1030, 0, 0, True)]
    tw = Fused(dev, kind, specs, seed=53)
    tw.step(1e-3, 0.5)
    tw.check('first step')
    e0 = tw.e.copy()
    tw.step(2e-3, 0.0)
    tw.check('omd 0')
    assert np.array_equal(oc.bits(tw.e), oc.bits(e0))
    tw.step(2e-3, 1.0)
    tw.check('omd 1')
    g = oc.magnitudes(tw.rs, tw.p.size)
    g[2], g[c + 1] = np.inf, np.nan
    p_before, e_before = tw.p.copy(), tw.e.copy()
    tw.step(1e-3, 0.25, scale=0.0, grads=g)
    tw.check('scale 0')
    assert np.isfinite(tw.p).all() and np.isfinite(tw.e).all()
    assert not np.array_equal(tw.e, e_before)
    if kind == 'adamw_wd':
        assert not np.array_equal(tw.p, p_before)


# ---- og_ema_lerp_f32 ------------------------------------------------------------------------------------------------------------
def _lerp_case(dev, specs, seed, omds, launch=True):
    """specs: (numel, e offset, x offset).  -> nothing; asserts e bit for bit after every call, x and the guards unchanged."""
    lib, chunk = _lib.load(), _chunk()
    rs = np.random.RandomState(seed)
    ns = [s[0] for s in specs]
    cuts = np.cumsum(ns)[:-1]
    e, x = oc.magnitudes(rs, sum(ns), 1e-3, 1e1), oc.magnitudes(rs, sum(ns), 1e-3, 1e1)
    de, dx = Placed(dev, np.split(e, cuts), [s[1] for s in specs]), Placed(dev, np.split(x, cuts), [s[2] for s in specs])
    keep, rows, _, prefix, n_chunks = _table(dev, list(zip(de.ptrs(), dx.ptrs(), ns)), [-(-n // chunk) for n in ns])
    for omd in omds:
        _lib.check(lib.og_ema_lerp_f32(rows, prefix, len(specs), n_chunks if launch else 0, omd, _lib.stream_ptr(dev)), lib)
        torch.cuda.synchronize(dev)
        if launch:
            e = ec.ema_step(e, x, np.float32(omd))
        assert np.array_equal(oc.bits(de.values()), oc.bits(e)), f'omd {omd}: e'
        assert np.array_equal(oc.bits(dx.values()), oc.bits(x)), f'omd {omd}: x'
        assert de.guards_intact() and dx.guards_intact()


def test_lerp_lengths_and_offsets(dev):
    _lerp_case(dev, [(n, eo, xo) for n in _sizes() for eo in range(4) for xo in range(4)], 59, [0.9, 1.0 - 0.9998, 0.0, 1.0])


def test_lerp_300_tensors(dev):
    rs = np.random.RandomState(61)
    _lerp_case(dev, [(int(n), int(a), int(b)) for n, a, b in zip(rs.randint(1, 40, 300), rs.randint(0, 4, 300), rs.randint(0, 4, 300))],
               67, [0.1, 0.5])


def test_lerp_no_chunks_launches_nothing(dev):
    _lerp_case(dev, [(5, 1, 0), (1030, 0, 3)], 71, [0.5], launch=False)


# ---- error cases ----------------------------------------------------------------------------------------------------------------
def test_error_cases_write_nothing(dev):
    lib = _lib.load()
    tw = Fused(dev, 'adamw_wd', [(37, 1, 2, True), (1030, 0, 1, True)], seed=73)
    g = oc.magnitudes(tw.rs, tw.p.size)
    dg = Placed(dev, np.split(g, tw.cuts), tw.go)
    (keep, rows, ema, prefix, n_chunks), _ = tw._tables(dg)
    stream = _lib.stream_ptr(dev)
    adam = lambda ema_, omd: lib.og_adam_step_ema_f32(rows, prefix, 2, 0, n_chunks, None, 1e-3, 0.9, 0.999, 0.1, 0.001, 1e-8, 0.0,   # noqa: E731
                                                      0.1, 0.001, 1, ema_, omd, stream)
    sgd = lambda ema_, omd: lib.og_sgd_step_ema_f32(rows, prefix, 2, 0, n_chunks, None, 1e-3, 0.9, 0.0, 1, ema_, omd, stream)     # noqa: E731
    de, dx = Placed(dev, [tw.e[:37]], [1]), Placed(dev, [tw.p[:37]], [0])
    lkeep, lrows, _, lprefix, lchunks = _table(dev, [(de.ptrs()[0], dx.ptrs()[0], 37)], [1])
    lerp = lambda omd: lib.og_ema_lerp_f32(lrows, lprefix, 1, lchunks, omd, stream)                                               # noqa: E731
    for call in (adam, sgd):
        for bad in ((None, 0.5), (ema + 4, 0.5), (ema, -0.1), (ema, 1.5), (ema, math.nan)):
            assert call(*bad) == _lib.OG_EINVAL, bad
    assert b'ema table' in (adam(None, 0.5), lib.og_last_error())[1]
    assert b'omd' in (sgd(ema, math.nan), lib.og_last_error())[1]
    for omd in (-0.1, 1.5, math.nan):
        assert lerp(omd) == _lib.OG_EINVAL
    assert lib.og_ema_lerp_f32(None, lprefix, 1, lchunks, 0.5, stream) == _lib.OG_EINVAL
    assert lib.og_ema_lerp_f32(lrows, lprefix, 0, lchunks, 0.5, stream) == _lib.OG_EINVAL
    assert lib.og_ema_lerp_f32(lrows + 4, lprefix, 1, lchunks, 0.5, stream) == _lib.OG_EINVAL
    assert lib.og_adam_step_ema_f32(rows, prefix, 2, 0, n_chunks, None, 1e-3, 0.9, 0.999, 0.1, 0.001, 1e-8, 0.0, 0.0, 0.001, 1, ema, 0.5,
                                    stream) == _lib.OG_EINVAL                  # the existing cases hold for the new entry point
    torch.cuda.synchronize(dev)
    for placed, host in ((tw.dp, tw.p), (tw.de, tw.e), (tw.dm, tw.m), (tw.dv, tw.v), (de, tw.e[:37])):
        assert np.array_equal(oc.bits(placed.values()), oc.bits(host)) and placed.guards_intact()


# ---- ModelEma + DeviceAdam.step(ema=) -------------------------------------------------------------------------------------------
class ConvBnConv(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(3, 8, 3, padding=1)
        self.bn = torch.nn.BatchNorm2d(8)
        self.conv2 = torch.nn.Conv2d(8, 5, 3, padding=1)

    def forward(self, x):
        return self.conv2(torch.relu(self.bn(self.conv1(x))))


def _module(dev):
    torch.manual_seed(5)
    net = ConvBnConv().to(dev).to(memory_format=torch.channels_last)
    net.conv2.bias.requires_grad_(False)                      # the frozen parameter: no row in any step
    w = net.conv1.weight
    assert not w.is_contiguous() and w.is_contiguous(memory_format=torch.channels_last)
    return net.train()


class ModuleRun:
    """Training steps of ConvBnConv with DeviceAdam.step(ema=); everything the restatement needs is CLONED on the device inside the
    step (gradients, the source's buffers), so nothing is read back while the steps are queued."""
    WD, NO_GRAD = 1e-2, 'conv1.bias'

    def __init__(self, dev, warmup):
        self.dev, self.net = dev, _module(dev)
        self.opt = optim.DeviceAdam([p for p in self.net.parameters() if p.requires_grad], lr=1e-3, weight_decay=self.WD)
        self.ema = optim.ModelEma(self.net, decay=0.9, warmup=warmup)
        self.images = [torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(i)).to(dev) for i in range(8)]
        self.records, self.count = [], 0

    def step(self, ema):
        net, i = self.net, self.count
        self.count += 1
        self.opt.zero_grad(set_to_none=True)
        (net(self.images[i]) ** 2).mean().backward()
        if i == 2:                                            # (the warm-up step is step 0) step 2 of the three: no gradient
            net.conv1.bias.grad = None
        grads = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
        self.opt.step(ema=ema)
        self.records.append((grads, {n: b.clone() for n, b in net.named_buffers()}))

    def state(self):
        """Host copies (logical order) of p, m, v, Adam's step count per parameter and the shadow."""
        f = lambda t: t.detach().cpu().numpy().copy()                                                      # noqa: E731
        named = dict(self.net.named_parameters())
        st = {n: self.opt.state[p] for n, p in named.items() if p in self.opt.state and 'exp_avg' in self.opt.state[p]}
        return ({n: f(p) for n, p in named.items()}, {n: f(s['exp_avg']) for n, s in st.items()},
                {n: f(s['exp_avg_sq']) for n, s in st.items()}, {n: self.opt._steps[named[n]] for n in st},
                {n: f(t) for n, t in self.ema.module.state_dict().items()})


def _restate(start, records, decay, warmup, first_update):
    """Continue (p, m, v, t, shadow) through the recorded steps -> (p, shadow) per step."""
    p, m, v, t, e = (dict(d) for d in start)
    out = []
    for k, (grads, buffers) in enumerate(records):
        omd = ec.omd_at(decay, warmup, first_update + k)
        for n in p:
            if n in grads:
                t[n] += 1
                p[n], m[n], v[n] = oc.adam_step(p[n], grads[n].cpu().numpy(), m[n], v[n], lr=1e-3, wd=ModuleRun.WD, t=t[n],
                                                adam_w_mode=True)
            e[n] = ec.ema_step(e[n], p[n], omd)
        for n, b in buffers.items():
            b = b.cpu().numpy()
            e[n] = ec.ema_step(e[n], b, omd) if b.dtype == np.float32 else b.copy()
        out.append((dict(p), dict(e)))
    return out


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('warmup', [True, False], ids=['warmup', 'constant'])
def test_model_ema_with_device_adam(dev, warmup):
    """One step outside the guarded region (allocator, pinned slots), the average started again at the weights it left (reset), then
    three steps under sync debug mode 'error'; a state-dict round trip into a fresh ModelEma and two steps more."""
    run = ModuleRun(dev, warmup)
    run.step(run.ema)
    torch.cuda.synchronize(dev)
    run.ema.reset()
    run.records.clear()
    start = run.state()
    assert run.ema.updates == 0 and all(_bits_equal(start[0][n], start[4][n]) for n in start[0])
    before = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode('error')
        for _ in range(3):
            run.step(run.ema)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert run.ema.updates == 3
    steps = _restate(start, run.records, 0.9, warmup, 0)
    p, _, _, t, shadow = run.state()
    assert t == {'conv1.weight': 4, 'conv1.bias': 3, 'bn.weight': 4, 'bn.bias': 4, 'conv2.weight': 4}
    assert set(shadow) == set(run.net.state_dict())
    for n, value in steps[-1][0].items():
        assert _bits_equal(p[n], value), f'p {n}'
    for n, value in steps[-1][1].items():
        assert _bits_equal(shadow[n], value), f'shadow {n}'
    # the running statistics are averaged, not copied; the counter is copied; the frozen parameter's average stays on it
    assert not _bits_equal(shadow['bn.running_var'], run.records[-1][1]['bn.running_var'].cpu().numpy())
    assert not _bits_equal(shadow['bn.running_var'], start[4]['bn.running_var'])
    assert int(shadow['bn.num_batches_tracked']) == int(run.net.bn.num_batches_tracked) == 4
    assert _bits_equal(shadow['conv2.bias'], p['conv2.bias'])
    assert not run.ema.module.training and run.ema.module.conv1.weight.stride() == run.net.conv1.weight.stride()
    # round trip: a fresh ModelEma of the same model continues where this one stands
    other = optim.ModelEma(run.net, decay=0.9, warmup=warmup)
    other.load_state_dict(copy.deepcopy(run.ema.state_dict()))
    assert other.updates == 3
    mid, n_before = run.state(), len(run.records)
    run.ema = other
    for _ in range(2):
        run.step(other)
    torch.cuda.synchronize(dev)
    more = _restate(mid, run.records[n_before:], 0.9, warmup, 3)
    assert other.updates == 5
    shadow = run.state()[4]
    for n, value in more[-1][1].items():
        assert _bits_equal(shadow[n], value), f'resumed shadow {n}'


def test_shadow_of_another_layout_raises(dev):
    run = ModuleRun(dev, True)
    w = run.ema.module.conv1.weight
    w.data = w.data.contiguous()                               # NCHW order beside a channels-last parameter
    assert w.stride() != run.net.conv1.weight.stride()
    with pytest.raises(_lib.OgError, match='layout'):
        run.step(run.ema)
    assert run.ema.updates == 0


def test_update_alone_equals_the_fused_step(dev):
    """ModelEma.update() behind a plain step() averages every tensor in one launch: the same numbers as step(ema=).  The second
    module takes the first one's recorded gradients and buffers instead of a forward and backward of its own: two runs of the
    convolution library need not agree bit for bit (its algorithm choice and its atomics), and that is not what is compared here."""
    a, b = ModuleRun(dev, True), ModuleRun(dev, True)
    named, buffers = dict(b.net.named_parameters()), dict(b.net.named_buffers())
    for _ in range(2):
        a.step(a.ema)
        grads, bufs = a.records[-1]
        for n, p in named.items():
            p.grad = grads[n].clone() if n in grads else None
        with torch.no_grad():
            for n, t in bufs.items():
                buffers[n].copy_(t)
        b.opt.step()
        b.ema.update()
    assert a.ema.updates == b.ema.updates == 2
    for (n, x), (_, y) in zip(a.net.state_dict().items(), b.net.state_dict().items()):
        assert _bits_equal(x.cpu().numpy(), y.cpu().numpy()), f'model {n}'
    for (n, x), (_, y) in zip(a.ema.module.state_dict().items(), b.ema.module.state_dict().items()):
        assert _bits_equal(x.cpu().numpy(), y.cpu().numpy()), n
    assert not _bits_equal(a.ema.module.conv1.weight.cpu().numpy(), a.net.conv1.weight.detach().cpu().numpy())


# ---- the loss scaler ------------------------------------------------------------------------------------------------------------
class Holder(torch.nn.Module):
    def __init__(self, arrays, dev):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(a.copy()).to(dev)) for a in arrays])


def test_scaler_and_ema_together(dev):
    """S = 2^16: the step on S * g with scaler= and ema= equals the scaler-less step on g with ema=, the average included."""
    rs = np.random.RandomState(79)
    arrays = [oc.magnitudes(rs, n, 1e-3, 1e1) for n in (5, 1030, _chunk() + 3)]
    grads = [oc.magnitudes(rs, a.size, 1e-6, 1e-2) for a in arrays]
    scaled, plain = Holder(arrays, dev), Holder(arrays, dev)
    for holder, factor in ((scaled, 65536.0), (plain, 1.0)):
        for p, g in zip(holder.ps, grads):
            p.grad = torch.from_numpy(g * np.float32(factor)).to(dev)
    emas = [optim.ModelEma(h, decay=0.9, warmup=False) for h in (scaled, plain)]
    for ema in emas:                                          # an average that differs from the weights
        with torch.no_grad():
            for e in ema.module.ps:
                e.mul_(0.75)
    opts = [optim.DeviceAdam(h.ps, lr=1e-3, weight_decay=1e-2) for h in (scaled, plain)]
    scaler = optim.DeviceLossScaler(init_scale=2. ** 16, device=dev)
    opts[0].step(scaler=scaler, ema=emas[0])
    opts[1].step(ema=emas[1])
    assert int(scaler.last_overflow) == 0 and emas[0].updates == emas[1].updates == 1
    omd = ec.omd_at(0.9, False, 0)
    for i, (a, g) in enumerate(zip(arrays, grads)):
        p2, m2, v2, e2 = ec.adam_step_ema(a, g, np.zeros_like(a), np.zeros_like(a), a * np.float32(0.75), omd, lr=1e-3, wd=1e-2, t=1,
                                          adam_w_mode=True)
        for holder, ema, opt in zip((scaled, plain), emas, opts):
            assert _bits_equal(holder.ps[i].detach().cpu().numpy(), p2)
            assert _bits_equal(ema.module.ps[i].cpu().numpy(), e2)
            assert _bits_equal(opt.state[holder.ps[i]]['exp_avg'].cpu().numpy(), m2)
            assert _bits_equal(opt.state[holder.ps[i]]['exp_avg_sq'].cpu().numpy(), v2)


# ---- the engine -----------------------------------------------------------------------------------------------------------------
def test_engine_refreshed_from_the_shadow(dev):
    """The model and shapes of tests/test_gpu_engine_refresh.py: an fp16 graph engine built from the model, refreshed from
    ema.module after the model moved and the average followed, replays what an engine built afresh from ema.module replays."""
    eng_mod.invalidate_engine_cache()
    model = rc.perturb(rc.make_model(), 1).to(dev).to(memory_format=torch.channels_last)
    ema = optim.ModelEma(model, decay=0.9998)
    engine = models.InferenceEngine(model, 1, 128, 128, dtype=torch.float16, device=dev)
    assert engine.fused and engine._graph is not None
    x = torch.randn(engine.shape, generator=torch.Generator().manual_seed(5)).to(dev)
    old = [o.clone() for o in engine.forward_raw(x)]
    ptrs = {k: t.data_ptr() for k, t in rc.persistent(engine._layers).items()}
    rc.perturb(model, 2)
    ema.update()                                              # update 0 with warm-up: decay 0.1, the shadow moves most of the way
    assert ema.updates == 1 and not torch.equal(ema.module.basenet.pre[1].conv1.weight, model.basenet.pre[1].conv1.weight)
    engine.refresh(model=ema.module)
    assert {k: t.data_ptr() for k, t in rc.persistent(engine._layers).items()} == ptrs
    new = [o.clone() for o in engine.forward_raw(x)]
    eng_mod.invalidate_engine_cache()
    fresh = models.InferenceEngine(ema.module, 1, 128, 128, dtype=torch.float16, device=dev)
    assert fresh._layers is not engine._layers
    mine, theirs = rc.persistent(engine._layers), rc.persistent(fresh._layers)
    assert list(mine) == list(theirs) and all(torch.equal(mine[k], theirs[k]) for k in mine)
    new_fresh = [o.clone() for o in fresh.forward_raw(x)]
    torch.cuda.synchronize(dev)
    assert all(bool(torch.isfinite(o).all()) for o in new)
    assert all(torch.equal(a, b) for a, b in zip(new, new_fresh))
    assert not any(torch.equal(a, b) for a, b in zip(new, old))
