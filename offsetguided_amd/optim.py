"""Optimizers whose step never waits for the device: DeviceAdam (apex FusedAdam of the reference, train_dist.py:236-246) and
DeviceSGD on the multi-tensor HIP kernels of csrc/optim.hip (include/og_decoder.h, "training step without a host wait").

step(loss=..., max_grad_norm=...) queues three launches on the current stream: the sum of squares of every gradient, the scale block
(the clip coefficient of torch.nn.utils.clip_grad_norm_ and the reference's `loss > 1e8` batch drop in ONE device-side number), and
the update, which multiplies every gradient by that number.  Nothing is read back: `last_grad_norm` and `dropped_steps` are device
tensors the caller converts when it prints.  step(..., scaler=DeviceLossScaler()) is the fp16 form (apex amp O1's dynamic loss
scaling, train_dist.py:336): the scale block in its scaler form also unscales, skips a step whose gradients overflowed and moves the
loss scale.  The update is one kernel with a rule: a subclass names its entry point and the rule's arguments (_rule), step() launches.

The state keys are torch's (`step`, `exp_avg`, `exp_avg_sq`, `momentum_buffer`): a checkpoint written with torch.optim.Adam / SGD
resumes here and the other way round.  `step` is counted on the host; the tensors under state[p]['step'] are brought up to date by
state_dict().

ModelEma keeps an exponential moving average of a model's weights in a shadow module; step(..., ema=ModelEma(model)) folds the
average of every parameter it updates into the update launch itself (og_adam_step_ema_f32 / og_sgd_step_ema_f32) and averages the
rest -- BatchNorm statistics, frozen parameters -- in one og_ema_lerp_f32 launch behind it.
"""
import copy
import math

import numpy as np
import torch

from . import _lib, _table


def _same_layout(a, b):
    """Same element order in memory: equal strides on every dimension longer than one."""
    return a.shape == b.shape and all(sa == sb for n, sa, sb in zip(a.shape, a.stride(), b.stride()) if n != 1)


def _dense(t):
    """Non-overlapping and dense: the tensor's elements are numel() consecutive addresses in some order."""
    if t.is_contiguous():
        return True
    expected = 1
    for stride, size in sorted((st, n) for n, st in zip(t.shape, t.stride()) if n != 1):
        if stride != expected:
            return False
        expected *= size
    return True


def _no_cpu_path(owner, what, tensor):
    """The error for a tensor that is not on a GPU; the caller tests is_cuda (in a step's loops, once per tensor) and raises it."""
    return _lib.OgError(f'{owner}: {what} on {tensor.device}; the HIP kernels need GPU tensors (offsetguided_amd has no CPU path)')


class _DeviceTable:
    """A tensor table (_table.py) on the device, cached: put() packs and uploads only when what it was built from has changed."""

    def __init__(self):
        self._pool = _table.Pool()
        self._signature = self._tensor = None
        self.n_rows = self.n_chunks = self._extra_at = self._prefix_at = 0

    def forget(self):
        self._signature = None

    def put(self, signature, rows, words, chunk, dev, extra=None):
        """rows: a tuple of `words` int64 per tensor, the last its element count (`chunk` elements to a workgroup); extra: _table.pack's.
        -> the host prefix of a table that was built anew, None when `signature` is the one the device table already has."""
        if signature == self._signature:
            return None
        table = np.array(rows, dtype=np.int64).reshape(-1, words)
        raw, prefix, self._prefix_at = _table.pack(table, -(-table[:, -1] // chunk), extra)
        self._tensor = _table.upload(raw, dev, self._pool)
        self.n_rows, self.n_chunks, self._extra_at = len(rows), int(prefix[-1]), 8 * table.size
        self._signature = signature
        return prefix

    rows = property(lambda self: self._tensor.data_ptr())                        # device addresses of the table's three parts
    extra = property(lambda self: self._tensor.data_ptr() + self._extra_at)
    prefix = property(lambda self: self._tensor.data_ptr() + self._prefix_at)


class DeviceLossScaler:
    """apex amp O1's LossScaler with its state on the device: a 16-byte block [loss_scale f32, unskipped i32, overflows i32,
    last_overflow i32] that og_step_scale_amp_f32 reads and moves inside the optimizer's step (include/og_decoder.h has the rule).
    loss_scale: 'dynamic' (start at init_scale, divide by scale_factor on an overflow, multiply after scale_window clean steps,
    inside [min_loss_scale, max_loss_scale]) or a number (static).  Only state_dict() reads anything back."""

    def __init__(self, loss_scale='dynamic', init_scale=2. ** 16, scale_factor=2., scale_window=2000, min_loss_scale=1.,
                 max_loss_scale=2. ** 24, device=None):
        self.dynamic = loss_scale == 'dynamic'
        start = float(init_scale if self.dynamic else loss_scale)
        min_loss_scale = 1. if min_loss_scale is None else min_loss_scale      # apex: None = no lower bound; a scale stays positive here
        numbers = (start, scale_factor, min_loss_scale, max_loss_scale)
        if not all(math.isfinite(x) for x in numbers) or not (start > 0 and scale_factor > 1 and int(scale_window) >= 1
                                                              and min_loss_scale > 0 and max_loss_scale >= min_loss_scale):
            raise ValueError(f'DeviceLossScaler: bad hyper-parameters loss_scale={loss_scale} init_scale={init_scale} '
                             f'scale_factor={scale_factor} scale_window={scale_window} min_loss_scale={min_loss_scale} '
                             f'max_loss_scale={max_loss_scale}')
        self.scale_factor, self.scale_window = float(scale_factor), int(scale_window)
        self.min_loss_scale, self.max_loss_scale = float(min_loss_scale), float(max_loss_scale)
        if device is None:
            device = 'cuda' if torch.cuda.is_available() else 'cpu'
        device = torch.device(device)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device.type == 'cuda' and device.index is None else device
        # a tensor of its own, never a slice of the optimizer's workspace (that one is reallocated when the parameter list grows)
        self._block = self._words(start, 0, 0, 0).to(self.device)

    @staticmethod
    def _words(loss_scale, unskipped, overflows, last_overflow):
        words = np.array([0, unskipped, overflows, last_overflow], dtype=np.int32)
        words[:1].view(np.float32)[0] = loss_scale
        return torch.from_numpy(words)

    def scale(self, loss):
        """loss * loss_scale, a product of device tensors: call backward() on it."""
        return loss * self.loss_scale

    @property
    def loss_scale(self):
        """fp32 device scalar: the factor the next backward's gradients carry."""
        return self._block[0:1].view(torch.float32)[0]

    @property
    def unskipped(self):
        """int32 device scalar: steps without an overflow since the scale last moved (dynamic)."""
        return self._block[1]

    @property
    def overflow_steps(self):
        """int32 device scalar: steps a dynamic scaler skipped for a non-finite gradient."""
        return self._block[2]

    @property
    def last_overflow(self):
        """int32 device scalar: 1 when the last step met a non-finite gradient."""
        return self._block[3]

    def state_dict(self):
        """apex's keys.  The one read-back: called when a checkpoint is written."""
        host = self._block.cpu()
        return {'loss_scale': float(host[0:1].view(torch.float32)[0]), 'unskipped': int(host[1])}

    def load_state_dict(self, state):
        """Scale and window position of a checkpoint (as apex does, also into a static scaler: the run goes on at the scale it had)."""
        scale, unskipped = float(state['loss_scale']), int(state['unskipped'])
        if not (math.isfinite(scale) and scale > 0 and unskipped >= 0):
            raise ValueError(f'DeviceLossScaler: bad state loss_scale={scale} unskipped={unskipped}')
        self._block[:2].copy_(self._words(scale, unskipped, 0, 0)[:2])


def amp_state_dict(scaler):
    """The layout of apex's amp.state_dict() with one loss scaler: save_model(amp_state=...) writes it as the checkpoint's `amp`."""
    return {'loss_scaler0': scaler.state_dict()}


def load_amp_state(scaler, state):
    """The `amp` entry of a checkpoint (load_model(load_amp=True)'s last result; False when the file has none) into the scaler.
    -> whether a state was loaded."""
    if not state:
        return False
    if 'loss_scaler0' not in state:
        raise ValueError(f"amp state without 'loss_scaler0' (keys {sorted(state)})")
    scaler.load_state_dict(state['loss_scaler0'])
    return True


class ModelEma:
    """An exponential moving average of a model's weights (include/og_decoder.h, "weight average"): e' = e + (1 - decay) (x - e) per
    element and update.  `module` is the shadow: a deep copy of the model (a DistributedDataParallel wrapper is unwrapped) in eval(),
    without gradients, every tensor in the memory layout of its source -- hand it to InferenceEngine(...), engine.refresh(model=) or
    save_model.  decay_at(t), t the updates taken so far: min(decay, (1 + t) / (10 + t)) with warmup (the TF / timm schedule), else
    decay.  The shadow follows the tensors the model has when this is made (or bind() is called): move the model to its device and
    memory format first.  optimizer.step(..., ema=this) is the fused update; update() averages every tensor in one launch of its own
    (behind another optimizer).  There is no CPU path: on a CPU module everything but an update works."""

    def __init__(self, model, decay=0.9998, warmup=True):
        if not 0 <= decay < 1:
            raise ValueError(f'ModelEma: decay must lie in [0, 1), got {decay}')
        self.decay, self.warmup, self.updates = float(decay), bool(warmup), 0
        model = _unwrap(model)
        self.module = copy.deepcopy(model).eval().requires_grad_(False)
        self._table = _DeviceTable()
        self.bind(model)

    _n_rows = property(lambda self: self._table.n_rows)      # rows of the last update()'s launch

    def bind(self, model):
        """Pair the tensors of `model` (by state_dict() name) with the shadow's and bring every shadow tensor to its source's layout."""
        source = _unwrap(model).state_dict(keep_vars=True)
        shadow = self.module.state_dict(keep_vars=True)
        if list(source) != list(shadow):
            raise ValueError('ModelEma.bind: the model does not have the tensors of the shadow module')
        with torch.no_grad():
            for name, x in source.items():
                e = shadow[name]
                if e.shape != x.shape or e.dtype != x.dtype:
                    raise ValueError(f'ModelEma.bind: {name} is {tuple(x.shape)} {x.dtype}, the shadow has {tuple(e.shape)} {e.dtype}')
                if e.device != x.device or not _same_layout(e, x):
                    e.data = torch.empty_like(x).copy_(e)
        self.tensors = {name: (x, shadow[name]) for name, x in source.items()}      # name -> (source tensor, shadow tensor)
        self._shadow_of = {x: e for x, e in self.tensors.values()}                   # tensors hash by identity
        self._table.forget()

    @torch.no_grad()
    def reset(self):
        """Start the average again from the bound model's present weights (after they were loaded from a file without an average)."""
        for x, e in self.tensors.values():
            e.copy_(x)
        self.updates = 0

    def decay_at(self, t):
        """The decay of the update after t updates (Python double)."""
        return min(self.decay, (1.0 + t) / (10.0 + t)) if self.warmup else self.decay

    def shadow_of(self, tensor):
        """The shadow tensor of a parameter or buffer of the bound model, or None."""
        return self._shadow_of.get(tensor)

    def state_dict(self):
        return {'module': self.module.state_dict(), 'updates': self.updates}

    def load_state_dict(self, state):
        self.module.load_state_dict(state['module'])        # copies in place: the layouts stay
        self.updates = int(state['updates'])

    @torch.no_grad()
    def update(self, skip=()):
        """Queue one update of the average on the current stream, at decay_at(updates): ONE og_ema_lerp_f32 launch over every
        floating tensor of the shadow's state_dict() whose source is not in `skip` (the parameters an optimizer's fused update has
        just averaged), copy_ for the integer buffers (num_batches_tracked); updates += 1.  Never waits for the device."""
        dev = None
        rows, ints, seen = [], [], set()
        for name, (x, e) in self.tensors.items():
            if e in seen:             # one tensor under two names (tied weights) is averaged once
                continue
            seen.add(e)
            if not x.is_cuda or not e.is_cuda:
                raise _no_cpu_path('ModelEma.update', name, x)
            if not e.is_floating_point():
                ints.append((e, x))
                continue
            if x in skip or x.numel() == 0:
                continue
            dev = x.device if dev is None else dev
            _check_shadow(name, x, e, dev)
            rows.append((e.data_ptr(), x.data_ptr(), x.numel()))
        omd = 1.0 - self.decay_at(self.updates)
        if rows:
            lib, t = _lib.load(), self._table
            with torch.cuda.device(dev):
                t.put(tuple(rows), rows, 3, lib.og_optim_chunk_elems(), dev)
                _lib.check(lib.og_ema_lerp_f32(t.rows, t.prefix, t.n_rows, t.n_chunks, omd, _lib.stream_ptr(dev)), lib)
        for e, x in ints:
            e.copy_(x)
        self.updates += 1


def _unwrap(model):
    return model.module if isinstance(model, (torch.nn.parallel.DistributedDataParallel, torch.nn.DataParallel)) else model


def _check_shadow(name, x, e, dev):
    """A source tensor and its average as the kernels take them: dense fp32 on `dev` in one element order.  The shadow is the
    caller's: a layout that differs is an error, not something to fix behind their back."""
    if x.dtype != torch.float32 or e.dtype != torch.float32:
        raise _lib.OgError(f'ModelEma: {name}: fp32 tensors only (got {x.dtype}, shadow {e.dtype})')
    if x.device != dev or e.device != dev:
        raise _lib.OgError(f'ModelEma: {name} on {x.device}, its shadow on {e.device}, the step on {dev}; one device')
    if not _same_layout(e, x) or not _dense(x):
        raise _lib.OgError(f'ModelEma: {name}: the shadow tensor (shape {tuple(e.shape)}, strides {e.stride()}) does not have the layout '
                           f'of its source (shape {tuple(x.shape)}, strides {x.stride()}), or the source is not dense')


class _DeviceOptimizer(torch.optim.Optimizer):
    MOMENTS = ()      # state keys of the m and v columns of the table

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._steps = {}          # parameter -> steps taken (the host's count; state[p]['step'] follows in state_dict())
        self._checked = set()     # parameters whose state tensors are known to have the parameter's layout
        self._table = _DeviceTable()
        self._segments = []       # (group index, key, first chunk, chunk count)
        self._ws = None

    _n_chunks = property(lambda self: self._table.n_chunks)      # chunks of the last step's table

    # ---- the state block ------------------------------------------------------------------------------------------------------
    def _device(self):
        for group in self.param_groups:
            for p in group['params']:
                if not p.is_cuda:
                    raise _no_cpu_path(type(self).__name__, 'parameter', p)
                return p.device
        raise _lib.OgError(f'{type(self).__name__}: no parameters')

    def _workspace(self, dev, lib):
        chunk = lib.og_optim_chunk_elems()
        most = sum(-(-p.numel() // chunk) for group in self.param_groups for p in group['params'])
        need = lib.og_optim_workspace_bytes(most)
        if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            ws = torch.zeros(need, dtype=torch.uint8, device=dev)
            if self._ws is not None and self._ws.device == dev:
                ws[:16].copy_(self._ws[:16])          # the dropped-batch count lives on
            self._ws = ws
        return self._ws

    def _state_word(self, i, dtype):
        """Word i of the workspace's state block [scale f32, norm f32, dropped i32] as a device scalar."""
        return self._workspace(self._device(), _lib.load())[4 * i:4 * i + 4].view(dtype)[0]

    last_scale = property(lambda self: self._state_word(0, torch.float32),
                          doc='fp32 device scalar: what the last step multiplied the gradients by (0: dropped, below 1: clipped).')
    last_grad_norm = property(lambda self: self._state_word(1, torch.float32),
                              doc='fp32 device scalar: the gradient norm of the last step that computed one (before clipping).')
    dropped_steps = property(lambda self: self._state_word(2, torch.int32),
                             doc='int32 device scalar: steps dropped so far (loss above loss_limit, or a non-finite gradient).')

    # ---- checkpoints ----------------------------------------------------------------------------------------------------------
    def state_dict(self):
        for p, t in self._steps.items():
            if p in self.state:
                self.state[p]['step'] = torch.tensor(float(t), dtype=torch.float32)
        return super().state_dict()

    def load_state_dict(self, state_dict):
        for group in state_dict['param_groups']:
            if group.get('amsgrad') or group.get('maximize') or group.get('nesterov') or group.get('dampening'):
                raise ValueError(f'{type(self).__name__}: the checkpoint asks for amsgrad, maximize, nesterov or dampening, which the '
                                 'HIP kernels do not implement')
        own = [dict(group) for group in self.param_groups]
        super().load_state_dict(state_dict)
        for group, old in zip(self.param_groups, own):     # a torch checkpoint has no adam_w_mode: this optimizer's stays
            for k, v in old.items():
                group.setdefault(k, v)
        self._steps = {p: int(round(float(st['step']))) for p, st in self.state.items() if st.get('step') is not None}
        self._checked = set()
        self._table.forget()

    # ---- the tensor table -----------------------------------------------------------------------------------------------------
    def _init_state(self, p, group, state):
        raise NotImplementedError

    def _key(self, p, group, state):
        raise NotImplementedError

    def _rule(self, group, key):
        """(the entry point's stem, the rule's arguments) of the segment `key` of `group`: step() calls stem + '_f32' or '_ema_f32'."""
        raise NotImplementedError

    def _after(self, entries):
        pass

    def _entries(self, dev):
        """[(group index, segment key, parameter, gradient, state)] of the parameters that have a gradient, segment by segment."""
        out = []
        for gi, group in enumerate(self.param_groups):
            for p in group['params']:
                g = p.grad
                if g is None:
                    continue
                if not p.is_cuda or not g.is_cuda:
                    raise _no_cpu_path(f'{type(self).__name__}.step', 'parameter', p)
                if p.device != dev:
                    raise _lib.OgError(f'{type(self).__name__}.step: parameters on {dev} and {p.device}; one device per optimizer')
                if p.dtype != torch.float32 or g.dtype != torch.float32 or g.is_sparse:
                    raise _lib.OgError(f'{type(self).__name__}.step: dense fp32 parameters and gradients only (got {p.dtype}, {g.dtype})')
                if p.numel() == 0:
                    continue
                state = self.state[p]
                if p not in self._checked:
                    if not _dense(p):
                        raise _lib.OgError(f'{type(self).__name__}.step: a parameter of shape {tuple(p.shape)} with strides '
                                           f'{p.stride()} is not dense')
                    self._init_state(p, group, state)
                    for k in self.MOMENTS:          # a checkpoint of another memory format: bring it to the parameter's
                        if state.get(k) is not None and not _same_layout(state[k], p):
                            state[k] = torch.empty_like(p).copy_(state[k])
                    self._checked.add(p)
                if not _same_layout(g, p):
                    g = torch.empty_like(p).copy_(g)
                out.append((gi, self._key(p, group, state), p, g, state))
        out.sort(key=lambda e: e[:2])               # stable: list order inside a segment
        return out

    def _averages(self, entries, dev, ema):
        """The address of every entry's average in the shadow of `ema`, 0 where the parameter is not in it."""
        out = []
        for _, _, p, _, _ in entries:
            e = ema.shadow_of(p)
            if e is not None:
                _check_shadow(f'a parameter of shape {tuple(p.shape)}', p, e, dev)
            out.append(0 if e is None else e.data_ptr())
        return out

    def _upload(self, entries, dev, lib, ema=None):
        moments = self.MOMENTS + (None,) * (2 - len(self.MOMENTS))
        rows = [(p.data_ptr(), g.data_ptr(), *(st[k].data_ptr() if k and st.get(k) is not None else 0 for k in moments), p.numel())
                for _, _, p, g, st in entries]
        keys = [e[:2] for e in entries]
        averages = None if ema is None else self._averages(entries, dev, ema)      # travels behind the rows, before the prefix
        prefix = self._table.put((rows, keys, averages), rows, 5, lib.og_optim_chunk_elems(), dev, averages)
        if prefix is None:
            return
        self._segments = []
        for i, key in enumerate(keys):
            if i == 0 or key != keys[i - 1]:
                self._segments.append([key[0], key[1], int(prefix[i]), 0])
            self._segments[-1][3] = int(prefix[i + 1]) - self._segments[-1][2]

    @torch.no_grad()
    def step(self, closure=None, *, loss=None, max_grad_norm=math.inf, loss_limit=1e8, scaler=None, ema=None):
        """Queue one optimisation step on the current stream.  loss: the weighted fp32 loss on the device (a batch whose loss exceeds
        loss_limit is dropped); max_grad_norm: clip_grad_norm_'s max_norm over every gradient.  With neither, only the update runs.
        scaler: the DeviceLossScaler whose scale(loss) was sent backward -- the sum of squares always runs, the scale block unscales
        (and clips) with one number, skips the step on a non-finite gradient and moves the loss scale; loss is the unscaled one.
        ema: a ModelEma -- the update launches average every parameter they step that is in its shadow (also on a dropped or skipped
        step: the average follows the weights the model has), one more launch averages the shadow's other tensors, ema.updates += 1.
        Never waits for the device."""
        out = None
        if closure is not None:
            with torch.enable_grad():
                out = closure()
        if max_grad_norm != max_grad_norm or max_grad_norm <= 0:
            raise ValueError(f'max_grad_norm must be positive, got {max_grad_norm}')
        dev = self._device()
        if scaler is not None and scaler.device != dev:
            raise _lib.OgError(f'{type(self).__name__}.step: loss scaler on {scaler.device}, parameters on {dev}; the scale block reads '
                               'the scaler on the device it runs on')
        lib = _lib.load()
        entries = self._entries(dev)
        if not entries:
            if ema is not None:
                ema.update()
            return out
        with torch.cuda.device(dev):
            ws = self._workspace(dev, lib)
            self._upload(entries, dev, lib, ema)
            stream, t = _lib.stream_ptr(dev), self._table
            suffix, avg = ('_f32', ()) if ema is None else ('_ema_f32', (t.extra, 1.0 - ema.decay_at(ema.updates)))
            state_ptr = None
            if loss is not None or math.isfinite(max_grad_norm) or scaler is not None:
                if loss is not None:
                    loss = _lib.require_device(loss.detach(), 'loss')
                    if loss.numel() != 1:
                        raise ValueError(f'loss: one element expected, got {tuple(loss.shape)}')
                _lib.check(lib.og_grad_sumsq_f32(t.rows, t.prefix, t.n_rows, t.n_chunks, _lib.ptr(ws), ws.numel(), stream), lib)
                loss_ptr = _lib.ptr(loss) if loss is not None else None
                if scaler is None:
                    _lib.check(lib.og_step_scale_f32(t.n_chunks, loss_ptr, loss_limit, max_grad_norm, _lib.ptr(ws), ws.numel(),
                                                     stream), lib)
                else:
                    _lib.check(lib.og_step_scale_amp_f32(t.n_chunks, loss_ptr, loss_limit, max_grad_norm, _lib.ptr(scaler._block),
                                                         int(scaler.dynamic), scaler.scale_factor, scaler.scale_window,
                                                         scaler.min_loss_scale, scaler.max_loss_scale, _lib.ptr(ws), ws.numel(),
                                                         stream), lib)
                state_ptr = _lib.ptr(ws)
            for gi, key, first, count in self._segments:
                stem, args = self._rule(self.param_groups[gi], key)
                _lib.check(getattr(lib, stem + suffix)(t.rows, t.prefix, t.n_rows, first, count, state_ptr, *args, *avg, stream), lib)
            if ema is not None:
                ema.update(skip={p for _, _, p, _, _ in entries if ema.shadow_of(p) is not None})
        self._after(entries)
        return out


class DeviceAdam(_DeviceOptimizer):
    """Adam on og_adam_step_f32.  adam_w_mode=True (apex FusedAdam's default, the reference's update) decays the weights next to the
    step; False is torch.optim.Adam's L2 form; with weight_decay == 0 the two are the same."""
    MOMENTS = ('exp_avg', 'exp_avg_sq')

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, adam_w_mode=True):
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError(f'DeviceAdam: bad hyper-parameters lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}')
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, adam_w_mode=bool(adam_w_mode)))

    def _init_state(self, p, group, state):
        if 'exp_avg' not in state:
            state['step'] = torch.tensor(0.0, dtype=torch.float32)
            state['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        self._steps.setdefault(p, 0)

    def _key(self, p, group, state):
        return self._steps[p]

    def _rule(self, group, key):
        t = key + 1
        b1, b2 = group['betas']
        return 'og_adam_step', (group['lr'], b1, b2, 1.0 - b1, 1.0 - b2, group['eps'], group['weight_decay'], 1.0 - b1 ** t,
                                1.0 - b2 ** t, int(group.get('adam_w_mode', True)))

    def _after(self, entries):
        for _, _, p, _, _ in entries:
            self._steps[p] += 1


class DeviceSGD(_DeviceOptimizer):
    """torch.optim.SGD (dampening 0, no Nesterov) on og_sgd_step_f32; with momentum == 0 no buffer exists."""
    MOMENTS = ('momentum_buffer',)

    def __init__(self, params, lr, momentum=0, weight_decay=0):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError(f'DeviceSGD: bad hyper-parameters lr={lr} momentum={momentum} weight_decay={weight_decay}')
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay))
        self._fresh = set()       # parameters whose momentum buffer has not been written yet

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._fresh = set()

    def _init_state(self, p, group, state):
        if group['momentum'] != 0 and state.get('momentum_buffer') is None:
            state['momentum_buffer'] = torch.zeros_like(p, memory_format=torch.preserve_format)    # the first step writes it, reads nothing
            self._fresh.add(p)

    def _key(self, p, group, state):
        return 1 if p in self._fresh else 0

    def _rule(self, group, key):
        return 'og_sgd_step', (group['lr'], group['momentum'], group['weight_decay'], key)

    def _after(self, entries):
        self._fresh.difference_update(e[2] for e in entries)
