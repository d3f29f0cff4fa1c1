"""The six fused loss kernels of csrc/losses.hip on the raw entry points, and the autograd wrappers of models/losses.py, against
the float64 restatement tests/losses_fp64.py (itself held to models/losses.py in float64 by tests/test_losses_fp64_cpu.py) at
the training shapes (batch 8, 128 x 128 maps: up to 10 grid-stride passes per lane), on either side of the 2048-block grid cap
on the 16-byte and the 4-byte path, at unit counts around a wave and a block, with misaligned operands, mask bytes from
{0, 1, 2, 255}, gamma in {1, 2, 0.5}, tau in {0.01, 0.5}, both margins, and the refusal paths.

Bounds (u = 2^-24; the derivations are in tests/losses_fp64.py's docstring, which computes `gbound` per element):
  gradient   roundings from the inputs to g, 1 u each, plus 2 u (1 ulp, HIP math-API accuracy table) per sqrtf / expf / powf;
             division is charged 1 u (correctly rounded: the library is built without fast-math):
               l2 1 u |g|; masked l1 0 (g = +-1) or 4 u |g| with sqrt; offset l1 u |g| or (4 u + 0.5 E/e) |g| with sqrt;
               focal 4 u (|A| + |B|) at gamma = 1, 9 u at gamma = 2, 8.5 u at gamma = 0.5 (g = A + B, relative to the terms);
               vector l1 7 u |g|, 12 u with sqrt; laplace (10 u + rel_k) |g| for pred, |k| ((rel_k + 2 u) |1 - r inv| + 7 u r inv)
               for logb, rel_k = 0 or 3 u + 0.5 Ev / v.
             The tolerance is the smaller of that bound and the suite's rtol 1e-5 / atol 1e-7, so it is never looser than
             either.  offset l1 with sqrt_re: where |p/ps| + |g/ps| > 7 e or so the float32 difference has lost more than the
             later roundings add; those elements (`cont`) are held, under the same cap, to the float64 continuation from the
             float32 difference fl(fl(p/ps) - fl(g/ps)) with 4 u for sgn / ps, sqrtf and the divide.
             One deviation from "never looser than rtol 1e-5 / atol 1e-7": the laplace kernel where the value under the root
             (logb + r inv with logb < 0) or grad_logb = k (1 - r inv) with r inv within a factor 2 of 1 cancels (`ill`,
             `ill_logb`).  The 7 u of r inv (4.2e-7 at 1) then remain as an absolute error above the atol (observed: 1.7e-7),
             and expf is not correctly rounded, so fl(r inv) cannot be restated: where the derived bound exceeds the cap on
             such an element it stands alone; how many is printed (`uncapped`).
  sum        |got - ref| <= (m + 6 + W) u sum|term|, m the longest per-lane chain, 6 wave-reduction levels, W one atomic per wave,
             from the launch geometry (losses_fp64.geometry).  Exact cases (dyadic inputs, every partial sum an integer number
             of quanta below 2^24): got == ref.  A case with nb borderline elements gets nb * 2 * margin more (nb *
             2 * sqrt(margin) with sqrt_re): a borderline term, about the margin in size, may enter or leave the sum.
  count      exact, but for at most 4 borderline elements per case (the CPU test asserts the cap).
Every figure is printed as an `FP64FIG` line before it is asserted (EXPERIMENTS.md has the table)."""
import ctypes

import numpy as np
import pytest
import torch

import losses_fp64 as ref64
import losses_heads_common as common
from offsetguided_amd import _lib
from offsetguided_amd.models import losses

pytestmark = pytest.mark.gpu

U = ref64.U
CANARY = 0x7FC0DEAD                       # a NaN: an element the kernel skipped stays non-finite
GUARD = 64                                # floats on either side of every output
FLOAT_OPERANDS = {'focal': ('pred', 'gt', 'grad'), 'offset': ('pred', 'gt', 'ps', 'grad'), 'l2': ('pred', 'gt', 'grad'),
                  'ml1': ('pred', 'gt', 'grad'), 'vector': ('pred', 'gt', 'grad'),
                  'laplace': ('pred', 'gt', 'logb', 'grad', 'grad_logb')}


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    return torch.device('cuda:0')


def _in(arr, off, dev):
    """The array as a view `off` items into a larger device allocation."""
    flat = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1))
    buf = torch.zeros(flat.numel() + 16, dtype=flat.dtype, device=dev)
    view = buf[off:off + flat.numel()]
    view.copy_(flat)
    return view


class _Out:
    """n floats filled with the canary, guard bands on both sides, `off` floats off the 16-byte grid."""

    def __init__(self, n, off, dev):
        self.raw = torch.full((GUARD + n + GUARD + 4,), CANARY, dtype=torch.int32, device=dev)
        self.lo, self.n = GUARD + off, n
        self.view = self.raw.view(torch.float32)[self.lo:self.lo + n]

    def guards_intact(self):
        return bool((self.raw[:self.lo] == CANARY).all()) and bool((self.raw[self.lo + self.n:] == CANARY).all())

    def untouched(self):
        return bool((self.raw == CANARY).all())

    def numpy(self, shape):
        return self.view.cpu().numpy().reshape(shape)


def _arglist(kernel, case, P, shape=None):
    n, c, hw = shape or (case['n'], case['c'], case['hw'])
    ms = (float(case.get('margin', 0)), int(case.get('sqrt_re', 0)))
    if kernel == 'focal':
        return [P['pred'], P['gt'], P['mask'], n, c, hw, float(case['tau']), float(case['gamma']), P['acc'], P['grad']]
    if kernel == 'offset':
        return [P['pred'], P['gt'], P['ps'], P['mask'], n, c, hw, *ms, P['acc'], P['grad']]
    if kernel == 'l2':
        return [P['pred'], P['gt'], P['mask'], n, c, hw, P['acc'], P['grad']]
    if kernel in ('ml1', 'vector'):
        return [P['pred'], P['gt'], P['mask'], n, c, hw, *ms, P['acc'], P['grad']]
    return [P['pred'], P['gt'], P['logb'], P['mask'], n, c, hw, *ms, P['acc'], P['grad'], P['grad_logb']]


class _Call:
    """One launch of a case's entry point: operands staged (each `offs[name]` items off alignment), outputs canary-filled."""

    def __init__(self, case, offs=None, preload=(0.0, 0.0)):
        dev, offs, k = _dev(), offs or {}, case['kernel']
        self.case, self.kernel = case, k
        self.ins = {name: _in(case[name], offs.get(name, 0), dev) for name in ('pred', 'gt', 'ps', 'logb', 'mask') if name in case}
        self.grad = _Out(case['pred'].size, offs.get('grad', 0), dev)
        self.grad_logb = _Out(case['logb'].size, offs.get('grad_logb', 0), dev) if k == 'laplace' else None
        self.acc = torch.tensor([preload[0], preload[1], 12345.0], dtype=torch.float32, device=dev)
        self.ptrs = {name: _lib.ptr(t) for name, t in self.ins.items()}
        self.ptrs.update(acc=_lib.ptr(self.acc), grad=_lib.ptr(self.grad.view))
        if self.grad_logb is not None:
            self.ptrs['grad_logb'] = _lib.ptr(self.grad_logb.view)
        self.aligned = all(p.value % 16 == 0 for name, p in self.ptrs.items() if name != 'acc')

    def run(self, null=None, shape=None):
        lib = _lib.load()
        P = dict(self.ptrs)
        if null:
            P[null] = ctypes.c_void_p(None)
        rc = getattr(lib, ref64.ENTRY[self.kernel])(*_arglist(self.kernel, self.case, P, shape), _lib.stream_ptr(self.acc.device))
        torch.cuda.synchronize()
        return rc

    def results(self):
        c = self.case
        acc = self.acc.cpu().numpy()
        assert acc[2] == 12345.0
        out = dict(sum=float(acc[0]), count=float(acc[1]), grad=self.grad.numpy(c['pred'].shape))
        if self.grad_logb is not None:
            out['grad_logb'] = self.grad_logb.numpy(c['logb'].shape)
        return out


def _grad_check(got, want, gbound, kept, skip, ill, what):
    """-> (worst error / bound, worst absolute error, elements whose derived bound exceeds the cap and stands alone)."""
    assert np.isfinite(got).all(), f'{what}: an element was not written, or is not finite'
    assert np.all(got[~kept & ~skip] == 0.0), f'{what}: gradient on a dropped or unlabelled element'
    got64 = got.astype(np.float64)
    err = np.abs(got64 - want)
    cap = 1e-5 * np.abs(want) + 1e-7
    tol = np.where(ill, gbound, np.minimum(gbound, cap))
    ok = ~skip
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err > 0, err / tol, 0.0)[ok]
    worst = float(ratio.max(initial=0.0))
    bad = ok & (err > tol)
    assert not bad.any(), (what, int(bad.sum()), 'worst error / bound', worst, 'at', np.argwhere(bad)[:3].tolist(),
                           got64[bad][:3].tolist(), want[bad][:3].tolist(), tol[bad][:3].tolist())
    return worst, float(err[ok].max(initial=0.0)), int((ill & ok & (gbound > cap)).sum())


def _pairs(x, grad_shape):
    return x if x.shape == grad_shape else np.repeat(x, 2, axis=1)


def _check(case, ref, call, preload=(0.0, 0.0)):
    k = case['kernel']
    got = call.results()
    assert call.grad.guards_intact() and (call.grad_logb is None or call.grad_logb.guards_intact()), 'write outside the gradient'
    v, units, blocks, m, w = ref64.geometry(k, case['n'], case['cp'], case['hw'], call.aligned)
    nb = int(ref.borderline.sum())
    gs = case['pred'].shape
    fig = _grad_check(got['grad'], ref.chk, ref.chk_bound, _pairs(ref.kept, gs), _pairs(ref.borderline, gs), _pairs(ref.ill, gs), 'grad')
    if k == 'laplace':
        fig_b = _grad_check(got['grad_logb'], ref.grad_logb, ref.gbound_logb, ref.kept, ref.borderline, ref.ill_logb, 'grad_logb')
        fig = (max(fig[0], fig_b[0]), max(fig[1], fig_b[1]), fig[2] + fig_b[2])
    sum_err = abs(got['sum'] - (preload[0] + ref.sum))
    bound = (m + 6 + w) * U * (ref.abs_sum + abs(preload[0]))
    if nb:                                        # a borderline element may enter or leave the sum: its term is about the margin
        mg = float(case.get('margin', 0))
        bound += nb * 2 * (np.sqrt(mg) if case.get('sqrt_re') else mg)
    rel = sum_err / ref.abs_sum if ref.abs_sum else 0.0
    print(f"FP64FIG {k} {case['name']} {ref64.vtag({x: case[x] for x in ('gamma', 'tau', 'margin', 'sqrt_re') if x in case})} "
          f"V={v} units={units} m={m} W={w} kept={ref.count} borderline={nb} cont={int(ref.cont.sum())} uncapped={fig[2]} grad_err/bound={fig[0]:.3f} "
          f"grad_abs_err={fig[1]:.3e} sum_rel_err={rel:.3e} sum_bound_rel={(m + 6 + w) * U:.3e} exact={int(case['exact'])}")
    if k not in ('focal', 'l2'):
        assert got['count'] == int(got['count']) and abs(got['count'] - preload[1] - ref.count) <= nb, (got['count'], ref.count, nb)
    else:
        assert got['count'] == preload[1], 'the l2 / focal kernels have no count'
    if case['exact']:
        assert got['sum'] == preload[0] + ref.sum, (got['sum'], ref.sum)
        assert np.array_equal(got['grad'].astype(np.float64), ref.grad)
    assert sum_err <= bound, (got['sum'], ref.sum, sum_err, bound)
    return got


CASES = [c for k in ref64.KERNELS for c in ref64.case_list(k)] + [c for k in ref64.EXACT for c in ref64.exact_case_list(k)]


@pytest.mark.parametrize("cid,shape,variant,seed,flags", CASES, ids=[c[0] for c in CASES])
def test_kernel_matches_float64(cid, shape, variant, seed, flags):
    case = ref64.make_case(cid.split('-')[0], shape, variant, seed, **flags)
    ref = ref64.reference(case)
    call = _Call(case)
    assert call.aligned
    _lib.check(call.run())
    got = _check(case, ref, call)
    if case['name'] == 'masked_image':
        assert np.all(got['grad'][1] == 0.0)
    if case['name'] == 'no_finite_target':
        assert got['sum'] == 0.0 and got['count'] == 0.0 and np.all(got['grad'] == 0.0)


MISALIGNED = [(k, vi, name) for k in ref64.KERNELS for vi in range(len(ref64.variants(k))) for name in FLOAT_OPERANDS[k] + ('mask',)]


@pytest.mark.parametrize("kernel,vi,name", MISALIGNED, ids=[f'{k}-{ref64.vtag(ref64.variants(k)[vi])}-{name}' for k, vi, name in MISALIGNED])
def test_misaligned_operand_gives_the_same_gradients(kernel, vi, name):
    """hw % 4 == 0 with one base pointer off the 16-byte grid (a float operand by one float, the mask by one byte, views into
    larger allocations): l2, masked l1, vector l1 and laplace fall back to their V = 1 kernels, and every gradient bit equals the
    aligned call's.  focal and offset l1 have no 16-byte path; they are here so that every entry point has seen such pointers."""
    case = ref64.make_case(kernel, ('misaligned', 2, 3, 1024), ref64.variants(kernel)[vi], 7000 + vi)
    ref = ref64.reference(case)
    base = _Call(case)
    assert base.aligned
    _lib.check(base.run())
    want = _check(case, ref, base)
    call = _Call(case, offs={name: 1})
    assert not call.aligned
    _lib.check(call.run())
    got = _check(case, ref, call)
    for key in ('grad', 'grad_logb'):
        if key in want:
            assert np.array_equal(got[key].view(np.int32), want[key].view(np.int32)), key
    assert got['count'] == want['count']


@pytest.mark.parametrize("kernel", ref64.KERNELS)
def test_accumulators_are_added_to(kernel):
    """sum / sum_count are added to with atomics, never overwritten (include/og_decoder.h); the count is a float."""
    variant = ref64.variants(kernel)[-1]
    case = ref64.make_case(kernel, ('preload', 2, 3, 1000), variant, 7100)
    call = _Call(case, preload=(3.5, 7.0))
    _lib.check(call.run())
    _check(case, ref64.reference(case), call, preload=(3.5, 7.0))
    if kernel in ref64.EXACT:
        cid, shape, variant, seed, flags = ref64.exact_case_list(kernel)[2]
        case = ref64.make_case(kernel, shape, variant, seed, **flags)
        pre = (1024 * case['quantum'], 5.0)
        call = _Call(case, preload=pre)
        _lib.check(call.run())
        _check(case, ref64.reference(case), call, preload=pre)        # exact: == old + sum


@pytest.mark.parametrize("kernel", ref64.KERNELS)
def test_refusals_launch_nothing(kernel):
    """A null pointer for each pointer argument, N, C or hw <= 0, an odd C for the vector kernels: OG_EINVAL, a message naming the
    entry point, and nothing launched -- canary-filled outputs and pre-loaded accumulators unchanged."""
    lib = _lib.load()
    case = ref64.make_case(kernel, ('refusal', 2, 2, 16), ref64.variants(kernel)[0], 7200)
    n, c, hw = case['n'], case['c'], case['hw']
    call = _Call(case, preload=(1.25, 2.0))
    refused = [dict(null=name) for name in call.ptrs]
    refused += [dict(shape=s) for s in ((0, c, hw), (-1, c, hw), (n, 0, hw), (n, -2, hw), (n, c, 0), (n, c, -4))]
    if kernel in ('vector', 'laplace'):
        refused += [dict(shape=(n, 1, hw)), dict(shape=(n, 3, hw))]
    assert len(refused) >= 11
    for kw in refused:
        rc = call.run(**kw)
        msg = lib.og_last_error().decode()
        assert rc == _lib.OG_EINVAL and ref64.ENTRY[kernel] in msg, (kw, rc, msg)
        with pytest.raises(_lib.OgError):
            _lib.check(rc, lib)
        assert call.grad.untouched() and (call.grad_logb is None or call.grad_logb.untouched()), kw
        assert call.acc.cpu().tolist() == [1.25, 2.0, 12345.0], kw
    _lib.check(call.run())                           # and the same staging is accepted as it stands
    assert not call.grad.untouched()


# ---- the autograd wrappers through lossfuncs_factory(..., fused=True) at the training shape ----
BATCH, SIDE = 8, 128
_cache = {}


def _train_inputs():
    if 'inputs' not in _cache:
        _cache['inputs'] = common.inputs(seed=41, n=BATCH, h=SIDE, w=SIDE)
    return _cache['inputs']


def _np3(t):
    a = t.detach().cpu().numpy()
    return a.reshape(a.shape[0], a.shape[1], -1)


def _head_ref(head, choice, sqrt_re, stack):
    """Ref of one head's kernel call on stack `stack` of the training inputs, cached over the 32 combinations."""
    key = (head, choice, bool(sqrt_re) if choice not in ('l2_loss', 'focal_l2_loss') else None, stack)
    if key not in _cache:
        d = _train_inputs()
        mask = d['mask'].numpy().reshape(BATCH, -1).astype(np.uint8)
        pred, gt = _np3(d[head][stack]), _np3(d[{'hm': 'hm_gt', 'bg': 'bg_gt', 'jit': 'jit_gt', 'off': 'off_gt', 'scale': 'scale_gt'}[head]])
        margin = ref64.MARGIN2 if head == 'scale' else ref64.MARGIN
        if choice == 'focal_l2_loss':
            r = ref64.focal_l2(pred, gt, mask, np.float32(losses.TAU), np.float32(losses.GAMMA))
        elif choice == 'l2_loss':
            r = ref64.l2(pred, gt, mask)
        elif head == 'off' and choice in ('offset_l1_loss', 'offset_instance_l1_loss'):
            ps = _np3(d['ps'].expand_as(d['off_gt'])) if choice == 'offset_instance_l1_loss' else np.ones_like(gt)
            r = ref64.offset_l1(pred, gt, ps, mask, margin, sqrt_re)
        elif choice in ('offset_l1_loss', 'scale_l1_loss'):
            r = ref64.masked_l1(pred, gt, mask, margin, sqrt_re)
        elif choice == 'vector_l1_loss':
            r = ref64.vector_l1(pred, gt, mask, margin, sqrt_re)
        else:
            r = ref64.laplace(pred, gt, _np3(d['spread'][stack]), mask, margin, sqrt_re)
        kernel = {'focal_l2_loss': 'focal', 'l2_loss': 'l2', 'vector_l1_loss': 'vector', 'offset_laplace_loss': 'laplace'}.get(
            choice, 'offset' if head == 'off' else 'ml1')
        cp = pred.shape[1] // (2 if kernel in ('vector', 'laplace') else 1)
        v, units, blocks, m, w = ref64.geometry(kernel, BATCH, cp, SIDE * SIDE)
        assert int(r.borderline.sum()) <= 4
        _cache[key] = (r, (m + 6 + w) * U * r.abs_sum, kernel in ('focal', 'l2'))
    return _cache[key]


@pytest.mark.parametrize("hmp,jit,off,sqrt_re", common.COMBOS, ids=[common.tag(*c) for c in common.COMBOS])
def test_fused_criterion_matches_float64_at_the_training_shape(hmp, jit, off, sqrt_re):
    """Batch 8, 128 x 128 maps, every head, two stacks: each of the five losses and every gradient against the restatement scaled as
    the criterion scales -- stack weight, 1 / batch, 1 / (1 + count), lambda (4 u more for those float32 scalings)."""
    _dev()
    d = _train_inputs()
    val, grads = common.run(losses, d, hmp, jit, off, sqrt_re, fused=True, device='cuda:0')
    ws = [w / sum(common.STACK_WEIGHTS) for w in common.STACK_WEIGHTS]
    heads = [('hm', hmp), ('bg', hmp), ('jit', jit), ('off', off), ('scale', 'scale_l1_loss')]
    worst = {}
    for (head, choice), lam, got_val in zip(heads, common.LAMBDAS, val):
        want_val = tol_val = 0.0
        for s, w in enumerate(ws):
            r, sum_bound, is_sum = _head_ref(head, choice, sqrt_re, s)
            nb = int(r.borderline.sum())
            denom = 1.0 if is_sum else 1.0 + r.count
            k = w / BATCH / denom
            want_val += r.sum * k
            tol_val += (sum_bound + (0.0 if is_sum else nb * (r.sum / denom + 1.0))) * k
            g = grads[head][s].reshape(r.grad.shape)
            ratio, _, n_ill = _grad_check(g, r.chk * (k * lam), (r.chk_bound + (4 * U + nb / denom) * np.abs(r.chk)) * (k * lam),
                                          _pairs(r.kept, g.shape), _pairs(r.borderline, g.shape), _pairs(r.ill, g.shape), f'{head}[{s}]')
            worst[head] = max(worst.get(head, 0.0), ratio)
            if choice == 'offset_laplace_loss':
                gb = grads['spread'][s].reshape(r.grad_logb.shape)
                _grad_check(gb, r.grad_logb * (k * lam), (r.gbound_logb + (4 * U + nb / denom) * np.abs(r.grad_logb)) * (k * lam),
                            r.kept, r.borderline, r.ill_logb, f'spread[{s}]')
        tol_val += 8 * U * abs(want_val)
        print(f'FP64FIG criterion {common.tag(hmp, jit, off, sqrt_re)} {head} value {got_val:.8g} float64 {want_val:.10g} '
              f'rel_err={abs(got_val - want_val) / max(abs(want_val), 1e-300):.3e} grad_err/bound={worst[head]:.3f}')
        assert abs(float(got_val) - want_val) <= tol_val, (head, got_val, want_val, tol_val)


def _hm_criterion():
    return losses.lossfuncs_factory(['hmp', 'omp'], 2, [1, 1], 'focal_l2_loss', 'offset_l1_loss', 'offset_l1_loss', 'scale_l1_loss',
                                    True, fused=True)


def _small(dev):
    rng = ref64.synth.HashRng(77)
    n, c, h, w = 2, 4, 16, 16
    t = lambda lo, hi, ch=c: torch.from_numpy(rng.uniform(n * ch * h * w, lo, hi).reshape(n, ch, h, w).astype(np.float32)).to(dev)  # noqa: E731
    gt = t(-4, 4)
    gt[t(0, 1) > 0.7] = float('inf')
    return t(-4, 4), gt, t(0, 1, 1) > 0.2


@pytest.mark.parametrize("form", ['bfloat16', 'channels_last', 'view', 'float16'])
def test_wrapper_gradient_has_the_dtype_and_shape_of_the_prediction(form):
    """Predictions as under torch.autocast (bf16 / fp16), channels-last, or a non-contiguous view: the gradient has the
    prediction's dtype and shape and is the float32 kernel gradient times g / denom, rounded once to that dtype."""
    dev = _dev()
    base, gt, mask = _small(dev)
    if form in ('bfloat16', 'float16'):
        pred = base.to(getattr(torch, form))
    elif form == 'channels_last':
        pred = base.contiguous(memory_format=torch.channels_last)
    else:
        pred = torch.cat([base, base], dim=3)[..., ::2]
        assert not pred.is_contiguous()
    pred = pred.detach().requires_grad_(True)
    crit = _hm_criterion()[1]
    out = crit(([pred, pred.detach()], [[], []], [[], []]), gt, None, None, mask)[0]
    out.backward()
    assert pred.grad.dtype == pred.dtype and pred.grad.shape == pred.shape
    # the kernel itself on what the wrapper hands it: float32, contiguous
    lib = _lib.load()
    p32 = pred.detach().float().contiguous()
    acc, g32 = torch.zeros(2, device=dev), torch.empty_like(p32)
    m8 = mask.to(torch.uint8).contiguous()
    _lib.check(lib.og_offset_l1_loss_f32(_lib.ptr(p32), _lib.ptr(gt), _lib.ptr(torch.ones_like(gt)), _lib.ptr(m8), 2, 4, 256,
                                         losses.MARGIN, 1, _lib.ptr(acc), _lib.ptr(g32), _lib.stream_ptr(dev)), lib)
    denom = 1.0 + acc[1]
    upstream = torch.tensor(0.5 / 2, device=dev)                   # stack weight 1 / 2, batch 2: exact in float32
    want = (g32 * (upstream / denom)).to(pred.dtype)
    assert float(acc[1]) > 100 and torch.equal(pred.grad, want)
    exact = g32.double() * (0.25 / float(denom))
    half_ulp = {'bfloat16': 2.0 ** -8, 'float16': 2.0 ** -11}.get(form, 2.0 ** -24)
    err = (pred.grad.double() - exact).abs()
    assert bool((err <= (half_ulp + 3 * U) * exact.abs() + (2.0 ** -25 if form == 'float16' else 1e-30)).all())   # fp16 subnormals
    assert bool((pred.grad[(~torch.isfinite(gt)) | ~mask.expand_as(gt)] == 0).all())


def test_second_backward_accumulates_exactly_twice():
    dev = _dev()
    base, gt, mask = _small(dev)
    hm_gt = (gt.clamp(0, 1) * torch.isfinite(gt)).nan_to_num(0.0)
    preds = {k: base.clone().requires_grad_(True) for k in ('hm', 'off')}
    crits = _hm_criterion()
    l_hm = crits[0](([preds['hm'], preds['hm']], [[], []], [[], []]), hm_gt, None, None, mask)[0]
    l_off = crits[1](([preds['off'], preds['off']], [[], []], [[], []]), gt, None, None, mask)[0]
    loss = l_hm + 100.0 * l_off
    loss.backward(retain_graph=True)
    first = {k: p.grad.clone() for k, p in preds.items()}
    loss.backward()
    for k, p in preds.items():
        assert bool((first[k] != 0).any()) and torch.equal(p.grad, 2 * first[k]), k
