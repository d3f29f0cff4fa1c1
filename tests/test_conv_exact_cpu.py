"""tests/conv_exact.py held honest on the CPU: the fp64 tap-sum reference against F.conv2d, the precondition that makes the operands
exact, what the exact comparison sees that the relative-error gate of tests/test_gpu_backbone.py cannot, and how much of the
expected output the final rounding really changes."""
import pytest
import torch
import torch.nn.functional as F

import conv_exact as cx

DTYPES = [torch.bfloat16, torch.float16]

# (n, h, w, cin, cout, k, stride, second (h2, w2, cin2, stride2) | None)
FORMS = [(2, 5, 7, 16, 8, 1, 1, None), (1, 6, 9, 8, 16, 1, 2, None), (2, 7, 5, 8, 8, 3, 1, None), (1, 8, 8, 16, 8, 3, 2, None),
         (1, 9, 7, 8, 8, 3, 2, None), (1, 1, 1, 8, 8, 3, 1, None), (1, 2, 3, 8, 8, 3, 1, None), (2, 32, 32, 3, 16, 7, 2, None),
         (1, 31, 33, 3, 8, 7, 2, None), (2, 5, 6, 8, 16, 3, 1, (5, 6, 24, 1)), (1, 4, 3, 8, 8, 3, 1, (7, 6, 16, 2)),
         (1, 4, 3, 8, 8, 3, 1, (8, 5, 16, 2)), (2, 6, 5, 16, 8, 1, 1, (6, 5, 16, 1)), (1, 7, 9, 8, 8, 1, 2, (7, 9, 8, 2))]


def _torch_sum(ops, k, stride, st2, dtype=torch.float64):
    ref = F.conv2d(ops['x'].to(dtype), ops['w'].to(dtype), None, stride, k // 2)
    if 'x2' in ops:
        ref = ref + F.conv2d(ops['x2'].to(dtype), ops['w2'].to(dtype)[:, :, None, None], None, st2, 0)[:, :, :ref.shape[2], :ref.shape[3]]
    return ref


@pytest.mark.parametrize("form", FORMS, ids=str)
def test_reference_equals_torch_fp64_and_fp32(form):
    """exact_sum == F.conv2d in fp64, bit for bit, for every form the kernels compute; the fp32 torch result equals the fp64 one on
    these operands (the precondition does what it claims); every epilogue and both output types; up2 with its two roundings."""
    n, h, w, cin, cout, k, stride, second = form
    st2 = second[3] if second else 1
    ops = cx.exact_operands(7, n, h, w, cin, cout, k, stride, second=second[:3] if second else None, up=True)
    ref = _torch_sum(ops, k, stride, st2)
    got = cx.exact_sum(ops['x'], ops['w'], stride=stride, x2=ops.get('x2'), w2=ops.get('w2'), stride2=st2)
    assert got.dtype == torch.float64 and torch.equal(got, ref)
    assert torch.equal(_torch_sum(ops, k, stride, st2, torch.float32).double(), ref)
    for use_bias, use_res, relu in ((True, True, True), (True, False, False), (False, False, False), (True, True, False)):
        full = ref + (ops['bias'].double().view(1, -1, 1, 1) if use_bias else 0) + (ops['res'].double() if use_res else 0)
        full = F.relu(full) if relu else full
        assert torch.equal(full.float().double(), full)
        assert torch.equal(cx.exact_reference(ops['x'], ops['w'], ops['bias'] if use_bias else None, ops['res'] if use_res else None, relu,
                                              stride, ops.get('x2'), ops.get('w2'), st2, dtype=torch.float32).double(), full)
        for dtype in DTYPES:
            exp = cx.exact_reference(ops['x'], ops['w'], ops['bias'] if use_bias else None, ops['res'] if use_res else None, relu,
                                     stride, ops.get('x2'), ops.get('w2'), st2, dtype=dtype)
            assert exp.dtype == dtype and torch.equal(exp, full.float().to(dtype))
            up2 = cx.exact_reference(ops['x'], ops['w'], ops['bias'] if use_bias else None, ops['res'] if use_res else None, relu,
                                     stride, ops.get('x2'), ops.get('w2'), st2, dtype=dtype, up=ops['up'])
            low = F.interpolate(full.float().to(dtype).float(), scale_factor=2, mode='nearest')
            assert torch.equal(up2, (ops['up'] + low).to(dtype))                     # two rounding points, one by one


def test_operands_lie_on_their_grids():
    ops = cx.exact_operands(3, 2, 6, 5, 64, 32, 3, 1, second=(6, 5, 64), up=True)
    assert ops['x'].abs().max() == 3 and ops['w'].abs().max() == 2 and torch.equal(ops['x'], ops['x'].round())
    assert torch.equal(ops['w'], ops['w'].round()) and torch.equal(ops['w2'], ops['w2'].round()) and ops['w2'].abs().max() == 2
    assert ops['bias'].abs().max().item() <= 4 and torch.equal(ops['bias'] * 64, (ops['bias'] * 64).round())
    for name, lim in (('res', 8), ('up', 8), ('x2', 3)):
        t = ops[name]
        assert t.abs().max().item() == lim and torch.equal(t * 8, (t * 8).round())
        for dtype in DTYPES:
            assert torch.equal(t.to(dtype).float(), t)                               # exact in both 16-bit types
    for dtype in DTYPES:
        assert torch.equal(ops['x'].to(dtype).float(), ops['x']) and torch.equal(ops['w'].to(dtype).float(), ops['w'])


def test_precondition_fires_for_a_shape_that_is_too_large():
    assert cx.check_precondition(9 * 512 + 512) == 30732                             # the largest K of the network
    assert cx.check_precondition(5459) == 32766
    with pytest.raises(AssertionError, match='2\\^15'):
        cx.check_precondition(5460)
    with pytest.raises(AssertionError, match='2\\^15'):
        cx.exact_operands(0, 1, 2, 2, 640, 8, 3, 1)                                  # K = 5760
    with pytest.raises(AssertionError, match='2\\^15'):
        cx.exact_operands(0, 1, 2, 2, 512, 8, 3, 1, second=(2, 2, 1024))             # the second input counts


def test_describe_mismatch_locates_the_first_difference():
    exp = torch.arange(2 * 3 * 20 * 18, dtype=torch.float32).view(2, 3, 20, 18).to(torch.bfloat16)
    assert cx.describe_mismatch(exp.clone(), exp) == ''
    got = exp.clone()
    got[1, 2, 17, 0] = float('nan')
    got[1, 2, 18, 5] += 64
    msg = cx.describe_mismatch(got, exp)
    assert msg.startswith('2 of 2160 elements differ; first at (n=1, c=2, y=17, x=0): got nan, expected') and 'border pixel of 20x18' in msg
    assert 'y % 16 = 1, x % 16 = 0' in msg
    got = exp.clone()
    got[0, 1, 16, 16] += 64
    assert 'interior pixel' in cx.describe_mismatch(got, exp) and 'y % 16 = 0, x % 16 = 0' in cx.describe_mismatch(got, exp)


def test_rounding_coverage_counts_changes_and_ties():
    v = torch.tensor([1.0, 257.0, 258.0, 259.0, 0.0, -385.0, 2049.0, 4098.0], dtype=torch.float64)
    assert cx.rounding_coverage(v, torch.bfloat16) == (5, 3, 8)      # 257 -> 256 (tie), 258 -> 258, 259 -> 260 (tie), -385 (tie), 2049, 4098
    assert cx.rounding_coverage(v, torch.float16) == (2, 2, 8)       # 2049 -> 2048 (tie), 4098 -> 4096 (tie)


# ------------------------------------------------------------------------------------------------------------------ sensitivity
def _truncate(v32, dtype):
    """Round toward zero to the 16-bit type instead of RNE: where RNE went away from zero, one step back in the bit pattern."""
    r = v32.to(dtype)
    away = r.float().abs() > v32.abs()
    r = torch.where(away, (r.view(torch.int16) - 1).view(dtype), r)
    assert bool((r.float().abs() <= v32.abs()).all())
    return r


def _outputs(x, w, bias, res, dtype, bias_fine=None):
    """name -> (subtly wrong output, correct output) of relu(conv3x3(x) + bias + res), from fp64 sums of the given operands (any
    values).  bias_fine: the bias of the 'bias rounded first' pair (one that the 16-bit type cannot hold; default: bias)."""
    conv = cx.exact_sum(x, w)
    b, r = bias.double().view(1, -1, 1, 1), res.double()
    fin = lambda v: torch.relu(v).float().to(dtype)          # noqa: E731
    good = fin(conv + b + r)
    n0, y0, x0 = (int(i) for i in (x[:, 0, 1:-1, 1:-1] != 0).nonzero()[0])
    one_tap = conv.clone()
    one_tap[n0, :, y0 + 1, x0 + 1] -= x[n0, 0, y0 + 1, x0 + 1].double() * w[:, 0, 1, 1].double()      # centre tap, channel 0, one pixel
    halo = conv.clone()                                       # outputs of column 16 read column 15 (the left halo of a 16-wide tile) as 0
    for ky in range(3):
        rows = F.pad(x[0, :8, :, 15].double(), (1, 1))[:, ky:ky + x.shape[2]]     # (8, H): rows y + ky - 1
        halo[0, :, :, 16] -= torch.einsum('ch,oc->oh', rows, w[:, :8, ky, 0].double())
    nan_fill = good.clone()
    nan_fill[1, 5, 7, 9] = float('nan')
    bf = bias if bias_fine is None else bias_fine
    return good, {
        'truncation instead of RNE': (_truncate(torch.relu(conv + b + r).float(), dtype), good),
        'residual added after a 16-bit rounding of conv + bias': (fin((conv + b).float().to(dtype).double() + r), good),
        'bias rounded to 16 bits first': (fin(conv + bf.to(dtype).double().view(1, -1, 1, 1) + r), fin(conv + bf.double().view(1, -1, 1, 1) + r)),
        'one tap of one input channel dropped at one output pixel': (fin(one_tap + b + r), good),
        'one halo column read as zero for one 8-channel group': (fin(halo + b + r), good),
        'one output element left at its NaN fill': (nan_fill, good)}


# what the gate of tests/test_gpu_backbone.py says to each corruption on that file's own data: the dtypes whose gate it fails too
OLD_GATE_CATCHES = {'truncation instead of RNE': (), 'residual added after a 16-bit rounding of conv + bias': (),
                    'bias rounded to 16 bits first': (), 'one tap of one input channel dropped at one output pixel': (torch.float16,),
                    'one halo column read as zero for one 8-channel group': DTYPES, 'one output element left at its NaN fill': DTYPES}


@pytest.mark.parametrize("dtype", DTYPES, ids=['bf16', 'fp16'])
def test_exact_comparison_sees_what_the_relative_gate_misses(dtype):
    """Six corruptions of the output of relu(conv3x3 + bias + residual) at (2, 20, 20, 384, 384), computed on the reference alone.
    On the exact operands every one fails torch.equal.  On the Gaussian data of test_gpu_backbone.py (same seed and scaling as
    test_conv3x3_matches_torch / test_conv3x3_tiled_kernel_matches_torch) the old metric max|out - ref| / max|ref| against torch's fp32
    convolution, gate 6e-3 (bf16) / 1e-3 (fp16), measured:

        corruption                                                  bf16      fp16
        none (correct RNE output)                                   2.37e-3   2.97e-4  passes
        truncation instead of RNE                                   4.75e-3   5.95e-4  passes: missed
        residual added after a 16-bit rounding of conv + bias       3.55e-3   4.46e-4  passes: missed
        bias rounded to 16 bits first                               2.37e-3   2.98e-4  passes: missed
        one tap of one input channel dropped at one output pixel    3.11e-3   2.87e-3  bf16 passes: missed; fp16 caught
        one halo column read as zero for one 8-channel group        5.64e-2   5.63e-2  caught
        one output element left at its NaN fill                     nan       nan      caught (nan <= gate is False)

    The first three (and the dropped tap in bf16) pass the old gate; the rest are the gross kind it does catch and are listed as caught
    in OLD_GATE_CATCHES, not asserted missed.  'bias rounded to 16 bits first' needs a bias the 16-bit type cannot hold: every k / 64 with
    |k| <= 256 has 8 significant bits and is exact in bf16 and fp16, so with the operands of the GPU file that one corruption changes
    nothing; its pair is computed with a bias on k / 256 (bf16) or, on the first 32 input channels, k / 4096 (fp16), both still exact in
    fp32 next to the sum (check_precondition counts the bits)."""
    n, h, w, cin, cout = 2, 20, 20, 384, 384
    tol = 6e-3 if dtype == torch.bfloat16 else 1e-3
    ops = cx.exact_operands(11, n, h, w, cin, cout)
    # a bias that the 16-bit type cannot hold, still exact in fp32 next to the sum: k / 256 (10 bits > bf16's 8; K = 3456: 15 + 8 = 23
    # bits); fp16 holds 11 bits, so its pair is computed on the first 32 input channels (K = 288: |sum| < 2^11) with a bias on k / 4096
    fine = cx.exact_operands(12, n, h, w, cin, cout, bias_grid=256)['bias']
    good, wrong = _outputs(ops['x'], ops['w'], ops['bias'], ops['res'], dtype, bias_fine=fine)
    if dtype == torch.float16:
        fine = cx.exact_operands(12, n, h, w, 32, cout, bias_grid=4096)['bias']
        wrong['bias rounded to 16 bits first'] = _outputs(ops['x'][:, :32], ops['w'][:, :32], ops['bias'], ops['res'], dtype, fine)[1][
            'bias rounded to 16 bits first']
    assert not torch.equal(fine.to(dtype).float(), fine)
    assert torch.equal(good, cx.exact_reference(ops['x'], ops['w'], ops['bias'], ops['res'], True, dtype=dtype))
    for name, (out, right) in wrong.items():
        assert not torch.equal(out, right), f'{name}: the exact comparison does not see it'
        assert cx.describe_mismatch(out, right) != ''
    # the old test's data and metric
    g = torch.Generator(device='cpu').manual_seed(h * 1000 + cin)
    x = torch.randn(n, cin, h, w, generator=g).to(dtype)
    wt = (torch.randn(cout, cin, 3, 3, generator=g) * (1.0 / (9 * cin)) ** 0.5).to(dtype)
    bias = torch.randn(cout, generator=g) * 0.1
    skip = torch.randn(n, cout, h, w, generator=g).to(dtype)
    ref = F.relu(F.conv2d(x.float(), wt.float(), bias, 1, 1) + skip.float())
    metric = lambda out: ((out.float() - ref).abs().max() / ref.abs().max()).item()      # noqa: E731
    good, wrong = _outputs(x.float(), wt.float(), bias, skip.float(), dtype)
    print(f'\nold metric, {dtype}, gate {tol}: correct output {metric(good):.2e}')
    assert metric(good) <= tol
    assert set(wrong) == set(OLD_GATE_CATCHES)
    for name, (out, _) in wrong.items():
        err = metric(out)
        passes = err <= tol
        print(f'  {name}: {err:.2e} -> {"passes the old gate" if passes else "caught by the old gate"}')
        assert passes == (dtype not in OLD_GATE_CATCHES[name]), f'{name}: old metric {err} against gate {tol}'


# ------------------------------------------------------------------------------------------------------------ rounding coverage
def _case(family, shape, regime=None):
    """One GPU case of tests/test_gpu_conv_exact.py on the CPU: (operands, stride, stride2, [(bias?, skip?, relu)] as that file runs
    them) -- same seed, same regime, same epilogue combinations."""
    import test_gpu_conv_exact as t
    k, st, second, st2, up = 3, 1, None, 1, False
    if family == 'stem7x7':
        n, h, w = shape
        cin, cout, k, st = 3, 128, 7, 2
    elif family == 'conv1x1_heads':
        n, h, w, cin, heads = shape
        cout, k = sum(heads), 1
    elif family == 'conv2d':
        n, h, w, cin, cout, k, st = shape
    elif family == 'conv2d_proj':
        n, h, w, cin, cout, h2, w2, c2, st2 = shape
        second = (h2, w2, c2)
    elif family == 'conv_band':
        n, h, w, cin, cout, st, proj = shape
        if proj:
            second, st2 = proj[:3], proj[3]
    elif family == 'conv1x1_tiled':
        n, h, w, cin, cout, st, two = shape
        k, st2, second = 1, st, ((h, w, cin) if two else None)
    else:
        n, h, w, cin, cout = shape
        st, up = (2 if family == 'conv3x3s2_tiled' else 1), family == 'conv3x3_tiled_up2'
    ops = t._operands(family, shape, regime, n, h, w, cin, cout, k, st, second=second, up=up)
    combos = {'stem7x7': [(True, False, 1), (True, False, 0)], 'conv1x1_heads': [(True, False, 0)], 'conv1x1_tiled': t.BIAS_SKIP_RELU,
              'conv2d_proj': [(True, False, 1), (True, False, 0)]}.get(family, [(True, s, r) for s, r in t.SKIP_RELU])
    return ops, st, st2, combos


def _family_values(family, shape):
    """The unrounded fp64 values behind every expected tensor of one GPU case (tests/test_gpu_conv_exact.py: same operands, same
    epilogue combinations); for up2 the values of the SECOND rounding, per dtype."""
    ops, st, st2, combos = _case(family, shape)
    base = cx.exact_sum(ops['x'], ops['w'], stride=st, x2=ops.get('x2'), w2=ops.get('w2'), stride2=st2)
    vals = [cx.apply_epilogue(base, ops['bias'] if b else None, ops['res'] if s else None, r) for b, s, r in combos]
    if 'up' not in ops:
        return lambda dtype: [(v, None) for v in vals]
    x2 = lambda v: v.repeat_interleave(2, 2).repeat_interleave(2, 3)          # noqa: E731
    return lambda dtype: [(ops['up'].double() + x2(v), cx.round_once(ops['up'].double() + x2(cx.round_once(v, dtype).double()), dtype))
                          for v in vals]


def _macs(family, shape):
    if family == 'stem7x7':
        return shape[0] * shape[1] * shape[2] // 4 * 147 * 128
    n, h, w, cin, cout = shape[:5]
    k = {'conv2d': shape[5] if family == 'conv2d' else 0, 'conv1x1_tiled': 1}.get(family, 3)
    return n * h * w * cin * cout * k * k


@pytest.mark.parametrize("family", ['conv3x3', 'conv2d', 'conv2d_proj', 'conv_band', 'conv3x3_tiled', 'conv3x3_tiled_up2',
                                    'conv3x3s2_tiled', 'conv1x1_tiled', 'stem7x7'])
def test_rounding_is_exercised_in_every_family(family):
    """The rounding-coverage condition of the GPU file, on the CPU for its small cases (up to 1e9 multiply-adds each): per case family
    and dtype at least 25 % of the expected outputs differ from their unrounded value and at least one is an exact tie, so the
    rounding step -- mode, ties, double rounding -- is really exercised.  (og_conv1x1_heads_* writes fp32: nothing is rounded.)

    Measured (bf16 / fp16, share of expected outputs the rounding changes; every family has > 10^4 exact ties): conv3x3 73.0 / 59.7 %,
    conv2d 71.7 / 49.7 %, conv2d_proj 73.2 / 60.4 %, conv_band 73.7 / 64.7 %, conv3x3_tiled 73.2 / 61.1 %, conv3x3_tiled_up2 74.2 /
    63.1 %, conv3x3s2_tiled 73.1 / 59.9 %, conv1x1_tiled 52.6 / 30.0 %, stem7x7 70.4 / 40.2 %.  fp16 holds 11 bits: on the 2^-6 grid
    nothing below 32 is rounded, which is why conv_exact draws half of the activations and weights at the ends of their ranges and
    gives every bias an odd numerator (uniform draws and any numerator left the stem at 12.9 % and the pointwise kernel at 13.7 %)."""
    import test_gpu_conv_exact as t
    small = [s for s in t.CASES[family] if _macs(family, s) <= 1e9]
    assert len(small) >= 3
    tot = {d: [0, 0, 0] for d in DTYPES}
    for shape in small:
        values = _family_values(family, shape)
        for d in DTYPES:
            for v, expected in values(d):
                for i, c in enumerate(cx.rounding_coverage(v, d, expected)):
                    tot[d][i] += c
    for d in DTYPES:
        changed, ties, total = tot[d]
        print(f'{family} {d}: {changed / total:.1%} of {total} expected outputs rounded, {ties} exact ties, {len(small)} cases')
        assert changed >= 0.25 * total and ties >= 1, (family, d, changed / total, ties)


# ------------------------------------------------------------------------------------------------ the ends of the 16-bit range
# The conditions that keep the range tests of tests/test_gpu_conv_exact.py (RANGE_CASES x RANGE_MODES) from passing vacuously, on
# the reference alone.  They are conditions on the test data, not measurements of any kernel.
def _range_ids():
    import test_gpu_conv_exact as t
    return [pytest.param(f, *p.values, id=f'{f}-{p.id}') for f in t.RANGE_CASES for p in t._range_params(f)]


_range_cache = {}
# sums of exact_operands(3, 2, 6, 5, 64, 32, 3, 1, second=(6, 5, 64), up=True) as drawn before the function had regimes
DEFAULT_DRAW_SUMS = [-2.0, 98.0, 5.59375, 238.5, -64.5, 73.0, -538.5]


def _range_expectations(family, shape, regime):
    """(operands, [(combo, never-rounded fp64 value, expected tensor, flushed expectation)]) of one range case, as the GPU file builds
    them (og_conv1x1_heads_*: fp32 out, expected = the value; up2: two roundings)."""
    key = (family, shape, regime)
    if key not in _range_cache:
        ops, st, st2, combos = _case(family, shape, regime)
        dtype = cx.REGIME_DTYPE[regime]
        out = torch.float32 if family == 'conv1x1_heads' else dtype
        fops = {k: v if k == 'bias' else cx.flush_operand(v) for k, v in ops.items()}
        base, fbase = (cx.exact_sum(o['x'], o['w'], stride=st, x2=o.get('x2'), w2=o.get('w2'), stride2=st2) for o in (ops, fops))
        x2 = lambda v: v.repeat_interleave(2, 2).repeat_interleave(2, 3)          # noqa: E731
        rows = []
        for b, s, r in combos:
            v, fv = (cx.apply_epilogue(a, o['bias'] if b else None, o['res'] if s else None, r) for a, o in ((base, ops), (fbase, fops)))
            exp, fl = cx.round_once(v, out), cx.round_once(fv, out)
            if 'up' in ops:
                v, exp, fl = (ops['up'].double() + x2(v), cx.round_once(ops['up'].double() + x2(exp.double()), out),
                              cx.round_once(fops['up'].double() + x2(fl.double()), out))
            rows.append(((b, s, r), v, exp, fl))
        b, s, r = combos[-1]                                                        # flushed_reference is what this test computes by hand
        assert torch.equal(rows[-1][3], cx.flushed_reference(ops['x'], ops['w'], ops['bias'] if b else None, ops['res'] if s else None, r,
                                                             st, ops.get('x2'), ops.get('w2'), st2, out, ops.get('up')))
        _range_cache[key] = ops, rows
    return _range_cache[key]


@pytest.mark.parametrize("regime", ['w_sub', 'x_sub', 'out_sub', 'overflow', 'far'])
def test_scaled_reference_equals_torch_fp64(regime):
    """One shape per regime (3x3 stride 1 with a strided second input; the 7x7 stride-2 form): the scaled reference is F.conv2d in
    fp64 bit for bit, and torch's fp32 result equals it -- scaling by powers of two left every product and partial sum exact."""
    for n, h, w, cin, cout, k, stride, second in ((1, 4, 3, 8, 8, 3, 1, (7, 6, 16, 2)), (2, 32, 32, 3, 16, 7, 2, None)):
        st2 = second[3] if second else 1
        ops = cx.exact_operands(7, n, h, w, cin, cout, k, stride, second=second[:3] if second else None, up=True, regime=regime)
        ref = _torch_sum(ops, k, stride, st2)
        got = cx.exact_sum(ops['x'], ops['w'], stride=stride, x2=ops.get('x2'), w2=ops.get('w2'), stride2=st2)
        assert torch.equal(got, ref) and torch.equal(_torch_sum(ops, k, stride, st2, torch.float32).double(), ref)
        full = ref + ops['bias'].double().view(1, -1, 1, 1) + ops['res'].double()
        dtype = cx.REGIME_DTYPE[regime]
        assert torch.equal(cx.exact_reference(ops['x'], ops['w'], ops['bias'], ops['res'], False, stride, ops.get('x2'), ops.get('w2'),
                                              st2, dtype=dtype), full.float().to(dtype))


def test_default_regime_is_unchanged_and_regimes_scale_it():
    """regime=None draws what the function drew before it had regimes (the pinned checksum), and w_sub / far are that draw times
    powers of two."""
    kw = dict(second=(6, 5, 64), up=True)
    ops = cx.exact_operands(3, 2, 6, 5, 64, 32, 3, 1, **kw)
    assert [round(float(ops[k].double().sum()), 6) for k in ('x', 'w', 'bias', 'res', 'x2', 'w2', 'up')] == DEFAULT_DRAW_SUMS
    for regime in ('w_sub', 'far'):
        a, b = cx.REGIMES[regime]
        sc = cx.exact_operands(3, 2, 6, 5, 64, 32, 3, 1, regime=regime, **kw)
        for name, e in (('x', a), ('x2', a), ('w', b), ('w2', b), ('bias', a + b), ('res', a + b), ('up', a + b)):
            assert torch.equal(sc[name].double(), ops[name].double() * 2.0 ** e), (regime, name)
    with pytest.raises(AssertionError, match='does not survive'):                   # the precondition is checked on the tensors themselves
        cx.exact_operands(3, 1, 4, 4, 64, 8, regime='overflow', shift=6)


def test_overflow_exponents_come_from_k_alone():
    assert [sum(cx.overflow_exponents(k)) for k in (64, 147, 576, 4608)] == [10, 10, 9, 7]
    assert cx.overflow_exponents(147, x_fp32=True) == (0, 10) and cx.overflow_exponents(576) == (4, 5)
    assert cx.overflow_exponents(576, shift=-1) == (4, 4)


def test_coverage_counts_in_the_subnormal_range():
    """Spacing 2^-24 below 2^-14: ties and roundings are counted on that spacing, not on 11 bits of the value's own exponent."""
    u = 2.0 ** -24
    v = torch.tensor([3 * u, 2.5 * u, 2.25 * u, 0.5 * u, 1023.5 * u, 1023.75 * u, -1023.75 * u, 0.0, 70000.0, 65519.0],
                     dtype=torch.float64)
    c = cx.range_coverage(v, torch.float16)
    assert c == {'elements': 10, 'subnormals': 3, 'ties': 3, 'nonties': 4, 'infs': 1, 'to_min_normal': 3}
    assert cx.rounding_coverage(v, torch.float16)[:2] == (8, 3)
    e = v.float().half()
    assert torch.equal(cx.saturated(e)[-2:], torch.tensor([65504.0, 65504.0]).half()) and torch.equal(cx.saturated(e)[:-2], e[:-2])
    assert torch.equal(cx.flush_operand(torch.tensor([2.0 ** -14, -2.0 ** -15, 3 * u, 0.0])), torch.tensor([2.0 ** -14, 0.0, 0.0, 0.0]))
    got = e.clone()
    got[0], got[8] = 0.0, 65504.0
    kinds = {'A': torch.zeros(1, 1, 1, 10), 'B': cx.saturated(e).view(1, 1, 1, -1)}
    assert cx.describe_kind(got.view(1, 1, 1, -1), e.view(1, 1, 1, -1), kinds) \
        == '; 1 of the differing elements equal A; 1 of the differing elements equal B'


@pytest.mark.parametrize("family,shape,dtype,regime", _range_ids())
def test_range_case_is_not_vacuous(family, shape, dtype, regime):
    """Per (family, shape, regime) of the GPU table, for EVERY epilogue combination the GPU test runs:

    w_sub / x_sub: every non-zero weight / activation (second input included) is a non-zero fp16 subnormal, and the expected tensor
        differs from flushed_reference in at least half of its elements.
    out_sub: at least 64 non-zero subnormals in the expected tensor; where the combination has a bias, at least 8 exact ties and 8
        roundings off a tie.  (og_conv1x1_tiled_*'s bias-less combination with one input sums integers times 2^-21: every value is
        an fp16 subnormal or a small normal exactly, there is nothing to round -- its subnormals are counted, ties cannot exist.)
        og_conv1x1_heads_* writes fp32: the counts are of what a rounding to fp16 would do to its expected values.
    overflow: between 1 % and 50 % of the expected tensor is +-inf (heads: beyond 65504 and finite), both signs without ReLU, and
        the tensor differs from saturated(expected).
    far: one operand magnitude above 65504 and one non-zero operand below 2^-24."""
    assert dtype == cx.REGIME_DTYPE[regime]
    ops, rows = _range_expectations(family, shape, regime)
    heads = family == 'conv1x1_heads'
    if regime in ('w_sub', 'x_sub'):
        for name in (('w', 'w2') if regime == 'w_sub' else ('x', 'x2')):
            if name in ops:
                t = ops[name][ops[name] != 0]
                assert t.numel() > 0 and bool((t.abs() < cx.F16_MIN_NORMAL).all()) and bool((t.half() != 0).all()), name
    if regime == 'far':
        mags = torch.cat([ops[k].abs().flatten() for k in ops if k != 'bias'])
        assert bool((mags > cx.F16_MAX).any()) and bool(((mags > 0) & (mags < 2.0 ** -24)).any())
    for (b, s, r), v, exp, fl in rows:
        what = f'bias={b} skip={s} relu={r}'
        c = cx.range_coverage(v, dtype, None if heads else exp)
        if regime in ('w_sub', 'x_sub'):
            assert int((exp != fl).sum()) * 2 >= exp.numel(), what
        if regime == 'out_sub':
            assert c['subnormals'] >= 64, (what, c)
            assert not b or (c['ties'] >= 8 and c['nonties'] >= 8), (what, c)
        if regime == 'overflow':
            assert 0.01 * c['elements'] <= c['infs'] <= 0.5 * c['elements'], (what, c['infs'] / c['elements'])
            big = v.float().half() if heads else exp
            assert bool((big == float('inf')).any()) and (r or bool((big == -float('inf')).any())), what
            assert bool(exp.isfinite().all()) if heads else not torch.equal(exp, cx.saturated(exp)), what


@pytest.mark.parametrize("family", ['conv3x3', 'conv2d', 'conv2d_proj', 'conv_band', 'conv3x3_tiled', 'conv3x3_tiled_up2',
                                    'conv3x3s2_tiled', 'conv1x1_tiled', 'stem7x7'])
def test_out_sub_reaches_the_smallest_normal_from_below(family):
    """Per 16-bit output family, over its out_sub cases: at least one expected element rounds UP to 2^-14, the smallest normal, from a
    value below it (a single small case need not hold one; the family does)."""
    import test_gpu_conv_exact as t
    n = sum(cx.range_coverage(v, torch.float16, exp)['to_min_normal']
            for shape in t.RANGE_CASES[family] for _, v, exp, _ in _range_expectations(family, shape, 'out_sub')[1])
    assert n >= 1, family
