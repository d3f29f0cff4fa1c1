"""Exactly representable convolution operands and their unique expected output (tests/test_conv_exact_cpu.py,
tests/test_gpu_conv_exact.py).

Small integer activations and weights (half of them at the ends of their ranges), bias on the 2^-6 grid (odd numerators), residual / second input / `up` operands on the 2^-3 grid: every
product, every partial sum in ANY order (MFMA accumulators, split-K slabs, LDS partial tiles), the bias add and the residual add are
exact in fp32.  What is left is the one final rounding to the output type, which is round-to-nearest-even for a correct kernel
(csrc/lp_dtype.h: f2lp) -- so the expected tensor is unique and the comparison is torch.equal, no tolerance.

The reference is a plain fp64 sum over the k*k taps of a shifted NHWC slice times that tap's (Cin, Cout) matrix; it never calls
torch's convolution (tests/test_conv_exact_cpu.py holds it to F.conv2d in fp64, bit for bit)."""
import math

import torch

X_MAX, W_MAX = 3, 2                      # integer activations in [-3, 3], integer weights in [-2, 2]
BIAS_GRID, BIAS_MAX = 64, 4              # bias = k / 64, k odd, |bias| <= 4 (fp32)
RES_GRID, RES_MAX = 8, 8                 # residual / up = k / 8, |.| <= 8: exact in bf16 (8 significant bits) and fp16 alike
SUM_LIMIT = 1 << 15
MANTISSA_BITS = {torch.bfloat16: 8, torch.float16: 11}      # significant bits, the hidden one included
MIN_ULP_EXP = {torch.bfloat16: -133, torch.float16: -24}    # log2 of the spacing of the subnormals
F16_MIN_NORMAL, F16_MAX = 2.0 ** -14, 65504.0

# Regimes: powers of two (a, b) on the operands.  x, x2 are multiplied by 2^a, w, w2 by 2^b, bias, res and up by 2^t, t = a + b:
# every product and every partial sum of the argument above is the old one times 2^t -- still exact -- but the operands or the
# result now lie at the ends of the 16-bit type's range.  fp16: w_sub (every non-zero weight +-2^-24 or +-2^-23, a subnormal),
# x_sub (every non-zero activation a subnormal), out_sub (normal operands; |v| < 128 rounds into the subnormal range, spacing
# 2^-24 = 2^-3 in units of v), overflow (exponents from the case's K, overflow_exponents).  bf16: far (operand exponents far outside
# fp16's range).
REGIMES = {'w_sub': (10, -24), 'x_sub': (-24, 10), 'out_sub': (-11, -10), 'far': (30, -40)}
REGIME_DTYPE = {'w_sub': torch.float16, 'x_sub': torch.float16, 'out_sub': torch.float16, 'overflow': torch.float16,
                'far': torch.bfloat16}
PRODUCT_VARIANCE = 19.5                  # of one product x * w under _ints: E[x^2] E[w^2] = 6.5 * 3
OUT_SUB_BIAS_GRID = 32


def overflow_exponents(k_total, shift=0, x_fp32=False):
    """(a, b) of the 'overflow' regime from K alone: s = ceil(log2(65504 / (2 sqrt(19.5 K)))) (+ shift), so that 65504 lies between
    one and two standard deviations of the scaled sum and a few per cent of the outputs lie beyond it; a = s // 2, b = s - s // 2.
    x_fp32 (the stem: its images are fp32 and are not scaled): (0, s)."""
    s = math.ceil(math.log2(F16_MAX / (2 * math.sqrt(PRODUCT_VARIANCE * k_total)))) + shift
    return (0, s) if x_fp32 else (s // 2, s - s // 2)


def regime_exponents(regime, k_total=None, shift=0, x_fp32=False):
    if regime is None:
        return 0, 0
    return overflow_exponents(k_total, shift, x_fp32) if regime == 'overflow' else REGIMES[regime]


def worst_case_sum(k_total):
    """Largest |conv + bias + residual| for a reduction over k_total products: 6 K + 4 + 8."""
    return X_MAX * W_MAX * k_total + BIAS_MAX + RES_MAX


def check_precondition(k_total, bias_grid=BIAS_GRID):
    """The bound that makes the exact test valid, from the shape alone: |sum| < 2^15 leaves at most 15 + 6 = 21 significant bits on the
    2^-6 grid -- exact in fp32's 24, in any summation order -- and stays far below fp16's 65504.  (The largest K of the network,
    9 * 512 + 512 = 5120, gives 30 732.)  A shape that breaks it is a mistake in the test: an error, never a skip."""
    worst = worst_case_sum(k_total)
    assert worst < SUM_LIMIT, f'K = {k_total}: worst-case |sum| {worst} >= 2^15, the operands are no longer exact in fp32'
    # (a finer bias grid, tests/test_conv_exact_cpu.py: the same count of significant bits must still fit fp32's 24)
    assert bias_grid >= RES_GRID and (worst * bias_grid).bit_length() <= 24, f'K = {k_total}, bias grid 1/{bias_grid}: more than 24 bits'
    return worst


def _ints(g, shape, lim):
    """Integers in [-lim, lim]: half of the draws uniform over the range, half at its two ends.  The ranges are fixed; the weight on the
    ends is what lets the sums of the small-K kernels (stem: K = 147, pointwise: K from 64) reach the magnitudes at which fp16, with
    11 significant bits, rounds on the 2^-6 grid at all (|v| >= 32) -- the rounding-coverage condition of the tests."""
    uniform = torch.randint(-lim, lim + 1, shape, generator=g).float()
    ends = (torch.randint(0, 2, shape, generator=g).float() * 2 - 1) * lim
    return torch.where(torch.rand(shape, generator=g) < 0.5, ends, uniform)


def _grid(g, shape, grid, lim):
    return torch.randint(-lim * grid, lim * grid + 1, shape, generator=g).float() / grid


def _odd_grid(g, shape, grid, lim):
    """k / grid with k odd, |k / grid| < lim: the lowest bit of the grid is set in every bias, hence in every sum that carries one."""
    return (torch.randint(-lim * grid // 2, lim * grid // 2, shape, generator=g).float() * 2 + 1) / grid


def exact_operands(seed, n, h, w, cin, cout, k=3, stride=1, second=None, up=False, bias_grid=BIAS_GRID, regime=None, shift=0,
                   x_fp32=False):
    """fp32 CPU tensors (NCHW) for one convolution case: x (n,cin,h,w), w (cout,cin,k,k), bias (cout,), res (n,cout,ho,wo) with
    ho = (h + 2 (k // 2) - k) // stride + 1; with second = (h2, w2, cin2): x2 (n,cin2,h2,w2) and w2 (cout,cin2), the operand
    concatenated along K (the residual's 1x1 projection, the junction's second input); with up: up (n,cout,2 ho,2 wo).
    x2 lies on the 2^-3 grid like the residual but within the ACTIVATION range |x2| <= 3: the worst-case sum 6 K + 4 + 8 counts
    every one of the K products, the second input's included, as at most 3 * 2.
    bias_grid: 64 everywhere but in the sensitivity test (every k / 64 with |k| <= 256 has 8 significant bits and is exact in bf16
    and fp16 alike; a bias that a 16-bit rounding would change needs a finer grid, and the precondition then counts its bits).
    regime: None (the tensors above, unscaled) or a name of REGIMES / 'overflow' (shift, x_fp32: overflow_exponents): x, x2 times
    2^a, w, w2 times 2^b, bias, res, up times 2^(a + b).  The draws are those of the default regime but for two operands that
    would fall off the type's grid or miss the regime's point:
      x_sub:    x2 is drawn as integers in [-3, 3] (k / 8 * 2^-24 is no fp16 number);
      out_sub:  the bias is drawn on the plain 2^-5 grid (_grid, any numerator).  The subnormal spacing is 2^-3 in units of v: an
                odd-numerator k / 64 never lands on a tie, and on the 2^-4 grid every inexact value IS a tie (no other rounding
                could occur below |v| = 256); k / 32 gives exact values, ties (k = 2 mod 4) and roundings off a tie (k odd).
    res and up stay on the 2^-3 grid: at t = -21 (out_sub) that is k 2^-24, at t = -14 k 2^-17 -- fp16 numbers by construction.
    Asserted from the tensors themselves: every 16-bit operand survives the regime's type unchanged."""
    cin2 = second[2] if second is not None else 0
    k_total = k * k * cin + cin2
    if regime == 'out_sub':
        assert bias_grid == BIAS_GRID
        bias_grid = OUT_SUB_BIAS_GRID
    check_precondition(k_total, bias_grid)
    g = torch.Generator(device='cpu').manual_seed(seed)
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    draw_bias = _grid if regime == 'out_sub' else _odd_grid
    ops = {'x': _ints(g, (n, cin, h, w), X_MAX), 'w': _ints(g, (cout, cin, k, k), W_MAX),
           'bias': draw_bias(g, (cout,), bias_grid, BIAS_MAX), 'res': _grid(g, (n, cout, ho, wo), RES_GRID, RES_MAX)}
    if second is not None:
        h2, w2, _ = second
        ops['x2'] = _grid(g, (n, cin2, h2, w2), 1 if regime == 'x_sub' else RES_GRID, X_MAX)
        ops['w2'] = _ints(g, (cout, cin2), W_MAX)
    if up:
        ops['up'] = _grid(g, (n, cout, 2 * ho, 2 * wo), RES_GRID, RES_MAX)
    if regime is None:
        return ops
    a, b = regime_exponents(regime, k_total, shift, x_fp32)
    dtype = REGIME_DTYPE[regime]
    for name, t in ops.items():
        e = a if name in ('x', 'x2') else b if name in ('w', 'w2') else a + b
        ops[name] = torch.ldexp(t, torch.tensor(e))
        assert torch.equal(ops[name].double(), torch.ldexp(t.double(), torch.tensor(e))) and bool(ops[name].isfinite().all()), name
        if name != 'bias':                                        # (fp32 on the device; the stem's fp32 images must convert exactly too)
            assert torch.equal(ops[name].to(dtype).float(), ops[name]), f'{regime}: {name} does not survive {dtype}'
    return ops


def exact_sum(x, w, bias=None, res=None, relu=False, stride=1, x2=None, w2=None, stride2=1):
    """act(conv(x, w) (+ conv1x1(x2, w2, stride2)) (+ bias) (+ res)) in fp64, NCHW, unrounded.  x (n,cin,h,w), w (cout,cin,k,k) with
    pad k // 2; on the device of x."""
    n, cin, h, wd = x.shape
    cout, _, k, _ = w.shape
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    xp = torch.zeros((n, h + 2 * pad, wd + 2 * pad, cin), dtype=torch.float64, device=x.device)
    xp[:, pad:pad + h, pad:pad + wd] = x.permute(0, 2, 3, 1).double()
    wt = w.double()
    acc = torch.zeros((n, ho, wo, cout), dtype=torch.float64, device=x.device)
    for ky in range(k):
        for kx in range(k):
            tap = xp[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride]
            acc += tap.reshape(-1, cin).matmul(wt[:, :, ky, kx].t()).view(n, ho, wo, cout)
    if x2 is not None:
        tap = x2.permute(0, 2, 3, 1).double()[:, 0:stride2 * (ho - 1) + 1:stride2, 0:stride2 * (wo - 1) + 1:stride2]
        assert tuple(tap.shape[1:3]) == (ho, wo), 'the second input does not map onto the output'
        acc += tap.reshape(-1, x2.shape[1]).matmul(w2.double().reshape(cout, -1).t()).view(n, ho, wo, cout)
    return apply_epilogue(acc.permute(0, 3, 1, 2), bias, res, relu)


def apply_epilogue(acc64, bias=None, res=None, relu=False):
    """act(acc (+ bias) (+ res)) in fp64 on an NCHW accumulator (one exact_sum serves every epilogue combination of a case)."""
    if bias is not None:
        acc64 = acc64 + bias.double().view(1, -1, 1, 1)
    if res is not None:
        acc64 = acc64 + res.double()
    return torch.relu(acc64) if relu else acc64


def round_once(v64, dtype):
    """The one rounding of a correct kernel: fp64 -> fp32 (exact under the precondition) -> RNE to the 16-bit type."""
    assert torch.equal(v64.float().double(), v64), 'not exact in fp32: the precondition does not hold for these values'
    return v64.float() if dtype == torch.float32 else v64.float().to(dtype)


def exact_reference(x, w, bias=None, res=None, relu=False, stride=1, x2=None, w2=None, stride2=1, dtype=torch.bfloat16, up=None):
    """The unique expected output.  dtype = the kernel's output type; torch.float32 (og_conv1x1_heads_*) = the exact value itself.
    up: the contract of og_conv3x3_tiled_up2_* (include/og_decoder.h, models/hourglass_104.py:170-176) -- the convolution's result is
    rounded to 16 bits, THEN added to `up` at nearest x2 and rounded again: round(up + nearest2x(round(act(conv + bias + skip))))."""
    out = round_once(exact_sum(x, w, bias, res, relu, stride, x2, w2, stride2), dtype)
    if up is not None:
        low = out.double().repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        out = round_once(up.double() + low, dtype)
    return out


def _ulp_scaled(v64, dtype):
    """|v| in units of the spacing of `dtype` at v (the subnormal spacing below the smallest normal)."""
    _, e = torch.frexp(v64.abs())                                   # |v| = m 2^e, m in [0.5, 1)
    ue = (e - MANTISSA_BITS[dtype]).clamp(min=MIN_ULP_EXP[dtype])
    return v64.abs() * torch.pow(torch.tensor(2.0, dtype=torch.float64, device=v64.device), -ue.double())   # (2^133 needs fp64)


def rounding_coverage(v64, dtype, expected=None):
    """(elements whose expected value differs from the unrounded fp64 value v64, exact ties of the rounding of v64 to `dtype`,
    elements).  expected: default the one rounding of v64; og_conv3x3_tiled_up2_* passes its twice-rounded expectation next to the
    never-rounded up + nearest2x(act(conv + bias + skip))."""
    r = (v64.float().to(dtype) if expected is None else expected).double()
    changed = int((r != v64).sum())
    scaled = _ulp_scaled(v64, dtype)
    ties = int(((scaled - scaled.floor()) == 0.5).sum())            # exactly half a unit in the last place: RNE decides
    return changed, ties, v64.numel()


RANGE_COUNTS = ('elements', 'subnormals', 'ties', 'nonties', 'infs', 'to_min_normal')


def range_coverage(v64, dtype, expected=None):
    """RANGE_COUNTS of one expected tensor (default: the one rounding of v64) as a dict: its elements; its non-zero elements below
    the type's smallest normal; exact ties of the rounding of v64; finite elements that the rounding changed off a tie; its
    infinities; elements that rounded to the smallest normal from below."""
    r = (v64.float().to(dtype) if expected is None else expected).double()
    tiny = torch.finfo(dtype).tiny
    scaled = _ulp_scaled(v64, dtype)
    tie = (scaled - scaled.floor()) == 0.5
    counts = (v64.numel(), (r != 0) & (r.abs() < tiny), tie, (r != v64) & r.isfinite() & ~tie, r.isinf(),
              (r.abs() == tiny) & (v64.abs() < tiny))
    return {k: int(c if isinstance(c, int) else c.sum()) for k, c in zip(RANGE_COUNTS, counts)}


def flush_operand(t):
    """A 16-bit operand as a unit that flushes fp16 subnormals reads it: zero below 2^-14."""
    return torch.where(t.abs() < F16_MIN_NORMAL, torch.zeros_like(t), t)


def flushed_reference(x, w, bias=None, res=None, relu=False, stride=1, x2=None, w2=None, stride2=1, dtype=torch.float16, up=None):
    """exact_reference with every 16-bit operand (all but the fp32 bias) of magnitude below 2^-14 set to zero first.  NOT an
    expectation any kernel is held to: a CPU condition (the regime must tell the two apart) and a count in the failure messages."""
    f = lambda t: None if t is None else flush_operand(t)      # noqa: E731
    return exact_reference(f(x), f(w), bias, f(res), relu, stride, f(x2), f(w2), stride2, dtype, f(up))


def saturated(expected):
    """The expectation of a kernel that clamps instead of overflowing: +-inf replaced by +-65504.  As flushed_reference: never a
    passing expectation."""
    return torch.where(expected.isinf(), torch.full_like(expected, F16_MAX) * expected.sign(), expected)


def describe_kind(got, exp, alternatives):
    """', of those N equal NAME' for each (name -> tensor) alternative expectation: what kind of failure a mismatch is."""
    g, e = got.float(), exp.float()
    bad = (g != e) | (g.isnan() != e.isnan())
    return ''.join(f'; {int((bad & (g == alt.float().to(g.device))).sum())} of the differing elements equal {name}'
                   for name, alt in alternatives.items())


def describe_mismatch(got, exp):
    """Assert message for torch.equal(got, exp) on (n, c, y, x) tensors: how many differ, the first one, border or interior, and the
    coordinates modulo 16 (tile and K-split seams show up as a pattern there).  '' when the tensors are equal."""
    if got.shape != exp.shape:
        return f'shape {tuple(got.shape)} != expected {tuple(exp.shape)}'
    g, e = got.float(), exp.float()
    bad = (g != e) | (g.isnan() != e.isnan())
    bad &= ~(g.isnan() & e.isnan())
    count = int(bad.sum())
    if count == 0:
        return ''
    n, c, y, x = (int(i) for i in bad.nonzero()[0])
    _, _, h, w = got.shape
    where = 'border' if y in (0, h - 1) or x in (0, w - 1) else 'interior'
    return (f'{count} of {bad.numel()} elements differ; first at (n={n}, c={c}, y={y}, x={x}): got {g[n, c, y, x].item()!r}, expected '
            f'{e[n, c, y, x].item()!r}; {where} pixel of {h}x{w}; y % 16 = {y % 16}, x % 16 = {x % 16}, c % 16 = {c % 16}')


# ------------------------------------------------------------------------------------------- recording the engine's conv launches
def record_key(name, a):
    """(family, shape tuple as in CASES, epilogue) of one launch: the entry point and its integer arguments; pointers as present / null."""
    has = lambda i: a[i] is not None        # noqa: E731
    if name in ('og_conv3x3_tiled', 'og_conv3x3_tiled_up2', 'og_conv3x3s2_tiled', 'og_conv3x3'):
        return name[3:], tuple(a[5:10]), (has(3), a[10])
    if name == 'og_conv2d':
        return 'conv2d', tuple(a[5:12]), (has(3), a[12])
    if name == 'og_conv2d_proj':
        assert (a[10], a[11]) == (3, 1)
        return 'conv2d_proj', tuple(a[5:10]) + tuple(a[12:16]), (False, a[16])
    if name == 'og_conv_band':
        return 'conv_band', tuple(a[6:12]) + ((tuple(a[13:17]) if has(4) else None),), (has(3), a[12])
    if name == 'og_conv1x1_tiled':
        assert not has(5) or (a[6], a[7], a[8], a[9]) == (a[1], a[2], a[3], a[4])
        assert (a[15], a[16]) == ((a[2] - 1) // a[4] + 1, (a[3] - 1) // a[4] + 1)
        return 'conv1x1_tiled', (a[14], a[2], a[3], a[1], a[17], a[4], has(5)), (has(11), has(12), a[18])
    if name == 'og_conv1x1_heads':
        heads = tuple(a[9][i] for i in range(a[8]))
        assert a[7] == (sum(heads) + 63) // 64 * 64
        return 'conv1x1_heads', (a[4], a[5], a[6], a[1], heads), ()
    if name == 'og_stem7x7':
        return 'stem7x7', tuple(a[4:7]), (a[7],)
    raise AssertionError(f'unknown conv entry point {name}')


def record_launches(monkeypatch, on_launch, extra=()):
    """Wrap every 16-bit conv / stem entry point of the loaded library so that each launch calls on_launch(record_key(...)) first,
    and hold _lib.lp to handing out wrapped functions only (a conv launch that bypassed the recorder fails there).  extra: further
    entry-point stems (both 16-bit twins) or full names, reported as (name, (), ()).  -> the number of conv entry points wrapped."""
    from offsetguided_amd import _lib
    lib = _lib.load()

    def recording(name, fn, conv):
        def call(*a):
            on_launch(record_key(name, a) if conv else (name, (), ()))
            return fn(*a)
        call.records_conv_launch = True
        return call
    launches = [n for n in _lib.SIGNATURES if n.startswith(('og_conv', 'og_stem')) and n.endswith(('_bf16', '_f16'))]
    for name in launches:
        monkeypatch.setattr(lib, name, recording(name.rsplit('_', 1)[0], getattr(lib, name), True))
    for stem in extra:
        for name in ([stem] if stem in _lib.SIGNATURES else [stem + '_bf16', stem + '_f16']):
            monkeypatch.setattr(lib, name, recording(stem, getattr(lib, name), False))
    orig_lp = _lib.lp

    def lp(lib_, stem, dtype):
        fn = orig_lp(lib_, stem, dtype)
        assert not stem.startswith(('og_conv', 'og_stem')) or getattr(fn, 'records_conv_launch', False), stem
        return fn
    monkeypatch.setattr(_lib, 'lp', lp)
    return len(launches)
