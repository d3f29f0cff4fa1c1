"""Every conv entry point of include/og_decoder.h, bit for bit, on exactly representable operands (tests/conv_exact.py): small
integers in, bias / residual on a coarse binary grid, so every product and every partial sum in any order is exact in fp32 and the
only inexact step is the final round-to-nearest-even.  The expected tensor is unique: the assertion is torch.equal, nothing else.

A dropped or mis-addressed tap, channel, halo pixel or K slice, a wrong rounding mode, an extra rounding, an element left unwritten
(the outputs start as NaN) or a ticket / slab not back at rest (every launch runs twice) fails the comparison.

CASES is the table the parametrisation is built from: the shapes tests/test_gpu_backbone.py uses for the entry point, edge shapes
(each asserted supported by the kernel's own query first -- the pointwise kernels, the heads and the stem have no query: their return
code is the answer), and the shapes the strict fp16 engine launches at four input sizes; test_engine_launches_are_all_in_the_table
records those launches and keeps the table complete when the routing thresholds of models/engine.py move.

RANGE_CASES x RANGE_MODES (test_*_range) run the same bodies with the operands scaled by powers of two to the ends of the 16-bit range
(conv_exact.REGIMES): fp16 subnormal weights, subnormal activations, outputs in the subnormal range, outputs beyond 65504; bf16 far
outside fp16's exponents.  Still torch.equal against the one expected tensor; flushed_reference and saturated(expected) appear in a
failure's message only, to name its kind."""
import ctypes as C
import zlib

import pytest
import torch

import conv_exact as cx
import test_gpu_backbone as tb
from offsetguided_amd import _lib, models

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
SKIP_RELU = ((True, 1), (False, 0), (False, 1), (True, 0))               # (residual operand, ReLU): all four
BIAS_SKIP_RELU = ((False, False, 0), (True, True, 1), (True, False, 1), (True, True, 0))      # og_conv1x1_tiled_*: bias may be null


def _proj_explicit(s):
    n, h, w, cin, cout, cin2, st2 = s
    return (n, h, w, cin, cout) + ((h, w) if st2 == 1 else (2 * h - 1, 2 * w)) + (cin2, st2)


# family -> [shape tuples]; the shape tuple is also what an engine launch is reduced to (_record_key)
CASES = {
    # (N, H, W, Cin, Cout): split-K kernel, 3x3 stride 1; M tiles of 64 pixels (128 from M = 2048 on)
    'conv3x3': tb.CONV3X3_SHAPES + [
        (1, 1, 1, 64, 64), (1, 2, 3, 64, 128), (1, 3, 1, 128, 64), (1, 1, 2, 512, 512),          # H, W of 1 / 2 / 3; channel range
        (1, 5, 13, 64, 64), (1, 8, 8, 64, 64),                                                   # M = 65, 64 (63: 3x7x9 above)
        (1, 23, 89, 64, 64), (2, 32, 32, 64, 128), (1, 3, 683, 64, 64)],                         # M = 2047 | 2048 | 2049: 128-pixel tiles
    # (N, Hin, Win, Cin, Cout, ksize, stride)
    'conv2d': tb.CONV2D_SHAPES + [s for s in tb.CONV2D_F16_SHAPES if s not in tb.CONV2D_SHAPES] + [
        (1, 1, 1, 64, 64, 3, 2), (1, 2, 3, 128, 64, 1, 2), (1, 3, 2, 64, 64, 3, 1), (1, 3, 3, 512, 512, 1, 1),
        (1, 9, 15, 64, 128, 3, 2), (1, 16, 8, 128, 128, 1, 1), (2, 65, 63, 64, 64, 3, 2), (1, 45, 46, 128, 64, 1, 1)],
    # (N, H, W, Cin, Cout, H2, W2, Cin2, stride2): 3x3 stride 1 + the 1x1 projection along K
    'conv2d_proj': [_proj_explicit(s) for s in tb.CONV2D_PROJ_SHAPES] + [
        (1, 1, 1, 64, 64, 1, 1, 64, 1), (1, 2, 3, 64, 128, 3, 5, 128, 2), (1, 3, 1, 512, 512, 6, 2, 512, 2),
        (1, 5, 13, 128, 64, 5, 13, 64, 1), (2, 32, 32, 64, 64, 64, 64, 64, 2), (1, 23, 89, 64, 128, 23, 89, 128, 1)],
    # (N, Hin, Win, Cin, Cout, stride, (H2, W2, Cin2, stride2) | None)
    'conv_band': tb.BAND_SHAPES + [
        (1, 1, 1, 64, 16, 1, None), (1, 2, 3, 96, 16, 1, None), (1, 3, 2, 512, 512, 1, None), (1, 1, 1, 64, 16, 2, None),
        (1, 5, 7, 64, 32, 2, None), (1, 2, 112, 64, 16, 1, None), (1, 40, 40, 64, 32, 1, None), (1, 3, 111, 64, 16, 2, None),
        (1, 3, 4, 128, 64, 1, (5, 7, 64, 2)), (1, 1, 1, 512, 16, 1, (1, 1, 512, 1)), (1, 15, 17, 64, 16, 1, None),
        (1, 16, 16, 64, 16, 1, None), (1, 17, 15, 64, 16, 2, None)],
    # (N, H, W, Cin, Cout): 16x16 tiles, 40x4 tiles (W == 40), 20x4 tiles (W == 20); K split where few tiles
    'conv3x3_tiled': tb.CONV3X3_TILED_SHAPES + [
        (8, 160, 160, 256, 256),                                                                  # (the repeat test's full-size layer)
        (1, 16, 32, 64, 128), (1, 32, 16, 64, 128), (1, 16, 16, 512, 512), (1, 4, 40, 128, 128), (1, 4, 40, 192, 128),
        (1, 8, 40, 384, 256), (1, 4, 20, 64, 128), (1, 4, 20, 128, 128), (1, 8, 20, 512, 128), (16, 20, 20, 384, 384)],
    'conv3x3_tiled_up2': tb.CONV3X3_TILED_UP2_SHAPES + [
        (1, 16, 16, 64, 128), (1, 16, 16, 512, 512), (1, 4, 40, 192, 128), (1, 4, 40, 128, 128), (1, 4, 20, 128, 128),
        (1, 4, 20, 64, 128), (1, 32, 16, 64, 128)],
    # (N, Hin, Win, Cin, Cout): stride 2, output tiles of 16x8, or 40x2 where the output is 40 wide
    'conv3x3s2_tiled': tb.CONV3X3S2_TILED_SHAPES + [
        (1, 16, 32, 512, 128), (1, 32, 32, 64, 512), (1, 16, 64, 64, 128), (1, 8, 80, 128, 256)],
    # (N, H1, W1, C1, Cout, stride, two inputs): 256-pixel tiles
    'conv1x1_tiled': tb.CONV1X1_TILED_CASES + [
        (1, 1, 1, 64, 128, 1, False), (1, 2, 3, 64, 128, 1, True), (1, 3, 1, 128, 128, 2, False), (1, 15, 17, 64, 128, 1, False),
        (1, 16, 16, 128, 128, 1, True), (1, 1, 257, 64, 256, 1, False), (1, 9, 7, 192, 256, 1, False), (1, 33, 21, 128, 128, 2, False),
        (1, 8, 8, 512, 512, 1, True), (1, 31, 33, 64, 128, 2, True)],
    # (N, H, W, C, head channels): fp32 outputs, no rounding
    'conv1x1_heads': tb.CONV1X1_HEADS_CASES + [
        (1, 1, 1, 64, (17, 38)), (1, 3, 2, 64, (1,)), (1, 15, 17, 192, (17, 38, 17, 2)), (1, 1, 257, 128, (17, 38)),
        (1, 16, 16, 512, (64,))],
    # (N, H, W): 7x7 stride 2 pad 3, 3 -> 128, fp32 NCHW images in
    'stem7x7': tb.STEM_SHAPES + [(1, 32, 64), (1, 64, 32), (3, 32, 32)],
}

# The launches of the strict fp16 engine (use_graph=False, bench_init weights) at ENGINE_SHAPES that are not in the lists above.
ENGINE_SHAPES = [(8, 640, 640), (16, 640, 640), (1, 640, 384), (1, 128, 128)]
ENGINE_CASES = {
    'stem7x7': [
        (1, 128, 128), (1, 640, 384), (16, 640, 640), (8, 640, 640)],
    'conv3x3s2_tiled': [
        (1, 320, 192, 128, 256), (16, 160, 160, 256, 256), (16, 320, 320, 128, 256), (16, 80, 80, 256, 384), (8, 160, 160,
        256, 256), (8, 320, 320, 128, 256), (8, 80, 80, 256, 384)],
    'conv3x3_tiled': [
        (1, 160, 96, 256, 256), (1, 80, 48, 256, 256), (16, 160, 160, 256, 256), (16, 40, 40, 384, 256), (16, 40, 40, 384,
        384), (16, 80, 80, 256, 256), (8, 40, 40, 384, 256), (8, 80, 80, 256, 256)],
    'conv3x3_tiled_up2': [
        (1, 80, 48, 256, 256), (16, 20, 20, 384, 384), (16, 40, 40, 256, 256), (16, 80, 80, 256, 256), (8, 40, 40, 256,
        256), (8, 80, 80, 256, 256)],
    'conv1x1_tiled': [
        (1, 160, 96, 256, 256, 1, True), (1, 32, 32, 256, 256, 1, True), (1, 320, 192, 128, 256, 2, False), (16, 160, 160,
        256, 256, 1, True), (16, 160, 160, 256, 256, 2, False), (16, 320, 320, 128, 256, 2, False), (16, 40, 40, 384, 256,
        1, False), (16, 80, 80, 256, 384, 2, False), (8, 160, 160, 256, 256, 1, True), (8, 160, 160, 256, 256, 2, False),
        (8, 320, 320, 128, 256, 2, False), (8, 40, 40, 384, 256, 1, False), (8, 80, 80, 256, 384, 2, False)],
    'conv1x1_heads': [
        (1, 160, 96, 256, (17, 38)), (1, 32, 32, 256, (17, 38)), (16, 160, 160, 256, (17, 38)), (8, 160, 160, 256, (17, 38))],
    'conv2d': [
        (1, 160, 96, 256, 256, 3, 2), (1, 64, 64, 128, 256, 3, 2), (1, 80, 48, 256, 384, 3, 2), (16, 10, 10, 384, 384, 3,
        1), (16, 10, 10, 384, 512, 3, 2), (16, 20, 20, 384, 384, 3, 2), (16, 40, 40, 384, 384, 3, 2), (16, 5, 5, 512, 384,
        3, 1), (16, 5, 5, 512, 512, 3, 1), (8, 20, 20, 384, 384, 3, 2), (8, 40, 40, 384, 384, 3, 2)],
    'conv2d_proj': [
        (1, 40, 24, 384, 384, 80, 48, 256, 2), (1, 80, 48, 256, 256, 160, 96, 256, 2), (16, 10, 10, 384, 384, 20, 20, 384,
        2), (16, 20, 20, 384, 384, 40, 40, 384, 2), (16, 5, 5, 384, 384, 5, 5, 512, 1), (16, 5, 5, 512, 512, 10, 10, 384,
        2), (8, 10, 10, 384, 384, 20, 20, 384, 2), (8, 20, 20, 384, 384, 40, 40, 384, 2)],
    'conv_band': [
        (1, 1, 1, 384, 384, 1, (1, 1, 512, 1)), (1, 1, 1, 512, 384, 1, None), (1, 1, 1, 512, 512, 1, (2, 2, 384, 2)), (1, 1,
        1, 512, 512, 1, None), (1, 10, 6, 384, 384, 1, (20, 12, 384, 2)), (1, 10, 6, 384, 384, 1, None), (1, 10, 6, 384,
        512, 2, None), (1, 16, 16, 256, 256, 1, (32, 32, 256, 2)), (1, 16, 16, 256, 256, 1, None), (1, 16, 16, 256, 384, 2,
        None), (1, 2, 2, 384, 384, 1, (4, 4, 384, 2)), (1, 2, 2, 384, 384, 1, None), (1, 2, 2, 384, 512, 2, None), (1, 20,
        12, 384, 384, 1, (40, 24, 384, 2)), (1, 20, 12, 384, 384, 1, None), (1, 20, 12, 384, 384, 2, None), (1, 32, 32, 256,
        256, 1, (64, 64, 128, 2)), (1, 32, 32, 256, 256, 1, None), (1, 32, 32, 256, 256, 2, None), (1, 4, 4, 384, 384, 1,
        (8, 8, 384, 2)), (1, 4, 4, 384, 384, 1, None), (1, 4, 4, 384, 384, 2, None), (1, 40, 24, 256, 256, 1, (40, 24, 384,
        1)), (1, 40, 24, 384, 256, 1, None), (1, 40, 24, 384, 384, 1, None), (1, 40, 24, 384, 384, 2, None), (1, 5, 3, 384,
        384, 1, (5, 3, 512, 1)), (1, 5, 3, 512, 384, 1, None), (1, 5, 3, 512, 512, 1, (10, 6, 384, 2)), (1, 5, 3, 512, 512,
        1, None), (1, 8, 8, 256, 256, 1, (8, 8, 384, 1)), (1, 8, 8, 384, 256, 1, None), (1, 8, 8, 384, 384, 1, (16, 16, 256,
        2)), (1, 8, 8, 384, 384, 1, None), (1, 8, 8, 384, 384, 2, None), (8, 5, 5, 512, 384, 1, None)],
}
for _f, _shapes in ENGINE_CASES.items():
    CASES[_f] = CASES[_f] + [s for s in _shapes if s not in CASES[_f]]

# og_conv3x3_tiled_workspace_bytes on both sides of the K-split switch (csrc/conv3x3_tiled.inc: tiled_ksplit)
TILED_SPLIT = [(1, 4, 40, 192, 128), (1, 8, 40, 384, 256), (1, 4, 20, 128, 128), (1, 8, 20, 512, 128), (8, 20, 20, 384, 384)]
TILED_UNSPLIT = [(1, 4, 40, 128, 128), (1, 4, 20, 64, 128), (16, 20, 20, 384, 384), (1, 16, 16, 512, 512), (8, 40, 40, 384, 384)]

_coverage = {}        # (family, dtype) -> [changed, ties, elements, cases]: the rounding really exercised, per case family

# The ends of the 16-bit range (conv_exact.REGIMES): the smallest shapes of CASES that still reach each path -- every one is in
# CASES, so its *_supported query is known to hold -- times the four fp16 regimes and bf16's 'far'.
RANGE_CASES = {
    'conv3x3': [(1, 5, 13, 64, 64), (1, 1, 2, 512, 512), (2, 32, 32, 64, 128)],
    'conv2d': [(1, 9, 15, 64, 128, 3, 2), (1, 3, 3, 512, 512, 1, 1), (1, 16, 8, 128, 128, 1, 1)],
    'conv2d_proj': [(1, 2, 3, 64, 128, 3, 5, 128, 2), (1, 5, 13, 128, 64, 5, 13, 64, 1)],
    'conv_band': [(1, 5, 7, 64, 32, 2, None), (1, 3, 4, 128, 64, 1, (5, 7, 64, 2)), (1, 16, 16, 64, 16, 1, None)],
    # 16x16, 40x4 and 20x4 tiles, both sides of the K split
    'conv3x3_tiled': [(1, 16, 32, 64, 128), (1, 16, 16, 512, 512), (1, 4, 40, 192, 128), (1, 4, 40, 128, 128), (1, 4, 20, 128, 128)],
    'conv3x3_tiled_up2': [(1, 16, 16, 64, 128), (1, 4, 40, 192, 128), (1, 4, 20, 64, 128)],
    'conv3x3s2_tiled': [(1, 16, 32, 512, 128), (1, 8, 80, 128, 256)],
    'conv1x1_tiled': [(1, 15, 17, 64, 128, 1, False), (1, 16, 16, 128, 128, 1, True), (1, 33, 21, 128, 128, 2, False),
                      (1, 8, 8, 512, 512, 1, True)],
    # fp32 outputs: the expectation is the exact value; out_sub and overflow must come out unrounded and finite
    'conv1x1_heads': [(1, 15, 17, 192, (17, 38, 17, 2)), (1, 16, 16, 512, (64,))],
    # (overflow: only the weights and the bias scale, the images are fp32)
    'stem7x7': [(1, 32, 64), (3, 32, 32)],
}
RANGE_MODES = [(torch.float16, 'w_sub'), (torch.float16, 'x_sub'), (torch.float16, 'out_sub'), (torch.float16, 'overflow'),
               (torch.bfloat16, 'far')]
# (family, shape) -> a step on s where the formula's share of infinities leaves 1 .. 50 % (test_conv_exact_cpu.py).  At 1x2 pixels
# only 2 of the 9 taps ever see a pixel: the live K is 1024, not the 4608 the formula is given, and s = 7 left 0 .. 0.1 %; s = 8
# gives 3.7 .. 7.4 %.
OVERFLOW_SHIFT = {('conv3x3', (1, 1, 2, 512, 512)): 1}
_range_coverage = {}  # (family, regime) -> {conv_exact.RANGE_COUNTS, 'cases'}: kept apart from _coverage


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    return torch.device("cuda:0")


def _params(family):
    return [pytest.param(s, id='-'.join(str(v).replace(' ', '') for v in s)) for s in CASES[family]]


def _range_params(family):
    return [pytest.param(s, d, r, id='-'.join(str(v).replace(' ', '') for v in s) + f"-{str(d).split('.')[1]}-{r}")
            for s in RANGE_CASES[family] for d, r in RANGE_MODES]


def _seed(family, shape):
    return zlib.crc32(repr((family, shape)).encode())


def _operands(family, shape, regime, *args, **kw):
    """The operands of one case: those of the default regime (same seed, same draws) scaled into `regime`."""
    return cx.exact_operands(_seed(family, shape), *args, regime=regime, shift=OVERFLOW_SHIFT.get((family, shape), 0),
                             x_fp32=family == 'stem7x7', **kw)


def _cl(t, dev, dtype):
    return t.to(dev).to(dtype).contiguous(memory_format=torch.channels_last)


def _nan_like(n, c, h, w, dev, dtype):
    return torch.full((n, c, h, w), float('nan'), dtype=dtype, device=dev).contiguous(memory_format=torch.channels_last)


def _assert_equal(got, exp, what, kinds=None):
    """kinds (the range regimes): () -> {name: alternative expectation}, evaluated on a mismatch only, for the message alone."""
    if not torch.equal(got, exp):
        raise AssertionError(f'{what}: {cx.describe_mismatch(got, exp)}' + (cx.describe_kind(got, exp, kinds()) if kinds else ''))


def _kinds(regime, expected, flushed):
    """None in the default regime; else what a mismatch is counted against: flushed() and saturated(expected) (fp32 outputs cannot
    saturate: the value rounded to the 16-bit type instead)."""
    if regime is None:
        return None
    if expected.dtype == torch.float32:
        return lambda: {'flushed_reference': flushed(), 'the value rounded to 16 bits': expected.to(cx.REGIME_DTYPE[regime]).float()}
    return lambda: {'flushed_reference': flushed(), 'saturated(expected)': cx.saturated(expected)}


def _cover(family, dtype, v64, last, expected=None, regime=None):
    if regime is not None:
        c = _range_coverage.setdefault((family, regime), dict.fromkeys(cx.RANGE_COUNTS + ('cases',), 0))
        for k, v in cx.range_coverage(v64, dtype, expected).items():
            c[k] += v
        c['cases'] += int(last)
        return
    changed, ties, total = cx.rounding_coverage(v64, dtype, expected)
    c = _coverage.setdefault((family, dtype), [0, 0, 0, 0])
    c[0] += changed
    c[1] += ties
    c[2] += total
    c[3] += int(last)


def _zeros_ws(need, dev):
    assert need > 0
    return torch.zeros(need, dtype=torch.uint8, device=dev)


def _run_twice(launch, make_out, expected, what, kinds=None):
    """Two launches, each into a fresh NaN-filled (or freshly cloned) output; both must equal the expectation: tickets and slabs are
    back at rest after the first."""
    for i in range(2):
        out = make_out()
        launch(out)
        _assert_equal(out, expected, f'{what}, launch {i + 1}', kinds)


def _splitk_case(dev, family, dtype, ops, dims, ws, call, second=None, combos=SKIP_RELU, regime=None):
    """Shared body of the split-K families: dims = (n, ho, wo, cout, stride); call(x, w, bias, skip, out, relu) launches."""
    n, ho, wo, cout, stride = dims
    x, bias = _cl(ops['x'], dev, dtype), ops['bias'].to(dev)
    res = _cl(ops['res'], dev, dtype)
    x2 = _cl(ops['x2'], dev, dtype) if second else None
    wd, w2 = ops['w'].to(dev), ops['w2'].to(dev) if second else None
    st2 = second if second else 1
    base = cx.exact_sum(x, wd, stride=stride, x2=x2, w2=w2, stride2=st2)
    for ci, (use_skip, relu) in enumerate(combos):
        skip = res if use_skip else None
        v64 = cx.apply_epilogue(base, bias, skip, relu)
        _cover(family, dtype, v64, ci == len(combos) - 1, regime=regime)
        exp = cx.round_once(v64, dtype)
        _run_twice(lambda out: call(x, x2, bias, skip, out, relu), lambda: _nan_like(n, cout, ho, wo, dev, dtype), exp,
                   f'skip={use_skip} relu={relu}',
                   _kinds(regime, exp, lambda: cx.flushed_reference(x, wd, bias, skip, relu, stride, x2, w2, st2, dtype)))
    assert ws[:256].count_nonzero().item() == 0                    # the zero page is never written


def _conv3x3_case(dev, shape, dtype, regime=None):
    n, h, w, cin, cout = shape
    lib = _lib.load()
    ops = _operands('conv3x3', shape, regime, n, h, w, cin, cout)
    wt = _cl(ops['w'], dev, dtype)
    ws = _zeros_ws(lib.og_conv3x3_workspace_bytes(n * h * w, cin, cout), dev)
    fn = _lib.lp(lib, 'og_conv3x3', dtype)

    def call(x, x2, bias, skip, out, relu):
        _lib.check(fn(_lib.ptr(x), _lib.ptr(wt), _lib.ptr(bias), _lib.ptr(skip) if skip is not None else None, _lib.ptr(out), n, h, w,
                      cin, cout, relu, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)), lib)
    _splitk_case(dev, 'conv3x3', dtype, ops, (n, h, w, cout, 1), ws, call, regime=regime)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", _params('conv3x3'))
def test_conv3x3_exact(dev, shape, dtype):
    _conv3x3_case(dev, shape, dtype)


@pytest.mark.parametrize("shape,dtype,regime", _range_params('conv3x3'))
def test_conv3x3_range(dev, shape, dtype, regime):
    _conv3x3_case(dev, shape, dtype, regime)


def _conv2d_case(dev, shape, dtype, regime=None):
    n, h, w, cin, cout, k, st = shape
    lib = _lib.load()
    ops = _operands('conv2d', shape, regime, n, h, w, cin, cout, k, st)
    ho, wo = ops['res'].shape[2:]
    wt = _cl(ops['w'], dev, dtype)
    ws = _zeros_ws(lib.og_conv2d_workspace_bytes(n, h, w, cin, cout, k, st), dev)
    fn = _lib.lp(lib, 'og_conv2d', dtype)

    def call(x, x2, bias, skip, out, relu):
        _lib.check(fn(_lib.ptr(x), _lib.ptr(wt), _lib.ptr(bias), _lib.ptr(skip) if skip is not None else None, _lib.ptr(out), n, h, w,
                      cin, cout, k, st, relu, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)), lib)
    _splitk_case(dev, 'conv2d', dtype, ops, (n, ho, wo, cout, st), ws, call, regime=regime)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", _params('conv2d'))
def test_conv2d_exact(dev, shape, dtype):
    _conv2d_case(dev, shape, dtype)


@pytest.mark.parametrize("shape,dtype,regime", _range_params('conv2d'))
def test_conv2d_range(dev, shape, dtype, regime):
    _conv2d_case(dev, shape, dtype, regime)


def _conv2d_proj_case(dev, shape, dtype, regime=None):
    n, h, w, cin, cout, h2, w2, cin2, st2 = shape
    lib = _lib.load()
    ops = _operands('conv2d_proj', shape, regime, n, h, w, cin, cout, second=(h2, w2, cin2))
    w_cat = torch.cat([ops['w'].permute(0, 2, 3, 1).reshape(cout, -1), ops['w2'].reshape(cout, -1)], 1).to(dev).to(dtype).contiguous()
    ws = _zeros_ws(lib.og_conv2d_proj_workspace_bytes(n, h, w, cin, cout, 3, 1, cin2), dev)
    fn = _lib.lp(lib, 'og_conv2d_proj', dtype)

    def call(x, x2, bias, skip, out, relu):
        assert skip is None
        _lib.check(fn(_lib.ptr(x), _lib.ptr(w_cat), _lib.ptr(bias), _lib.ptr(x2), _lib.ptr(out), n, h, w, cin, cout, 3, 1, h2, w2, cin2,
                      st2, relu, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)), lib)
    _splitk_case(dev, 'conv2d_proj', dtype, ops, (n, h, w, cout, 1), ws, call, second=st2, combos=((False, 1), (False, 0)),
                 regime=regime)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", _params('conv2d_proj'))
def test_conv2d_proj_exact(dev, shape, dtype):
    """act(conv3x3(y) + conv1x1(x, stride2) + bias): the projection's weights appended along K, as _Residual.w_cat builds them."""
    _conv2d_proj_case(dev, shape, dtype)


@pytest.mark.parametrize("shape,dtype,regime", _range_params('conv2d_proj'))
def test_conv2d_proj_range(dev, shape, dtype, regime):
    _conv2d_proj_case(dev, shape, dtype, regime)


def _conv_band_case(dev, shape, dtype, regime=None):
    n, h, w, cin, cout, st, proj = shape
    lib = _lib.load()
    h2, w2, c2, st2 = proj if proj is not None else (0, 0, 0, 1)
    assert lib.og_conv_band_supported(n, h, w, cin, cout, st, h2, w2, c2, st2) > 0
    ops = _operands('conv_band', shape, regime, n, h, w, cin, cout, 3, st, second=(h2, w2, c2) if proj else None)
    ho, wo = ops['res'].shape[2:]
    x, bias, res = _cl(ops['x'], dev, dtype), ops['bias'].to(dev), _cl(ops['res'], dev, dtype)
    wt = _cl(ops['w'], dev, dtype)
    x2 = _cl(ops['x2'], dev, dtype) if proj else None
    wp = ops['w2'].to(dev).to(dtype).contiguous() if proj else None
    packed = torch.empty(cout * (9 * cin + c2), dtype=dtype, device=dev)
    _lib.check(lib.og_conv_band_pack_w16(_lib.ptr(wt), _lib.ptr(wp) if proj else None, cin, cout, c2, _lib.ptr(packed),
                                         _lib.stream_ptr(dev)), lib)
    fn = _lib.lp(lib, 'og_conv_band', dtype)
    wd, w2d = ops['w'].to(dev), ops['w2'].to(dev) if proj else None
    base = cx.exact_sum(x, wd, stride=st, x2=x2, w2=w2d, stride2=st2)
    for ci, (use_skip, relu) in enumerate(SKIP_RELU):
        skip = res if use_skip else None
        v64 = cx.apply_epilogue(base, bias, skip, relu)
        _cover('conv_band', dtype, v64, ci == len(SKIP_RELU) - 1, regime=regime)
        exp = cx.round_once(v64, dtype)

        def launch(out):
            _lib.check(fn(_lib.ptr(x), _lib.ptr(packed), _lib.ptr(bias), _lib.ptr(res) if use_skip else None,
                          _lib.ptr(x2) if proj else None, _lib.ptr(out), n, h, w, cin, cout, st, relu, h2, w2, c2, st2,
                          _lib.stream_ptr(dev)), lib)
        _run_twice(launch, lambda: _nan_like(n, cout, ho, wo, dev, dtype), exp, f'skip={use_skip} relu={relu}',
                   _kinds(regime, exp, lambda: cx.flushed_reference(x, wd, bias, skip, relu, st, x2, w2d, st2, dtype)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", _params('conv_band'))
def test_conv_band_exact(dev, shape, dtype):
    _conv_band_case(dev, shape, dtype)


@pytest.mark.parametrize("shape,dtype,regime", _range_params('conv_band'))
def test_conv_band_range(dev, shape, dtype, regime):
    _conv_band_case(dev, shape, dtype, regime)


def _tiled_setup(lib, dev, dtype, family, shape, order, stride, up=False, regime=None):
    n, h, w, cin, cout = shape
    ops = _operands(family, shape, regime, n, h, w, cin, cout, 3, stride, up=up)
    wt = _cl(ops['w'], dev, dtype)
    packed = torch.empty(wt.numel(), dtype=dtype, device=dev)
    _lib.check(lib.og_conv3x3_pack_w16(_lib.ptr(wt), cin, cout, order, _lib.ptr(packed), _lib.stream_ptr(dev)), lib)
    x, bias, res = _cl(ops['x'], dev, dtype), ops['bias'].to(dev), _cl(ops['res'], dev, dtype)
    return ops, packed, x, bias, res, cx.exact_sum(x, ops['w'].to(dev), stride=stride)


def _conv3x3_tiled_case(dev, shape, dtype, regime=None):
    n, h, w, cin, cout = shape
    lib = _lib.load()
    assert lib.og_conv3x3_tiled_supported(n, h, w, cin, cout) > 0
    ops, packed, x, bias, res, base = _tiled_setup(lib, dev, dtype, 'conv3x3_tiled', shape, 0, 1, regime=regime)
    need = lib.og_conv3x3_tiled_workspace_bytes(n, h, w, cin, cout)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev) if need else None
    fn = _lib.lp(lib, 'og_conv3x3_tiled', dtype)
    for ci, (use_skip, relu) in enumerate(SKIP_RELU):
        skip = res if use_skip else None
        v64 = cx.apply_epilogue(base, bias, skip, relu)
        _cover('conv3x3_tiled', dtype, v64, ci == len(SKIP_RELU) - 1, regime=regime)
        exp = cx.round_once(v64, dtype)

        def launch(out):
            _lib.check(fn(_lib.ptr(x), _lib.ptr(packed), _lib.ptr(bias), _lib.ptr(res) if use_skip else None, _lib.ptr(out), n, h, w,
                          cin, cout, relu, _lib.ptr(ws) if need else None, need, _lib.stream_ptr(dev)), lib)
        _run_twice(launch, lambda: _nan_like(n, cout, h, w, dev, dtype), exp, f'skip={use_skip} relu={relu}',
                   _kinds(regime, exp, lambda: cx.flushed_reference(x, ops['w'].to(dev), bias, skip, relu, dtype=dtype)))
    if need:
        assert ws[:256].count_nonzero().item() == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", _params('conv3x3_tiled'))
def test_conv3x3_tiled_exact(dev, shape, dtype):
    _conv3x3_tiled_case(dev, shape, dtype)


@pytest.mark.parametrize("shape,dtype,regime", _range_params('conv3x3_tiled'))
def test_conv3x3_tiled_range(dev, shape, dtype, regime):
    _conv3x3_tiled_case(dev, shape, dtype, regime)


def _conv3x3_tiled_up2_case(dev, shape, dtype, regime=None):
    n, h, w, cin, cout = shape
    lib = _lib.load()
    assert lib.og_conv3x3_tiled_supported(n, h, w, cin, cout) > 0
    ops, packed, x, bias, res, base = _tiled_setup(lib, dev, dtype, 'conv3x3_tiled_up2', shape, 0, 1, up=True, regime=regime)
    up = _cl(ops['up'], dev, dtype)
    need = lib.og_conv3x3_tiled_workspace_bytes(n, h, w, cin, cout)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev) if need else None
    fn = _lib.lp(lib, 'og_conv3x3_tiled_up2', dtype)
    for ci, (use_skip, relu) in enumerate(SKIP_RELU):
        skip = res if use_skip else None
        raw = cx.apply_epilogue(base, bias, skip, relu)
        low = cx.round_once(raw, dtype)                                                                      # first rounding
        v64 = up.double() + low.double().repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        exp = cx.round_once(v64, dtype)                                                                      # second rounding
        # coverage: the expectation against the never-rounded up + nearest2x(raw) -- either rounding point may have moved it
        _cover('conv3x3_tiled_up2', dtype, up.double() + raw.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3),
               ci == len(SKIP_RELU) - 1, expected=exp, regime=regime)

        def launch(out):
            _lib.check(fn(_lib.ptr(x), _lib.ptr(packed), _lib.ptr(bias), _lib.ptr(res) if use_skip else None, _lib.ptr(out), n, h, w,
                          cin, cout, relu, _lib.ptr(ws) if need else None, need, _lib.stream_ptr(dev)), lib)
        _run_twice(launch, lambda: up.clone(memory_format=torch.preserve_format), exp, f'skip={use_skip} relu={relu}',
                   _kinds(regime, exp, lambda: cx.flushed_reference(x, ops['w'].to(dev), bias, skip, relu, dtype=dtype, up=up)))
    if need:
        assert ws[:256].count_nonzero().item() == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", _params('conv3x3_tiled_up2'))
def test_conv3x3_tiled_up2_exact(dev, shape, dtype):
    """up += nearest_x2(round(act(conv + bias + skip))), rounded again: the kernel's contract has two rounding points
    (include/og_decoder.h: og_conv3x3_tiled_up2_bf16; models/hourglass_104.py:170-176) and the expectation restates them one by one."""
    _conv3x3_tiled_up2_case(dev, shape, dtype)


@pytest.mark.parametrize("shape,dtype,regime", _range_params('conv3x3_tiled_up2'))
def test_conv3x3_tiled_up2_range(dev, shape, dtype, regime):
    _conv3x3_tiled_up2_case(dev, shape, dtype, regime)


def _conv3x3s2_tiled_case(dev, shape, dtype, regime=None):
    n, h, w, cin, cout = shape
    lib = _lib.load()
    assert lib.og_conv3x3s2_tiled_supported(n, h, w, cin, cout) > 0
    ops, packed, x, bias, res, base = _tiled_setup(lib, dev, dtype, 'conv3x3s2_tiled', shape, 1, 2, regime=regime)
    fn = _lib.lp(lib, 'og_conv3x3s2_tiled', dtype)
    for ci, (use_skip, relu) in enumerate(SKIP_RELU):
        skip = res if use_skip else None
        v64 = cx.apply_epilogue(base, bias, skip, relu)
        _cover('conv3x3s2_tiled', dtype, v64, ci == len(SKIP_RELU) - 1, regime=regime)
        exp = cx.round_once(v64, dtype)

        def launch(out):
            _lib.check(fn(_lib.ptr(x), _lib.ptr(packed), _lib.ptr(bias), _lib.ptr(res) if use_skip else None, _lib.ptr(out), n, h, w,
                          cin, cout, relu, _lib.stream_ptr(dev)), lib)
        _run_twice(launch, lambda: _nan_like(n, cout, h // 2, w // 2, dev, dtype), exp, f'skip={use_skip} relu={relu}',
                   _kinds(regime, exp, lambda: cx.flushed_reference(x, ops['w'].to(dev), bias, skip, relu, 2, dtype=dtype)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", _params('conv3x3s2_tiled'))
def test_conv3x3s2_tiled_exact(dev, shape, dtype):
    _conv3x3s2_tiled_case(dev, shape, dtype)


@pytest.mark.parametrize("shape,dtype,regime", _range_params('conv3x3s2_tiled'))
def test_conv3x3s2_tiled_range(dev, shape, dtype, regime):
    _conv3x3s2_tiled_case(dev, shape, dtype, regime)


def _conv1x1_tiled_case(dev, shape, dtype, regime=None):
    n, h, w, cin, cout, st, two = shape
    lib = _lib.load()
    ops = _operands('conv1x1_tiled', shape, regime, n, h, w, cin, cout, 1, st, second=(h, w, cin) if two else None)
    ho, wo = ops['res'].shape[2:]
    x1, bias, res = _cl(ops['x'], dev, dtype), ops['bias'].to(dev), _cl(ops['res'], dev, dtype)
    x2 = _cl(ops['x2'], dev, dtype) if two else None
    w1 = ops['w'].reshape(cout, cin)
    wcat = (torch.cat([w1, ops['w2']], 1) if two else w1).to(dev).to(dtype).contiguous()
    packed = torch.empty(wcat.numel(), dtype=dtype, device=dev)
    _lib.check(lib.og_conv3x3_pack_w16(_lib.ptr(wcat), wcat.shape[1], cout, 2, _lib.ptr(packed), _lib.stream_ptr(dev)), lib)
    fn = _lib.lp(lib, 'og_conv1x1_tiled', dtype)
    wd, w2d = ops['w'].to(dev), ops['w2'].to(dev) if two else None
    base = cx.exact_sum(x1, wd, stride=st, x2=x2, w2=w2d, stride2=st)
    for ci, (use_bias, use_skip, relu) in enumerate(BIAS_SKIP_RELU):
        b, skip = bias if use_bias else None, res if use_skip else None
        v64 = cx.apply_epilogue(base, b, skip, relu)
        _cover('conv1x1_tiled', dtype, v64, ci == len(BIAS_SKIP_RELU) - 1, regime=regime)
        exp = cx.round_once(v64, dtype)

        def launch(out):
            _lib.check(fn(_lib.ptr(x1), cin, h, w, st, _lib.ptr(x2) if two else None, cin if two else 0, h, w, st, _lib.ptr(packed),
                          _lib.ptr(bias) if use_bias else None, _lib.ptr(res) if use_skip else None, _lib.ptr(out), n, ho, wo, cout,
                          relu, _lib.stream_ptr(dev)), lib)
        _run_twice(launch, lambda: _nan_like(n, cout, ho, wo, dev, dtype), exp, f'bias={use_bias} skip={use_skip} relu={relu}',
                   _kinds(regime, exp, lambda: cx.flushed_reference(x1, wd, b, skip, relu, st, x2, w2d, st, dtype)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", _params('conv1x1_tiled'))
def test_conv1x1_tiled_exact(dev, shape, dtype):
    """One input (stride 1 / 2) and two inputs concatenated along K, with and without bias (null: the raw projection)."""
    _conv1x1_tiled_case(dev, shape, dtype)


@pytest.mark.parametrize("shape,dtype,regime", _range_params('conv1x1_tiled'))
def test_conv1x1_tiled_range(dev, shape, dtype, regime):
    _conv1x1_tiled_case(dev, shape, dtype, regime)


def _conv1x1_heads_case(dev, shape, dtype, regime=None):
    n, h, w, cin, heads = shape
    lib = _lib.load()
    tot = sum(heads)
    cout = (tot + 63) // 64 * 64
    ops = _operands('conv1x1_heads', shape, regime, n, h, w, cin, tot, 1)
    x = _cl(ops['x'], dev, dtype)
    wt = torch.zeros(cout, cin, dtype=dtype, device=dev)
    wt[:tot] = ops['w'].reshape(tot, cin).to(dev).to(dtype)
    bias = torch.zeros(cout, device=dev)
    bias[:tot] = ops['bias'].to(dev)
    packed = torch.empty(wt.numel(), dtype=dtype, device=dev)
    _lib.check(lib.og_conv3x3_pack_w16(_lib.ptr(wt), cin, cout, 3, _lib.ptr(packed), _lib.stream_ptr(dev)), lib)
    exp = cx.exact_reference(x, ops['w'].to(dev), ops['bias'].to(dev), dtype=torch.float32)
    assert bool(exp.isfinite().all())
    if regime is not None:
        _cover('conv1x1_heads', dtype, exp.double(), True, regime=regime)      # (what a rounding to 16 bits WOULD do to the values)
    kinds = _kinds(regime, exp, lambda: cx.flushed_reference(x, ops['w'].to(dev), ops['bias'].to(dev), dtype=torch.float32))
    chans = (C.c_int * len(heads))(*heads)
    for i in range(2):
        outs = [torch.full((n, c, h, w), float('nan'), device=dev) for c in heads]
        ptrs = (C.c_void_p * len(heads))(*[o.data_ptr() for o in outs])
        _lib.check(_lib.lp(lib, 'og_conv1x1_heads', dtype)(_lib.ptr(x), cin, _lib.ptr(packed), _lib.ptr(bias), n, h, w, cout, len(heads),
                                                         chans, ptrs, _lib.stream_ptr(dev)), lib)
        c0 = 0
        for hi, (o, c) in enumerate(zip(outs, heads)):
            _assert_equal(o, exp[:, c0:c0 + c], f'head {hi}, launch {i + 1}',
                          kinds and (lambda: {k: v[:, c0:c0 + c] for k, v in kinds().items()}))
            c0 += c


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", _params('conv1x1_heads'))
def test_conv1x1_heads_exact(dev, shape, dtype):
    """fp32 NCHW outputs written from the fp32 accumulators, bias added in fp32: the expectation is the exact value itself."""
    _conv1x1_heads_case(dev, shape, dtype)


@pytest.mark.parametrize("shape,dtype,regime", _range_params('conv1x1_heads'))
def test_conv1x1_heads_range(dev, shape, dtype, regime):
    """The exact value in fp32 again: below 2^-14 (out_sub) and beyond 65504 (overflow) it comes out unrounded and finite."""
    _conv1x1_heads_case(dev, shape, dtype, regime)


def _stem7x7_case(dev, shape, dtype, regime=None):
    n, h, w = shape
    lib = _lib.load()
    ops = _operands('stem7x7', shape, regime, n, h, w, 3, 128, 7, 2)
    x, bias = ops['x'].to(dev).contiguous(), ops['bias'].to(dev)
    packed = torch.zeros((128, 7, 8, 4), device=dev)
    packed[:, :, :7, :3] = ops['w'].to(dev).permute(0, 2, 3, 1)
    packed = packed.to(dtype).contiguous()
    fn = _lib.lp(lib, 'og_stem7x7', dtype)
    base = cx.exact_sum(x, ops['w'].to(dev), stride=2)
    assert tuple(base.shape) == (n, 128, h // 2, w // 2)
    for relu in (1, 0):
        v64 = cx.apply_epilogue(base, bias, None, relu)
        _cover('stem7x7', dtype, v64, relu == 0, regime=regime)
        exp = cx.round_once(v64, dtype)
        _run_twice(lambda out: _lib.check(fn(_lib.ptr(x), _lib.ptr(packed), _lib.ptr(bias), _lib.ptr(out), n, h, w, relu,
                                             _lib.stream_ptr(dev)), lib),
                   lambda: _nan_like(n, 128, h // 2, w // 2, dev, dtype), exp, f'relu={relu}',
                   _kinds(regime, exp, lambda: cx.flushed_reference(x, ops['w'].to(dev), bias, None, relu, 2, dtype=dtype)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", _params('stem7x7'))
def test_stem7x7_exact(dev, shape, dtype):
    """fp32 NCHW integer images in (their conversion to 16 bits is exact), weights packed [cout][ky][8 taps][4 channels] as the engine does."""
    _stem7x7_case(dev, shape, dtype)


@pytest.mark.parametrize("shape,dtype,regime", _range_params('stem7x7'))
def test_stem7x7_range(dev, shape, dtype, regime):
    """The fp32 images are of the regime's size (x_sub: the kernel's own conversion must produce the subnormals); under overflow only
    the weights and the bias are scaled."""
    _stem7x7_case(dev, shape, dtype, regime)


def test_tiled_edge_shapes_sit_on_both_sides_of_the_k_split():
    lib = _lib.load()
    for s in TILED_SPLIT:
        assert s in CASES['conv3x3_tiled'] and lib.og_conv3x3_tiled_workspace_bytes(*s) > 0, s
    for s in TILED_UNSPLIT:
        assert s in CASES['conv3x3_tiled'] and lib.og_conv3x3_tiled_supported(*s) > 0 and lib.og_conv3x3_tiled_workspace_bytes(*s) == 0, s


def test_rounding_is_exercised_in_every_family():
    """Per case family and dtype, over the expected tensors of the cases above (all epilogue combinations; ReLU zeros count as
    unrounded): at least 25 % of the expected outputs differ from their unrounded value and at least one is an exact tie.  A family
    is judged once all of its cases have run (a -k selection judges none); og_conv1x1_heads_* writes fp32 and rounds nothing."""
    judged = 0
    for (family, dtype), (changed, ties, total, cases) in sorted(_coverage.items(), key=str):
        print(f'{family} {dtype}: {changed / total:.1%} of {total} expected outputs rounded, {ties} exact ties, {cases} cases')
        if cases == len(CASES[family]):
            judged += 1
            assert changed >= 0.25 * total and ties >= 1, (family, dtype, changed / total, ties)
    assert judged == 0 or judged == 2 * (len(CASES) - 1), f'{judged} (family, dtype) pairs judged'


@pytest.mark.parametrize("dtype,regime", RANGE_MODES)
def test_device_casts_keep_the_regime_operands(dev, dtype, regime):
    """What _cl does to a regime's operands on the device -- fp32 -> 16 bits, channels-last -- is what the CPU cast does: subnormals
    and all.  (A cast that flushed them would make a correct kernel look like flushed_reference.)"""
    ops = cx.exact_operands(1, 1, 5, 7, 64, 32, second=(5, 7, 64), up=True, regime=regime)
    for name, t in ops.items():
        if name != 'bias':
            src = t if t.dim() == 4 else t[:, :, None, None]
            assert torch.equal(_cl(src, dev, dtype).cpu(), src.to(dtype)) and torch.equal(src.to(dtype).float(), src), name


def test_range_regimes_are_exercised_in_every_family():
    """Per case family and regime, over the expected tensors of the range cases above (all epilogue combinations): the elements
    compared, the subnormals, exact ties and infinities among them -- printed; a family whose cases have all run must show the
    regime's point (og_conv1x1_heads_* writes fp32: its counts are of what a rounding to 16 bits would do to its expected values).
    Kept apart from _coverage: the 25 % condition above is about the default regime alone."""
    judged = 0
    for (family, regime), c in sorted(_range_coverage.items()):
        print(f"{family} {regime}: {c['elements']} elements compared, {c['subnormals']} subnormals, {c['ties']} ties, {c['infs']} infs, "
              f"{c['nonties']} other roundings, {c['to_min_normal']} rounded up to the smallest normal, {c['cases']} cases")
        if c['cases'] == len(RANGE_CASES[family]):
            judged += 1
            assert c['elements'] > 0 and (regime != 'out_sub' or c['subnormals'] >= 64 * c['cases']) and (regime != 'overflow' or c['infs'] > 0)
    assert judged in (0, len(RANGE_CASES) * len(RANGE_MODES)), f'{judged} (family, regime) pairs judged'


# ---------------------------------------------------------------------------------------- the engine's launches are in the table
def _table_keys():
    keys = set()
    for family, shapes in CASES.items():
        combos = {'conv2d_proj': [(False, 1), (False, 0)], 'conv1x1_tiled': BIAS_SKIP_RELU, 'conv1x1_heads': [()],
                  'stem7x7': [(1,), (0,)]}.get(family, SKIP_RELU)
        keys.update((family, tuple(s), tuple(c)) for s in shapes for c in combos)
    return keys


@pytest.mark.parametrize("shape", ENGINE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_engine_launches_are_all_in_the_table(dev, shape, monkeypatch):
    """Every conv launch of the strict fp16 engine (use_graph=False, bench_init weights) at this input shape -- entry point, integer
    arguments, which optional operands are present -- is one of the cases this file runs exactly."""
    records = set()
    assert cx.record_launches(monkeypatch, records.add) == 2 * len(CASES)
    model = tb._bench_model(5, dev)
    eng = models.InferenceEngine(model, *shape, device=dev, dtype=torch.float16, use_graph=False)
    assert eng.strict
    eng.forward_raw(torch.randn(shape[0], 3, shape[1], shape[2], device=dev))
    torch.cuda.synchronize(dev)
    assert eng.torch_conv_calls == [] and len(records) > 10
    missing = sorted(records - _table_keys(), key=str)
    assert not missing, f'{len(missing)} engine launches at {shape} are not in CASES:\n' + '\n'.join(map(str, missing))
