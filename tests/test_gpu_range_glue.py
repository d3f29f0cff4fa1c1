"""The glue passes of csrc/epilogue.hip at the ends of the 16-bit range, on hand-built tensors: og_bias_act_*, og_upsample2_add_*,
og_nchw_f32_to_nhwc_* and og_nhwc_*_to_nchw_f32.  No convolution is involved.  Every element is a directed case -- subnormals kept,
+-65504 through unchanged, 60000 + 60000 -> +inf (and the negative twin under ReLU -> 0), a sum exactly on the tie between two
subnormals, a sum that rounds up to the smallest normal 2^-14 -- and each enters once as x, once as skip / low and once through the
fp32 bias.  The bf16 twins get the same kinds at 'far' magnitudes (2^30, 2^-40, the type's largest number).

The expectation is the fp64 sum rounded once.  Every case is chosen so that the kernels' fp32 partial sums (x + bias, then + skip)
are exact (asserted), so the expected tensor is unique and the comparison is torch.equal.  Outputs are NaN-filled or, where the
pass works in place, sit between guard bands that must come back untouched."""
import pytest
import torch

from offsetguided_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 64                      # elements on either side of an in-place operand (128 B: the 16-byte alignment is kept)
PIXELS = 37                     # > the longest column below, odd; 37 * channels / 8 groups end inside a wavefront
U = 2.0 ** -24                  # the spacing of the fp16 subnormals
BIG, SMALL = 2.0 ** 30, 2.0 ** -40
BF_MAX = (2.0 - 2.0 ** -7) * 2.0 ** 127

# bias -> [(x, skip)]: one channel per bias, the pairs down the pixels.  The first eight biases are what an 8-channel launch sees.
F16_TABLE = [
    (0.0, [(3 * U, 0), (0, 3 * U), (-1023 * U, 0), (0, -1023 * U), (U, 2 * U),                    # subnormals kept
           (65504, 0), (0, 65504), (-65504, 0), (0, -65504),                                      # the largest number, unchanged
           (60000, 60000), (-60000, -60000),                                                      # +-inf; 0 under ReLU
           (1023 * U, U),                                                                         # 2^-14 exactly, from two subnormals
           (2050 * U, U), (U, 2050 * U),                                                          # a tie one binade up: 2051 U -> 2052 U
           (65504, 16), (16, 65504), (65504, 15)]),                                               # 65520 ties to inf, 65519 does not
    (0.5 * U, [(2 * U, 0), (0, 2 * U), (3 * U, 0), (0, 3 * U), (U, U), (0, 0), (-2 * U, -U)]),     # ties between two subnormals
    (0.75 * U, [(1023 * U, 0), (0, 1023 * U), (1000 * U, 23 * U), (0, 0)]),                       # 1023.75 U rounds up to 2^-14
    (2.5 * U, [(0, 0), (U, 0), (0, U), (1021 * U, 0), (0, 1021 * U)]),                            # the tie through the bias; 1023.5 U -> 2^-14
    (60000.0, [(60000, 0), (0, 60000), (0, 0), (5504, 0), (0, 5504)]),                            # inf, 60000, 65504
    (-60000.0, [(-60000, 0), (0, -60000), (0, 0)]),
    (3 * U, [(0, 0), (-3 * U, 0), (0, -3 * U), (1020 * U, 0)]),                                   # a subnormal through the bias
    (65504.0, [(0, 0), (-65504, 0), (0, -65504)]),
    (1023.75 * U, [(0, 0)]), (-65504.0, [(0, 0)]), (120000.0, [(0, 0)]), (-120000.0, [(0, 0), (60000, 60000)]),
]
BF16_TABLE = [
    (0.0, [(3 * BIG, 0), (0, 3 * BIG), (3 * SMALL, 0), (0, 3 * SMALL), (256 * BIG, BIG), (BIG, 256 * BIG), (258 * BIG, BIG),
           (512 * BIG, BIG), (256 * SMALL, SMALL), (SMALL, 256 * SMALL), (512 * SMALL, 3 * SMALL),
           (BF_MAX, 0), (0, BF_MAX), (-BF_MAX, 0), (2.0 ** 127, 2.0 ** 127), (-2.0 ** 127, -2.0 ** 127), (BF_MAX, 2.0 ** 119),
           (BF_MAX, 2.0 ** 118)]),
    (BIG, [(256 * BIG, 0), (0, 256 * BIG), (258 * BIG, 0), (512 * BIG, 0), (0, 0), (-BIG, 0)]),
    (SMALL, [(256 * SMALL, 0), (0, 256 * SMALL), (512 * SMALL, 0), (0, 0)]),
    (257 * BIG, [(0, 0)]), (2.0 ** 127, [(2.0 ** 127, 0), (0, 2.0 ** 127), (0, 0)]), (-2.0 ** 127, [(-2.0 ** 127, 0), (0, 0)]),
    (BF_MAX, [(0, 0), (-BF_MAX, 0)]), (2.0 ** 119, [(BF_MAX, 0), (0, BF_MAX)]),
    (3 * SMALL, [(0, 0)]), (513 * SMALL, [(0, 0)]),
]
TABLES = {torch.float16: F16_TABLE, torch.bfloat16: BF16_TABLE}
DTYPES = [torch.float16, torch.bfloat16]
IDS = ['fp16', 'bf16']


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    return torch.device("cuda:0")


def _table(dtype, channels):
    """fp64 CPU tensors x, skip (PIXELS, channels) and bias (channels,): channel c carries entry c % len(table), its pairs cycled
    down the pixels.  x and skip are numbers of `dtype`, the bias of fp32 (asserted)."""
    table = TABLES[dtype]
    assert channels >= 8 and max(len(p) for _, p in table) <= PIXELS
    x, skip = (torch.zeros(PIXELS, channels, dtype=torch.float64) for _ in range(2))
    bias = torch.zeros(channels, dtype=torch.float64)
    for c in range(channels):
        b, pairs = table[c % len(table)]
        bias[c] = b
        for p in range(PIXELS):
            x[p, c], skip[p, c] = pairs[p % len(pairs)]
    for t in (x, skip):
        assert torch.equal(t.float().to(dtype).double(), t)
    assert torch.equal(bias.float().double(), bias)
    return x, skip, bias


def _exact32(v64):
    """A partial sum that the kernel forms in fp32: it must be exact there, or overflow fp32 itself (2^127 + 2^127: inf, and inf in
    the 16-bit type too)."""
    f = v64.float().double()
    assert bool(((f == v64) | (f.isinf() & (v64.abs() >= 2.0 ** 128))).all()), 'a directed case is not exact in fp32'
    return v64


def _guarded(t64, dev, dtype, fill):
    """(buffer, view): t64 as `dtype` on the device between two guard bands of `fill`."""
    buf = torch.full((t64.numel() + 2 * GUARD,), fill, dtype=dtype, device=dev)
    view = buf[GUARD:GUARD + t64.numel()].view(t64.shape)
    view.copy_(t64.float().to(dtype).to(dev))
    return buf, view


def _guards_intact(buf, fill):
    g = torch.cat([buf[:GUARD], buf[-GUARD:]]).float()
    return bool((g == fill).all())


def _describe(got, exp):
    bad = ((got != exp) & ~(got.isnan() & exp.isnan())).nonzero()
    i = tuple(int(v) for v in bad[0])
    return f'{len(bad)} of {exp.numel()} elements differ; first at {i}: got {got[i].item()!r}, expected {exp[i].item()!r}'


def _assert_equal(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype
    assert torch.equal(got, exp), f'{what}: {_describe(got.double().cpu(), exp.double().cpu())}'


@pytest.mark.parametrize("channels", [8, 24])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bias_act_at_the_ends_of_the_range(dev, dtype, channels):
    """x = act(x + bias[c] (+ skip)) in place, all four (skip, ReLU) combinations."""
    lib = _lib.load()
    x64, skip64, bias64 = _table(dtype, channels)
    bias = bias64.float().to(dev)
    skip = skip64.float().to(dtype).to(dev).contiguous()
    fn = _lib.lp(lib, 'og_bias_act', dtype)
    seen = {}
    for use_skip in (True, False):
        v = _exact32(x64 + bias64)
        if use_skip:
            v = _exact32(v + skip64)
        for relu in (0, 1):
            exp = (torch.relu(v) if relu else v).float().to(dtype).to(dev)
            seen[use_skip, relu] = exp
            buf, x = _guarded(x64, dev, dtype, 7.0)
            _lib.check(fn(_lib.ptr(x), _lib.ptr(bias), _lib.ptr(skip) if use_skip else None, PIXELS, channels, relu,
                          _lib.stream_ptr(dev)), lib)
            _assert_equal(x, exp, f'skip={use_skip} relu={relu}')
            assert _guards_intact(buf, 7.0)
    # the table does what its comments say (conditions on the expectation, not on the kernel)
    e = seen[True, 0].double().cpu()
    assert bool((e == float('inf')).any()) and bool((e == -float('inf')).any()) and not bool(seen[True, 1].double().lt(0).any())
    if dtype == torch.float16:
        tiny = 2.0 ** -14
        exact = x64 + bias64 + skip64
        assert int(((e != 0) & (e.abs() < tiny)).sum()) >= 20 and bool((e == 65504).any()) and bool((e == -65504).any())
        assert bool(((e == tiny) & (exact < tiny)).any())                                           # rounded up to the smallest normal
        frac = exact.abs() / U
        assert int(((frac - frac.floor() == 0.5) & (exact.abs() < tiny)).sum()) >= 8               # ties between two subnormals
        neg = (exact == -120000)
        assert bool(neg.any()) and bool((seen[True, 1].cpu()[neg] == 0).all()) and bool((e[neg] == -float('inf')).all())


@pytest.mark.parametrize("channels", [8, 24])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_upsample2_add_at_the_ends_of_the_range(dev, dtype, channels):
    """up += nearest_x2(low), in place: the bias-free pairs of the table, (up, low) = (x, skip); low pixel i holds pair i + c.
    Both operands are 16-bit numbers, and a sum of two fp16 numbers below 2^-13 is a multiple of 2^-24: it cannot land between two
    subnormals or round up to 2^-14 (those two kinds need the fp32 bias of og_bias_act_*).  What this pass can meet instead: the sum
    that is 2^-14 exactly (1023 U + U), the tie one binade up (2050 U + U -> 2052 U), and 65504 + 16, the tie that goes to inf."""
    lib = _lib.load()
    pairs = TABLES[dtype][0][1]
    h2, w2 = 3, 6
    assert h2 * w2 >= len(pairs)
    low64, up64 = torch.zeros(1, h2, w2, channels, dtype=torch.float64), torch.zeros(1, 2 * h2, 2 * w2, channels, dtype=torch.float64)
    for i in range(h2 * w2):
        for c in range(channels):
            a, b = pairs[(i + c) % len(pairs)]
            y, x = divmod(i, w2)
            low64[0, y, x, c] = b
            up64[0, 2 * y:2 * y + 2, 2 * x:2 * x + 2, c] = a
    for t in (low64, up64):
        assert torch.equal(t.float().to(dtype).double(), t)
    v = _exact32(up64 + low64.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2))
    exp = v.float().to(dtype).to(dev)
    low = low64.float().to(dtype).to(dev).contiguous()
    buf, up = _guarded(up64, dev, dtype, 7.0)
    _lib.check(_lib.lp(lib, 'og_upsample2_add', dtype)(_lib.ptr(up), _lib.ptr(low), 1, 2 * h2, 2 * w2, channels, _lib.stream_ptr(dev)), lib)
    _assert_equal(up, exp, 'up')
    assert _guards_intact(buf, 7.0)
    e = exp.double().cpu()
    assert bool((e == float('inf')).any()) and bool((e == -float('inf')).any()) and int((e != v).sum()) >= 4 * channels


F32_IN = {
    torch.float16: [3 * U, 2.5 * U, 3.5 * U, -2.5 * U, 0.5 * U, 0.5 * U * (1 + 2.0 ** -23), 1.5 * U, 1023 * U, 1023.5 * U, 1023.75 * U,
                    -1023.75 * U, 2.0 ** -14, 1e-10, -0.0, 65504.0, -65504.0, 65519.0, 65520.0, -65520.0, 1e6, 2051 * U, 1.0],
    torch.bfloat16: [3 * BIG, 257 * BIG, 259 * BIG, 513 * BIG, -257 * BIG, 257 * SMALL, 513 * SMALL, 3 * SMALL, BF_MAX, -BF_MAX,
                     BF_MAX + 2.0 ** 119, BF_MAX + 2.0 ** 118, -(BF_MAX + 2.0 ** 119), 1.0, -0.0],
}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_nchw_f32_to_nhwc_at_the_ends_of_the_range(dev, dtype):
    """fp32 NCHW images -> 16-bit NHWC: one rounding per element, subnormals produced, 65520 and beyond to inf.  C = 3 is the only
    channel count the entry point accepts (OG_EUNSUPPORTED otherwise), so there is no 8- or 24-channel form of this test."""
    lib = _lib.load()
    vals = torch.tensor(F32_IN[dtype], dtype=torch.float64).float()                  # (1e-10 is whatever fp32 makes of it)
    n, h, w = 2, 5, 7
    idx = (torch.arange(n * 3 * h * w) * 7 % len(vals)).view(n, 3, h, w)
    src = vals[idx]
    assert set(idx.flatten().tolist()) == set(range(len(vals)))
    exp = src.to(dtype).permute(0, 2, 3, 1).contiguous().to(dev)
    buf = torch.full((exp.numel() + 2 * GUARD,), float('nan'), dtype=dtype, device=dev)
    dst = buf[GUARD:GUARD + exp.numel()].view(exp.shape)
    _lib.check(_lib.lp(lib, 'og_nchw_f32_to_nhwc', dtype)(_lib.ptr(src.to(dev).contiguous()), _lib.ptr(dst), n, 3, h, w,
                                                         _lib.stream_ptr(dev)), lib)
    _assert_equal(dst, exp, 'dst')
    assert bool(torch.cat([buf[:GUARD], buf[-GUARD:]]).isnan().all())
    e = exp.double().cpu()
    assert bool(e.isinf().any()) and int((e != src.permute(0, 2, 3, 1).double()).sum()) >= 8
    if dtype == torch.float16:
        assert int(((e != 0) & (e.abs() < 2.0 ** -14)).sum()) >= 8


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("channels,first,count", [(8, 0, 8), (24, 8, 13)], ids=['8-all', '24-slice'])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_nhwc_to_nchw_f32_at_the_ends_of_the_range(dev, dtype, channels, first, count, with_bias):
    """All 8 channels, and a 13-channel slice of 24, of 16-bit NHWC (+ fp32 bias[first + c]) -> fp32 NCHW: the exact value, nothing
    rounded, flushed or clamped (60000 + 60000 = 120000)."""
    lib = _lib.load()
    x64, _, bias64 = _table(dtype, channels)
    n, h, w = 1, 1, PIXELS
    src = x64.float().to(dtype).to(dev).view(n, h, w, channels).contiguous()
    v = _exact32(x64 + bias64) if with_bias else x64
    exp = v[:, first:first + count].t().reshape(n, count, h, w).float().to(dev)
    assert bool(exp.isfinite().all()) or dtype == torch.bfloat16
    buf = torch.full((exp.numel() + 2 * GUARD,), float('nan'), device=dev)
    dst = buf[GUARD:GUARD + exp.numel()].view(exp.shape)
    fn = lib.og_nhwc_f16_to_nchw_f32 if dtype == torch.float16 else lib.og_nhwc_bf16_to_nchw_f32
    _lib.check(fn(_lib.ptr(src), channels, first, count, _lib.ptr(bias64.float().to(dev)) if with_bias else None, _lib.ptr(dst),
                  n, h, w, _lib.stream_ptr(dev)), lib)
    _assert_equal(dst, exp, 'dst')
    assert bool(torch.cat([buf[:GUARD], buf[-GUARD:]]).isnan().all())
    if dtype == torch.float16:
        e = exp.double().cpu()
        assert int(((e != 0) & (e.abs() < 2.0 ** -14)).sum()) >= 8 and (not with_bias or bool((e.abs() > 65504).any()))
