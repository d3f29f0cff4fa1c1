"""Shared by the range-report tests: the nine words of a stats row (include/og_decoder.h, "range report") restated in numpy on bit
patterns, independently of the kernel -- the 16-bit value y is COMPUTED (an integer round-to-nearest-even for fp16, the to_lp rule
of csrc/fold.hip for bf16) and the classes are read off x and y, where the kernel compares x against thresholds -- and the directed
values both tests use."""
import numpy as np

WORDS = 9
NAMES = ('n', 'nan', 'inf', 'over', 'zero', 'flush', 'sub', 'max', 'min')
F32_INF = 0x7f800000
LP = {'f16': (0x7c00, 0x0400), 'bf16': (0x7f80, 0x0080)}       # target -> (pattern of inf, smallest normal), without the sign


def f32_to_f16_bits(u):
    """uint32 fp32 patterns -> uint16 fp16 patterns of |x|, round to nearest even, subnormals kept, integers only."""
    a = (np.asarray(u, np.uint32) & np.uint32(0x7fffffff)).astype(np.int64)
    exp, man = a >> 23, a & 0x7fffff
    sig = np.where(exp > 0, man | (1 << 23), man)
    e = np.maximum(exp, 1)                                    # |x| = sig * 2^(e - 150)
    field = e - 112                                           # fp16's exponent field of a normal result
    shift = np.clip(np.where(field >= 1, 13, 126 - e), 13, 40)     # below the normals the unit stays 2^-24
    q, rem, half = sig >> shift, sig & ((1 << shift) - 1), 1 << (shift - 1)
    q = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    out = np.where(field >= 1, ((field - 1) << 10) + q, q)   # the carry of a rounded-up mantissa moves the exponent by itself
    out = np.minimum(out, 0x7c00)
    out = np.where(exp == 255, np.where(man == 0, 0x7c00, 0x7e00), out)
    return out.astype(np.uint16)


def f32_to_bf16_bits(u):
    """to_lp of csrc/fold.hip on |x|: u += 0x7fff + ((u >> 16) & 1); u >> 16; a NaN becomes 0x7fc0."""
    a = (np.asarray(u, np.uint32) & np.uint32(0x7fffffff)).astype(np.int64)
    r = (a + 0x7fff + ((a >> 16) & 1)) >> 16
    return np.where(a > F32_INF, 0x7fc0, r).astype(np.uint16)


def widen(bits16, target):
    """16-bit patterns -> the fp32 patterns of the same values (exact)."""
    bits16 = np.asarray(bits16, np.uint16)
    if target == 'bf16':
        return bits16.astype(np.uint32) << np.uint32(16)
    return bits16.view(np.float16).astype(np.float32).view(np.uint32)


def stats_ref(bits, source, target):
    """The nine words (int64[9]) of the elements whose bit patterns are `bits`: uint32 for source 'f32', uint16 for a 16-bit source
    (which must be the target)."""
    inf_t, normal_t = LP[target]
    if source == 'f32':
        x = np.asarray(bits, np.uint32).reshape(-1)
        y = (f32_to_f16_bits(x) if target == 'f16' else f32_to_bf16_bits(x)).astype(np.int64)
    else:
        assert source == target
        y = (np.asarray(bits, np.uint16).reshape(-1) & np.uint16(0x7fff)).astype(np.int64)
        x = widen(np.asarray(bits, np.uint16).reshape(-1), target)
    a = (x & np.uint32(0x7fffffff)).astype(np.int64)
    fin = a < F32_INF
    out = np.zeros(WORDS, np.int64)
    out[0] = a.size
    out[1] = (a > F32_INF).sum()
    out[2] = (a == F32_INF).sum()
    out[3] = (fin & (y == inf_t)).sum()
    out[4] = (a == 0).sum()
    out[5] = ((a != 0) & (y == 0)).sum()
    out[6] = ((y > 0) & (y < normal_t)).sum()
    out[7] = a[fin].max() if fin.any() else 0
    some = fin & (a != 0)
    out[8] = (F32_INF - a[some]).max() if some.any() else 0
    return out


def combine(parts):
    parts = np.stack([np.asarray(p, np.int64) for p in parts])
    return np.concatenate([parts[:, :7].sum(0), parts[:, 7:].max(0)])


# fp32 patterns at every edge of the two targets (each also with the sign set, see directed32)
DIRECTED32 = [
    0x477fefff, 0x477ff000, 0x477fe000,            # 65519.996 (the last fp32 below 65520), 65520, 65504
    0x32ffffff, 0x33000000, 0x33000001,            # 2^-25 and its two fp32 neighbours
    0x33800000,                                    # 2^-24
    0x387fdfff, 0x387fe000, 0x387fffff,            # round the tie 1023.5 * 2^-24, and the largest fp32 below 2^-14: up to a normal
    0x38800000,                                    # 2^-14
    0x7f7f7fff, 0x7f7f8000, 0x7f7fffff,            # bf16: the last pattern that stays finite, the first that does not, fp32's largest
    0x00008000, 0x00008001, 0x00000001, 0x007fffff, 0x00800000,      # bf16's flush edge, fp32 subnormals, fp32's smallest normal
    0x007f8000, 0x007f7fff, 0x00800000 - 0x8000,   # round bf16's subnormal / normal edge
    0x00000000, 0x7f800000, 0x7fc00000, 0x7f800001, 0x7fc12345, 0x7fffffff,     # 0, inf, NaNs with payloads
    0x3f800000, 0x40490fdb,
]


def directed32():
    v = np.array(DIRECTED32, np.uint32)
    return np.concatenate([v, v | np.uint32(0x80000000)])


def directed16(target):
    inf_t, normal_t = LP[target]
    v = np.array([0, 1, normal_t - 1, normal_t, normal_t + 1, inf_t - 1, inf_t, inf_t + 1, inf_t | 0x155, 0x7fff, 0x3c00 if target == 'f16' else 0x3f80],
                 np.uint16)
    return np.concatenate([v, v | np.uint16(0x8000)])
