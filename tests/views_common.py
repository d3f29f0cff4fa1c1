"""The specifications of the model-inspection views (og_draw_heatmap_u8, og_draw_segments_u8, og_limbs_to_segments_f32,
og_offsets_to_segments_f32 in include/og_decoder.h) restated in numpy, and the cases the CPU and GPU tests share.

The restatements are written from the header text, not from the kernels: no tiles, no halo, no lists, no culling -- every pixel and every
primitive is evaluated on the whole image -- and ONE numpy operation per arithmetic operation, so that dtype=np.float32 reproduces every
rounding of the kernels (numpy's +, -, *, / and sqrt are correctly rounded, as theirs are) and dtype=np.float64 is the check of the
restatement itself, as in draw_common.py.  They take the x4 maps as inputs: `hires(case)` gets them from the oracle's bicubic / bilinear
upsample (which existing tests pin og_upsample_*4_f32 to)."""
import numpy as np

import oracle
from draw_common import LIST_CAP

TILE_W, TILE_H = 64, 16            # the heat-map overlay's tile (csrc/views.hip); the painter's tile is draw_common's 32 x 8
ROUND = 256                        # rows / grid points one workgroup pass of the compactions handles


# ---------------------------------------------------------------------------------------------------------------- restatements
def heatmap_reference(images, v, lut, vmin, vmax, alpha, nms, dtype):
    """images (N,H,W,3) uint8, v (N,H,W) float32: the x4 bicubic plane of the channel, lut (n_colors,3) uint8 -> painted copy."""
    T = dtype
    images, lut = np.asarray(images), np.asarray(lut, dtype=np.uint8)
    v = np.asarray(v, dtype=np.float32)
    N, H, W, _ = images.shape
    assert v.shape == (N, H, W)
    out = images.copy()
    zero, one, half = T(0), T(1), T(0.5)
    vmin, vmax, alpha = T(np.float32(vmin)), T(np.float32(vmax)), T(np.float32(alpha))
    with np.errstate(all='ignore'):
        vt = v.astype(T)
        if nms:
            padded = np.zeros((N, H + 2, W + 2), T)                       # a neighbour outside the image counts as 0
            padded[:, 1:-1, 1:-1] = vt
            m = np.full((N, H, W), -np.inf, T)
            for dy in range(3):
                for dx in range(3):
                    m = np.fmax(m, padded[:, dy:dy + H, dx:dx + W])       # fmax: a NaN is never the larger one
            u = vt * np.where(m == vt, one, zero)
        else:
            u = vt
        written = ~np.isnan(u)
        t = np.fmin(np.fmax((u - vmin) / (vmax - vmin), zero), one)
        idx = np.floor(t * T(np.float32(len(lut) - 1)) + half)
        idx = np.where(written, idx, 0).astype(np.int64)
        for ch in range(3):
            c = images[..., ch].astype(T)
            c = c + (lut[idx, ch].astype(T) - c) * alpha
            out[..., ch][written] = np.floor(c + half)[written].astype(np.uint8)
    return out


def segments_reference(images, segs, n_segs, line_rgb, marker_rgb, line_width, r_start, r_end, alpha, dtype):
    """images (N,H,W,3) uint8, segs (N,S,4) float32 rows x1, y1, x2, y2, n_segs (N) -> painted copy.  The coverage, blending and rounding
    are og_draw_poses_u8's (the arithmetic of draw_common.draw_reference), over the primitives capsule, start disc, end disc."""
    T = dtype
    images, segs = np.asarray(images), np.asarray(segs, dtype=np.float32)
    N, H, W, _ = images.shape
    S = segs.shape[1]
    out = images.copy()
    PX = np.broadcast_to(np.arange(W, dtype=T)[None, :], (H, W))
    PY = np.broadcast_to(np.arange(H, dtype=T)[:, None], (H, W))
    half, zero, one, alpha = T(0.5), T(0), T(1), T(np.float32(alpha))
    r_line, r_start, r_end = T(np.float32(line_width)) / T(2), T(np.float32(r_start)), T(np.float32(r_end))
    line, marker = np.asarray(line_rgb, np.uint8).astype(T), np.asarray(marker_rgb, np.uint8).astype(T)
    with np.errstate(all='ignore'):
        for n in range(N):
            c = [images[n, :, :, ch].astype(T) for ch in range(3)]
            touched = np.zeros((H, W), bool)
            for s in range(min(max(int(n_segs[n]), 0), S)):
                x1, y1, x2, y2 = (T(v) for v in segs[n, s])
                if not (np.isfinite(x1) and np.isfinite(y1) and np.isfinite(x2) and np.isfinite(y2)):
                    continue
                prims = [(x1, y1, x2, y2, r_line, line)]
                if r_start > 0:
                    prims.append((x1, y1, x1, y1, r_start, marker))
                if r_end > 0:
                    prims.append((x2, y2, x2, y2, r_end, marker))
                for ax, ay, bx, by, r, colour in prims:
                    dx = bx - ax
                    dy = by - ay
                    len2 = dx * dx + dy * dy
                    if len2 == 0:
                        t = np.zeros((H, W), T)
                    else:
                        t = ((PX - ax) * dx + (PY - ay) * dy) / len2
                        t = np.fmin(np.fmax(t, zero), one)
                    qx = ax + t * dx
                    qy = ay + t * dy
                    ex = PX - qx
                    ey = PY - qy
                    d = np.sqrt(ex * ex + ey * ey)
                    cov = np.fmin(np.fmax((r + half) - d, zero), one)
                    hit = cov > 0
                    w = cov * alpha
                    for ch in range(3):
                        c[ch] = np.where(hit, c[ch] + (colour[ch] - c[ch]) * w, c[ch])
                    touched |= hit
            for ch in range(3):
                out[n, :, :, ch][touched] = np.floor(c[ch] + half)[touched].astype(np.uint8)
    return out


def limbs_to_segments_reference(limbs, limb, dist_max):
    """limbs (N,L,K,13) float32 -> a list of N arrays (n_segs[n], 4): the kept rows in (l, i) order (boolean-mask selection keeps it)."""
    limbs = np.asarray(limbs, dtype=np.float32)
    N, L, K, _ = limbs.shape
    with np.errstate(invalid='ignore'):
        keep = (limbs[..., 0] > 0) & (limbs[..., 3] > 0) & (limbs[..., 8] <= np.float32(dist_max))
    if limb is not None and limb >= 0:
        keep &= (np.arange(L) == limb)[None, :, None]
    return [limbs[n][keep[n]][:, [0, 1, 3, 4]] for n in range(N)]


def offsets_to_segments_reference(heat, U, V, step, thre):
    """heat, U, V (N,H,W) float32: the x4 bicubic plane of the joint and the x4 bilinear planes of the limb's two offset channels ->
    a list of N arrays (n_segs[n], 4) in row-major grid order."""
    heat, U, V = (np.asarray(a, dtype=np.float32) for a in (heat, U, V))
    N, H, W = heat.shape
    ys, xs = np.arange(0, H, step), np.arange(0, W, step)
    Y, X = np.meshgrid(ys, xs, indexing='ij')
    out = []
    with np.errstate(invalid='ignore', over='ignore'):
        for n in range(N):
            h_, u_, v_ = heat[n][Y, X], U[n][Y, X], V[n][Y, X]
            keep = (h_ >= np.float32(thre)) & np.isfinite(u_) & np.isfinite(v_)
            fx, fy = X.astype(np.float32), Y.astype(np.float32)
            rows = np.stack([fx, fy, fx + u_, fy + v_], axis=2)          # float32 + float32: one fp32 add each
            out.append(rows[keep])
    return out


# ------------------------------------------------------------------------------------------------------------------------ cases
def _base(N, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (N, H, W, 3), dtype=np.uint8)


def heatmap_cases():
    """name -> dict(images, hm (N,C,h,w), channel, lut, vmin, vmax, alpha, nms): the smallest shapes at which the overlay can go wrong
    (64 x 16 tiles with a one-pixel halo, four rows per thread)."""
    from offsetguided_amd.visualization import VIRIDIS
    two = np.array([[10, 200, 90], [240, 30, 160]], np.uint8)
    out = {}
    rng = np.random.default_rng(21)
    # 5 x 11 -> a 20 x 44 image: partial tiles on both axes
    small = rng.uniform(-0.2, 1.2, (1, 1, 5, 11)).astype(np.float32)
    for nms in (0, 1):
        out[f'small_nms{nms}'] = dict(images=_base(1, 20, 44, 1), hm=small, channel=0, lut=VIRIDIS, vmin=0.0, vmax=1.0, alpha=0.8, nms=nms)
    # 9 x 35 -> 36 x 140: 3 x 3 tiles, N = 2, C = 3, channel 2 (plane and batch strides), a range other than [0, 1], two colours
    multi = rng.uniform(-0.3, 0.9, (2, 3, 9, 35)).astype(np.float32)
    for nms in (0, 1):
        out[f'multi_nms{nms}'] = dict(images=_base(2, 36, 140, 2), hm=multi, channel=2, lut=two, vmin=-0.1, vmax=0.7, alpha=1.0, nms=nms)
    # a plateau: a constant map upsamples to the same constant everywhere (the weights are dyadics that sum to 1): every pixel is kept
    out['plateau'] = dict(images=_base(1, 20, 44, 3), hm=np.full((1, 1, 5, 11), 0.5, np.float32), channel=0, lut=VIRIDIS, vmin=0.0,
                          vmax=1.0, alpha=1.0, nms=1)
    # negative everywhere: on the border the zero padding wins (nothing kept there, u = -0), inside every pixel is its window's maximum
    out['negative'] = dict(images=_base(1, 20, 44, 4), hm=np.full((1, 1, 5, 11), -0.25, np.float32), channel=0, lut=VIRIDIS, vmin=-0.5,
                           vmax=0.5, alpha=1.0, nms=1)
    # peaks on every corner and edge of the image and on the tile seams: a spike in a corner / border cell of the stride-4 map puts its
    # x4 maximum on the image's corner / border pixels; two equal neighbouring cells put a pair of equal maxima on the pixels either side
    # of their boundary -- cells 15 | 16 across meet at the tile seam X = 63 | 64, cells 3 | 4 down at Y = 15 | 16
    peaks = rng.uniform(0.0, 0.05, (1, 1, 9, 35)).astype(np.float32)
    for y, x in [(0, 0), (0, 34), (8, 0), (8, 34), (0, 10), (8, 20), (5, 0), (4, 34)]:
        peaks[0, 0, y, x] = 1.0
    # (the seam pairs sit in a patch of zeros and carry dyadic values, so that the two maxima are equal to the last bit)
    peaks[0, 0, 1:9, 13:19] = 0.0
    peaks[0, 0, 1:7, 26:31] = 0.0
    peaks[0, 0, 7, 15:17] = 0.75         # the X seam
    peaks[0, 0, 3:5, 28] = 0.5           # the Y seam
    peaks[0, 0, 3:5, 15:17] = 0.625      # the corner where four tiles meet
    out['peaks'] = dict(images=_base(1, 36, 140, 5), hm=peaks, channel=0, lut=VIRIDIS, vmin=0.0, vmax=1.0, alpha=0.8, nms=1)
    # NaN and +-inf in the map
    bad = rng.uniform(0.0, 1.0, (1, 1, 5, 11)).astype(np.float32)
    bad[0, 0, 1, 2], bad[0, 0, 3, 6], bad[0, 0, 2, 9] = np.nan, np.inf, -np.inf
    for nms in (0, 1):
        out[f'nonfinite_nms{nms}'] = dict(images=_base(1, 20, 44, 6), hm=bad, channel=0, lut=VIRIDIS if nms else two, vmin=0.0, vmax=1.0,
                                          alpha=0.8, nms=nms)
    return out


def segment_cases():
    """name -> dict(images, segs (N,S,4), n_segs, line_rgb, marker_rgb, line_width, r_start, r_end, alpha)."""
    red, green = (255, 0, 0), (0, 128, 0)
    out = {}
    rng = np.random.default_rng(31)
    # a zero-length segment, segments wholly and partly outside the image, an image without segments, a count beyond S, rows never read
    segs = np.zeros((3, 6, 4), np.float32)
    segs[:, :, 0::2] = rng.uniform(-8.0, 52.0, (3, 6, 2))
    segs[:, :, 1::2] = rng.uniform(-8.0, 26.0, (3, 6, 2))
    segs[0, 0] = (12.0, 9.0, 12.0, 9.0)                     # zero length
    segs[0, 1] = (-30.0, -20.0, -12.0, -15.0)               # wholly outside
    segs[0, 2] = (40.0, 10.0, 60.0, 30.0)                   # partly outside
    segs[2, 4:] = (np.nan, 1e30, 5.0, 5.0)                  # beyond n_segs[2]: never read
    out['basic'] = dict(images=_base(3, 19, 45, 1), segs=segs, n_segs=[9, 0, 4], line_rgb=red, marker_rgb=green, line_width=2.0,
                        r_start=3.0, r_end=3.0, alpha=1.0)
    # non-finite coordinates skip the whole segment, discs included; r_start = 0: no start disc
    bad = segs[:1].copy()
    bad[0, 1, 2], bad[0, 3, 1], bad[0, 4, 0] = np.nan, np.inf, -np.inf
    out['nonfinite_rstart0'] = dict(images=_base(1, 19, 45, 2), segs=bad, n_segs=[6], line_rgb=(20, 40, 250), marker_rgb=(250, 250, 0),
                                    line_width=1.0, r_start=0.0, r_end=1.5, alpha=0.5)
    # more capsules through one tile than the list holds, plus one more (no discs: one primitive per segment), alpha 0.5
    S = LIST_CAP + 1
    stack = np.zeros((1, S, 4), np.float32)
    stack[0, :, :2] = np.array([36.0, 2.0]) + rng.uniform(-1.5, 1.5, (S, 2))
    stack[0, :, 2:] = np.array([56.0, 5.0]) + rng.uniform(-1.5, 1.5, (S, 2))
    out['overflow'] = dict(images=_base(1, 16, 64, 3), segs=stack, n_segs=[S], line_rgb=(200, 100, 50), marker_rgb=green, line_width=2.0,
                           r_start=0.0, r_end=0.0, alpha=0.5)
    # red lines and green discs overlapping, the two rows in both orders: b starts at (20, 9), on a's line
    cross = np.array([[(10.0, 6.0, 30.0, 12.0), (20.0, 9.0, 34.0, 16.0)]], np.float32)
    for name, table in (('order_ab', cross), ('order_ba', cross[:, ::-1].copy())):
        out[name] = dict(images=_base(1, 19, 45, 4), segs=table, n_segs=[2], line_rgb=red, marker_rgb=green, line_width=3.0, r_start=3.0,
                         r_end=3.0, alpha=1.0)
    return out


HEATMAP_CASES = heatmap_cases()
SEGMENT_CASES = segment_cases()


def limb_tables():
    """name -> dict(limbs (N,L,K,13), limb, dist_max): rejected rows of each kind, the boundary values, a filter, nothing kept."""
    rng = np.random.default_rng(41)

    def random(N, L, K):
        t = rng.uniform(-5.0, 60.0, (N, L, K, 13)).astype(np.float32)        # ~8 % of x1 / x2 are <= 0, ~60 % of col8 beyond 20
        t[..., 8] = rng.uniform(0.0, 50.0, (N, L, K))
        return t
    big = random(2, 19, 48)
    big[0, 0, 0, [0, 3, 8]] = (0.0, 5.0, 1.0)               # col0 == 0: rejected
    big[0, 0, 1, [0, 3, 8]] = (5.0, 5.0, 20.0)              # col8 == dist_max: kept
    big[0, 0, 2, [0, 3, 8]] = (5.0, 5.0, np.nan)            # NaN: rejected
    big[0, 0, 3, [0, 3, 8]] = (5.0, -1.0, 1.0)              # col3 <= 0: rejected
    big[0, 0, 4, [0, 3, 8]] = (np.nan, 5.0, 1.0)
    nothing = random(2, 19, 48)
    nothing[..., 8] += 100.0
    one = np.zeros((1, 1, 1, 13), np.float32)
    one[0, 0, 0, [0, 1, 3, 4, 8]] = (3.0, 4.0, 5.0, 6.0, 2.0)
    return {'random': dict(limbs=big, limb=None, dist_max=20.0), 'filter': dict(limbs=big, limb=7, dist_max=35.0),
            'nothing': dict(limbs=nothing, limb=None, dist_max=20.0), 'one': dict(limbs=one, limb=None, dist_max=20.0),
            'one_filtered': dict(limbs=one, limb=0, dist_max=1.0)}


def offset_fields():
    """name -> dict(hm (N,C,h,w), off (N,2L,h,w), joint_from, limb, step, thre)."""
    rng = np.random.default_rng(51)
    hm = rng.uniform(0.0, 0.6, (2, 3, 5, 11)).astype(np.float32)
    hm[1] *= 0.5                                             # another count in the second image
    hm[0, 1, :, 3:8] = 0.25                                  # a 5 x 5 block of equal cells: where all sixteen taps fall inside it the
                                                             # x4 value is 0.25 itself (dyadic weights that sum to 1), e.g. at (7, 21)
    off = rng.uniform(-9.0, 9.0, (2, 8, 5, 11)).astype(np.float32)
    off[0, 4, 1, 2], off[0, 5, 3, 7], off[1, 4, 4, 10] = np.inf, -np.inf, np.nan
    dense = rng.uniform(0.3, 0.9, (1, 1, 5, 11)).astype(np.float32)         # everything kept at step 1: 880 points, four passes
    return {'step7': dict(hm=hm, off=off, joint_from=1, limb=2, step=7, thre=0.25),
            'step3': dict(hm=hm, off=off, joint_from=2, limb=0, step=3, thre=0.2),
            'step1': dict(hm=hm, off=off, joint_from=1, limb=2, step=1, thre=0.25),
            'dense': dict(hm=dense, off=rng.uniform(-3.0, 3.0, (1, 2, 5, 11)).astype(np.float32), joint_from=0, limb=0, step=1,
                          thre=0.2)}


LIMB_TABLES = limb_tables()
OFFSET_FIELDS = offset_fields()

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        value = make()
        for a in (value if isinstance(value, (list, tuple)) else [value]):
            a.setflags(write=False)
        _CACHE[key] = value
    return _CACHE[key]


def hires(case):
    """The x4 bicubic plane (N,4h,4w) of a heat-map case's channel, from the oracle."""
    return np.ascontiguousarray(oracle.bicubic4(case['hm'])[:, case['channel']])


def heatmap_expected(name, dtype=np.float32):
    """The restatement's result for a heat-map case, computed once per process and handed out read-only."""
    c = HEATMAP_CASES[name]
    return _once(('hm', name, np.dtype(dtype).name), lambda: heatmap_reference(
        c['images'], hires(c), c['lut'], c['vmin'], c['vmax'], c['alpha'], c['nms'], dtype))


def segments_expected(name, dtype=np.float32):
    c = SEGMENT_CASES[name]
    return _once(('seg', name, np.dtype(dtype).name), lambda: segments_reference(dtype=dtype, **c))


def limbs_expected(name):
    c = LIMB_TABLES[name]
    return _once(('limbs', name), lambda: limbs_to_segments_reference(c['limbs'], c['limb'], c['dist_max']))


def offset_planes(case):
    """(heat, U, V), each (N,4h,4w): the oracle's x4 bicubic of the joint's channel and x4 bilinear of the limb's two channels."""
    with np.errstate(all='ignore'):
        heat = oracle.bicubic4(case['hm'][:, case['joint_from']])
        U = oracle.bilinear4(case['off'][:, 2 * case['limb']])
        V = oracle.bilinear4(case['off'][:, 2 * case['limb'] + 1])
    return heat, U, V


def offsets_expected(name):
    c = OFFSET_FIELDS[name]
    return _once(('offs', name), lambda: offsets_to_segments_reference(*offset_planes(c), c['step'], c['thre']))
