"""Directed scenes for the limb pairing (og_collect::limb_rows, csrc/collect_body.h) -- shared by tools/gen_golden_pairing.py,
tests/test_pairing_cpu.py and tests/test_gpu_pairing.py.  No GPU code, no reference import.

A case PLANTS its candidates: isolated positive pixels in a zero heat map at input resolution, so the peak list of every plane
and its scores are exactly what was planted (K + 2 peaks per plane with distinct scores: no zero filler, no top-k tie).  Every value
-- scores, stride-4 offset / scale / jitter maps -- sits on a dyadic grid, so the x4 bilinear taps, the guide points and the
planned distance ties are exact in fp32.  What a scene holds (`build`):

  common pixel   image 0: one pixel planted in EVERY plane with the best score, zero offsets around it -> from- and to-candidate
                 on the same pixel, len clamped to min_len
  tie            limb TIE_LIMB, offsets 0: the from-peak TIE_FROM has two to-candidates at distance exactly 5 (5,0) / (3,4) and none
                 nearer -> torch.min's first-minimum rule decides
  border         peaks on the corners and on the first / last row and column (both taps of the x4 sampling clamp there); the odd
                 planes leave the origin free, so a guide point up and left of the image has no candidate there
  guide points   limb NEG_LIMB, offsets (-1/2, -1/2), from-peaks on column 0 / row 0: guide points in (-1, 0), which .int() truncates
                 to 0, so the jitter gate admits them; limb OUT_LIMB, offsets (+8.5, -1/4), from-peaks on the last column: x >= W
  sub-threshold  every list ends in candidates with a score in (0, thre_hmp) (the -100000 shift); image 1, plane SUB_PLANE lies
                 below the threshold as a whole

Each case names the conditions it is built for (`conditions`); `count` counts their occurrences from the reference's intermediate
values (its top-k lists, its limbs, the x4 maps), and the generator, the CPU test and the GPU test all assert every count >= 1.

STORED cases have the reference's lists and limbs in the fixture.  DIGEST cases -- K on both sides of the collect fallback of
og_generate_limbs_f32 (`plan` restates where it lies), the scale head on 4-component offsets, scale and jitter heads together, the
44-limb skeleton at K = 33 / 65 / 100 -- have the SHA-256 of them there; `load` gives the C oracle's rows, held to those digests."""
from collections import namedtuple

import numpy as np

from offsetguided_amd import synth
from offsetguided_amd.config import coco_data as cd

THRE, MIN_LEN, N_IMAGES = 0.04, 0.5, 2
SKELETONS = {'omp19': cd.COCO_PERSON_SKELETON, 'omp44': cd.DENSER_COCO_PERSON_SKELETON}
TIE_LIMB, NEG_LIMB, OUT_LIMB, SUB_PLANE = 2, 5, 7, 16
TIE_FROM, TIE_TO = (12, 20), ((12, 15), (16, 23))          # (y, x): the to-peaks are (-5, 0) and (+3, +4) away from the guide point

Case = namedtuple('Case', 'name K H W skeleton nd heads')


def _cases():
    out = [Case(f'plain_k{k}', k, 48, 80, 'omp19', 2, 'none') for k in (1, 3, 7, 31, 32, 33, 63, 64, 65, 100)]
    out.append(Case('plain44_k7', 7, 48, 80, 'omp44', 2, 'none'))
    out += [Case(f'scale_k{k}', k, 48, 80, 'omp19', 2, 'scale') for k in (7, 32, 33, 65)]      # the plain scene + scale maps
    out += [Case(f'jitter_k{k}', k, 64, 64, 'omp19', 2, 'jitter') for k in (7, 32, 33, 65)]     # square: the [x][y] lookup
    out += [Case(f'cat_k{k}', k, 48, 80, 'omp19', 4, 'none') for k in (32, 48, 65)]
    return out


# ---------------------------------------------------------------------------------- what og_generate_limbs_f32 does with a shape
LDS_LIMIT = 64 * 1024 - 256            # kDynLdsLimit (csrc/nms_topk.hip, run_topk)
Plan = namedtuple('Plan', 'route nbands wl lds workspace')


def plan(N, C, H, W, k):
    """og_generate_limbs_f32 on hi-res heat maps (16-byte aligned, OG_NMS_ROWS at its default), restated from make_plan, run_topk and
    two_step_bytes (csrc/nms_topk.hip): route 'in_launch' (the merge launch pairs the limbs) / 'fallback' (the lists go through the
    workspace to og_collect_launch) / 'merge_refused' (the band lists do not fit the merge stage's LDS: OG_EUNSUPPORTED after the band
    launch) / None (make_plan refuses: og_generate_limbs_workspace_bytes = 0), the bands per plane, the lists per band, the dynamic LDS
    of the merge-and-pair launch, og_generate_limbs_workspace_bytes."""
    up = lambda v: (v + 255) // 256 * 256  # noqa: E731
    planes, vec = N * C, 4 if W % 4 == 0 else 1
    ws_waves = -(-(-(-W // vec)) // 62)                                   # kInterior lanes per wave panel
    rows = min(max(80, -(-H // 64)), H)
    nbands, cap = -(-H // rows), (2 * k + 64 + 63) // 64 * 64
    if ws_waves > 16 or ws_waves * 2 * cap * 8 > 60 * 1024:
        return Plan(None, nbands, 0, 0, 0)
    wl = ws_waves if ws_waves > 1 and 4 * nbands * ws_waves * k * 8 <= 40 * 1024 else 1
    topk = 256 + up(planes * 256 * 4) + up(planes * nbands * wl * k * 8)    # [magic | slot tables | band keys]
    workspace = 64 * 1024 + up(topk) + up(N * C * k * 12)                   # [tickets | top-k | inds | scores]
    mlds = 2 * nbands * wl * k * 8
    plds = 2 * mlds + ((k + 3) & ~3) * 32
    if mlds > LDS_LIMIT:
        return Plan('merge_refused', nbands, wl, plds, workspace)
    return Plan('in_launch' if plds <= LDS_LIMIT and k <= 2048 else 'fallback', nbands, wl, plds, workspace)


def smallest_plane(k):
    """The smallest plane with H, W multiples of 4 (the stride-4 maps) that the entry point admits for k (2 (H + W) - 4 >= k): the
    smallest such H + W, split as evenly as one wave panel per row allows (W <= 4 * 62; a second panel halves the k make_plan takes)."""
    s = -(-(-(-(k + 4) // 2)) // 4) * 4
    w = min(-(-(s // 2) // 4) * 4, 248)
    return s - w, w


# The switch to the collect fallback, read from run_topk: plds = 32 k nbands wl + 32 ((k + 3) & ~3) <= LDS_LIMIT.  On its smallest plane
# k = 644 has 160 rows = 2 bands of 80 (61 824 bytes: in-launch); k = 645 needs 164 rows = 3 bands (82 656 bytes: the first k that takes
# the fallback UNDER THIS PLANE CONVENTION -- the switch is a property of (H, W, k), not of k: 160 x 168 admits k = 645 with 2 bands
# and pairs it in the launch, and with H <= 80, W = 248 every k up to 652 does).  k = 1020 on 264 x 248 (4 bands) fills the merge
# stage's own LDS to the byte (mlds = 65 280) and is the largest k og_generate_limbs_f32 runs at all on a smallest plane: k = 1021 is refused there (merge_refused), a wider plane needs a second wave
# panel, whose band buffers make_plan admits up to k = 928 only, and past k = 1888 make_plan refuses every plane.  So no k reaches
# the `k <= 2048` half of can_pair, and og_collect_launch refuses k > 2048 as well: test_gpu_pairing.py pins those refusals.
IN_LAUNCH_K, FALLBACK_K, LARGEST_K = 644, 645, 1020


def _new_cases():
    out = [Case(f'fallback_k{k}', k, *smallest_plane(k), 'omp19', 2, 'none') for k in (IN_LAUNCH_K, FALLBACK_K, LARGEST_K)]
    out += [Case(f'scale_cat_k{k}', k, 48, 80, 'omp19', 4, 'scale') for k in (32, 65)]           # the cat scene + scale maps
    out += [Case(f'both_k{k}', k, 64, 64, 'omp19', 2, 'both') for k in (7, 33, 65)]              # the jitter scene + scale maps
    out += [Case(f'plain44_k{k}', k, 48, 80, 'omp44', 2, 'none') for k in (33, 65, 100)]
    return out


STORED = _cases()                      # the fixture holds the reference's lists and limbs
DIGEST = _new_cases()                  # the fixture holds SHA-256 digests of them: expected = the oracle's rows, held to the digests
SCALES_STORED = ('scale_cat_k32',)     # DIGEST cases whose columns 11 / 12 fit into the fixture as arrays besides (8 KB of its 12 KB of room)
CASES = STORED + DIGEST
BY_NAME = {c.name: c for c in CASES}


def skeleton(case):
    return SKELETONS[case.skeleton]


def conditions(case):
    """The conditions the case is built for; every one must occur (count >= 1)."""
    k = case.K
    out = ['border_from', 'min_len', 'sub_to_list']
    if k >= 3:
        out += ['sub_from', 'border_to']
    if case.heads in ('jitter', 'both'):
        out += ['guide_neg', 'guide_x_ge_w', 'jitter_xy']
    elif k >= 3:
        out += ['tie']
    if k % 4:
        out += ['origin_nearest']
    if k > 64:
        out += ['second_candidate']
    if case.name.startswith('fallback'):
        out += ['fallback_taken' if k >= FALLBACK_K else 'last_in_launch']
        if k > FALLBACK_K:
            out += ['rows_past_switch']
    if case.heads == 'scale' and case.nd == 4:
        out += ['scale_differs_on_cat']
    if case.heads == 'both':
        out += ['both_heads_move']
    if case.skeleton == 'omp44' and k > 64:
        out += ['k64_taps_differ']
    return out


# ---------------------------------------------------------------------------------- scene
def _seed(case):
    return 9000 + 7 * case.K + case.H + 3 * case.nd + len(skeleton(case))     # the heads do not enter: scale_k7 shares plain_k7's scene


def _dyadic(seed, shape, lo, hi, den):
    n = int(np.prod(shape))
    return (synth.HashRng(seed).integers(n, lo, hi).astype(np.float32) / np.float32(den)).reshape(shape)


def _plant(order, forced, avoid, P, H, W):
    """P pairwise non-adjacent pixels: the forced ones in their order, then pixels in the shuffled `order` outside `avoid`."""
    taken = np.zeros((H + 2, W + 2), bool)
    out = []

    def take(y, x):
        if taken[y:y + 3, x:x + 3].any():
            return
        taken[y + 1, x + 1] = True
        out.append((y, x))
    for y, x in forced:
        if len(out) < P:
            take(y, x)
    for i in order:
        if len(out) >= P:
            break
        y, x = int(i) // W, int(i) % W
        if all((y - cy) ** 2 + (x - cx) ** 2 > r2 for cy, cx, r2 in avoid):
            take(y, x)
    assert len(out) == P
    return out


def build(case):
    """-> dict(hm_hr (N,17,H,W), off_lr (N,nd*L,H/4,W/4), scl_lr (N,17,H/4,W/4) | None, jit_lr (N,2,H/4,W/4) | None)"""
    sk, K, H, W, nd = skeleton(case), case.K, case.H, case.W, case.nd
    L, C, P, seed = len(sk), 17, case.K + 2, _seed(case)
    jf, jt = [a for a, _ in sk], [b for _, b in sk]
    common = (H // 2 + 1, W // 2 + 3)
    borders = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2 + 1), (H // 2, 0), (H // 2 + 1, W - 1)]
    hm = np.zeros((N_IMAGES, C, H, W), np.float32)
    n_sub = min(P - 1, 2 + max(1, K // 8))
    pow2 = lambda v: 1 << (int(v) - 1).bit_length()  # noqa: E731
    d_top, d_sub, d_plane = max(128, pow2(P + 23)), max(512, pow2(26 * n_sub)), max(4096, pow2(26 * P))   # 128, 512, 4096 up to K = 100
    for n in range(N_IMAGES):
        for c in range(C):
            forced, avoid = ([common] if n == 0 else []), []
            if c == jf[TIE_LIMB]:
                forced.append(TIE_FROM)
            if c == jt[TIE_LIMB]:
                forced += list(TIE_TO)
                avoid.append((TIE_FROM[0], TIE_FROM[1], 42))          # nothing else within sqrt(42) > 5 of the guide point
            if c == jf[NEG_LIMB]:
                forced += [(0, 0), (10, 0), (0, 10)]
            if c == jf[OUT_LIMB]:
                forced += [(H // 2 + 1, W - 1), (H - 1, W - 1)]
            forced += [b for b in borders[c % 8:] + borders[:c % 8] if b != (0, 0) or c % 2 == 0]   # odd planes: no peak on the origin, where
            #                                                                    a to-list padded with zeros would put its padding
            order = np.argsort(synth.HashRng(seed + 100 * n + c).uniform(H * W), kind='stable')
            for j, (y, x) in enumerate(_plant(order, forced, avoid, P, H, W)):      # j = rank: the forced peaks score best
                if n == 1 and c == SUB_PLANE:
                    s = (P - j) / float(d_plane)                                    # the whole plane below thre_hmp
                elif j >= P - n_sub:
                    s = (P - j) / float(d_sub)                                      # in (0, thre_hmp)
                else:
                    s = (P - j + 23) / float(d_top)
                hm[n, c, y, x] = s
    assert float(hm.max()) <= 1.0 and n_sub / d_sub < THRE and P / d_plane < THRE and (n_sub + 24) / d_top >= THRE
    h4, w4 = H // 4, W // 4
    off = _dyadic(seed + 1, (N_IMAGES, L, nd, h4, w4), -48, 47, 4)                   # multiples of 1/4 in [-12, 12)
    y0, x0 = common[0] // 4, common[1] // 4
    off[0, :, :, y0 - 1:y0 + 3, x0 - 1:x0 + 3] = 0.0                                # guide point = the common pixel itself
    off[:, TIE_LIMB] = 0.0
    for l, (ox, oy) in ((NEG_LIMB, (-0.5, -0.5)), (OUT_LIMB, (8.5, -0.25))):
        off[:, l, 0::2], off[:, l, 1::2] = ox, oy
    out = dict(hm_hr=hm, off_lr=np.ascontiguousarray(off.reshape(N_IMAGES, L * nd, h4, w4)), scl_lr=None, jit_lr=None)
    if case.heads in ('scale', 'both'):
        out['scl_lr'] = _dyadic(seed + 2, (N_IMAGES, C, h4, w4), 4, 131, 4)          # 1 .. 32.75
    if case.heads in ('jitter', 'both'):
        out['jit_lr'] = _dyadic(seed + 3, (N_IMAGES, 2, h4, w4), -16, 15, 8)         # -2 .. 1.875
    return out


def input_arrays(scene):
    return [scene[k] for k in ('hm_hr', 'off_lr', 'scl_lr', 'jit_lr') if scene[k] is not None]


# ---------------------------------------------------------------------------------- coverage
def count(case, cond, scores, inds, limbs, off_hr, jit_hr=None, scl_hr=None):
    """Occurrences of `cond` in the reference's intermediate values: its top-k lists (N,C,K), its limbs (N,L,K,13), the x4 bilinear
    offsets (N,nd*L,H,W), jitter maps (N,2,H,W) and scale maps (N,17,H,W) it was given."""
    sk, K, H, W, nd = skeleton(case), case.K, case.H, case.W, case.nd
    jf, jt = [a for a, _ in sk], [b for _, b in sk]
    s1, s2 = limbs[..., 2], limbs[..., 5]
    ok1, ok2 = s1 >= np.float32(THRE), s2 >= np.float32(THRE)
    if cond in ('fallback_taken', 'last_in_launch'):   # from the restated plan, not from the kernel: a moved limit fails here
        here, nxt = plan(N_IMAGES, 17, H, W, K).route, plan(N_IMAGES, 17, *smallest_plane(K + 1), K + 1).route
        return int(here == 'fallback') if cond == 'fallback_taken' else int(here == 'in_launch' and nxt == 'fallback')
    if cond == 'rows_past_switch':   # rows with both ends above the threshold at the ranks only a k past the switch has
        return int((ok1 & ok2)[:, :, FALLBACK_K:].sum())
    if cond == 'sub_from':
        return int((~ok1).sum())
    if cond == 'sub_to_list':        # an above-threshold from-candidate whose nearest to-candidate lies below it: the whole list does
        return int((ok1 & ~ok2).sum())
    if cond == 'min_len':
        return int((ok1 & ok2 & (limbs[..., 9] == np.float32(MIN_LEN))).sum())
    i_f = inds[:, jf].astype(np.int64)                                   # (N,L,K)
    xf, yf = i_f % W, i_f // W
    if cond == 'border_from':
        return int((ok1 & ((xf == 0) | (xf == W - 1) | (yf == 0) | (yf == H - 1))).sum())
    if cond == 'border_to':
        i2 = limbs[..., 7].astype(np.int64) % (H * W)
        x2, y2 = i2 % W, i2 // W
        return int((ok2 & ((x2 == 0) | (x2 == W - 1) | (y2 == 0) | (y2 == H - 1))).sum())
    # guide points (collect.py:152), before the jitter refinement
    shift = np.where(scores[:, jf] < np.float32(THRE), 100000, 0)
    o = off_hr.reshape(off_hr.shape[0], len(sk), nd, H * W)
    g = [(xf - shift if c % 2 == 0 else yf - shift).astype(np.float32) + np.take_along_axis(o[:, :, c], i_f, axis=2) for c in range(nd)]
    if cond in ('second_candidate', 'k64_taps_differ'):   # rows of a lane's LATER from-candidates (k >= 64) whose offset taps differ
        #                                                    from those of its first; k64_taps_differ: on the limbs only omp44 has
        taps = np.stack([np.take_along_axis(o[:, :, c], i_f, axis=2) for c in range(nd)], -1)[:, 19 if cond == 'k64_taps_differ' else 0:]
        first = taps[:, :, np.arange(64, K) % 64]
        return int((taps[:, :, 64:] != first).any(-1).sum()) if K > 64 else 0
    gx, gy = g[0], g[1]
    qx, qy = np.trunc(gx).astype(np.int64), np.trunc(gy).astype(np.int64)
    gate = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)

    def squares(px, py, nd=nd):      # exact squared match distance of every row to the point(s) (px, py): dyadic values, fp64
        r = g
        if jit_hr is not None:       # the guide point as refined at [x][y] (collect.py:158-165)
            nn = np.arange(limbs.shape[0])[:, None, None]
            r = [np.where(gate, g[c] + jit_hr[nn, c, np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)], g[c]) for c in range(2)]
        return sum((r[c].astype(np.float64)[..., None] - (px if c % 2 == 0 else py)) ** 2 for c in range(nd))
    if cond in ('tie', 'origin_nearest'):
        i_t = inds[:, jt].astype(np.int64)
        sh_t = np.where(scores[:, jt] < np.float32(THRE), 100000, 0)
        d2 = squares((i_t % W - sh_t).astype(np.float64)[:, :, None, :], (i_t // W - sh_t).astype(np.float64)[:, :, None, :])
        d2 = np.partition(d2, 1, axis=-1) if K >= 2 else d2          # [..., 0] and [..., 1]: the two smallest, as sorted
        if cond == 'tie':            # the two smallest distances are equal and belong to above-threshold candidates
            return int((ok1 & (d2[..., 0] == d2[..., 1]) & (d2[..., 0] < 1e8)).sum()) if K >= 2 else 0
        # the guide point lies nearer to the origin than to any to-candidate: a to-list padded with zeros instead of INFINITY
        # (K is no multiple of 4) would match its padding
        return int((squares(0.0, 0.0)[..., 0] < d2[..., 0]).sum())
    if cond == 'guide_neg':          # a coordinate in (-1, 0): truncation admits it, a floor would not
        return int((gate & (((gx > -1) & (gx < 0)) | ((gy > -1) & (gy < 0)))).sum())
    if cond == 'guide_x_ge_w':
        return int((ok1 & (gx >= W)).sum())
    if cond == 'jitter_xy':          # admitted lookups at [x][y], x != y, where [y][x] holds another vector
        nn = np.arange(limbs.shape[0])[:, None, None]
        a = jit_hr[nn, :, np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)]
        b = jit_hr[nn, :, np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
        return int((gate & (qx != qy) & (a != b).any(-1)).sum())
    if cond == 'both_heads_move':    # the jitter moves the guide point AND the scale column is not the head-less row's 4
        nn = np.arange(limbs.shape[0])[:, None, None]
        a = jit_hr[nn, :, np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)]
        return int((ok1 & gate & (a != 0).any(-1) & (limbs[..., 11] != 4) & (limbs[..., 12] != 4)).sum())
    if cond == 'scale_differs_on_cat':   # rows matched to another to-candidate than components 0-1 alone would choose, whose scale
        #                                  differs: column 12 is right only if all four components entered the distance
        i_t = inds[:, jt].astype(np.int64)
        sh_t = np.where(scores[:, jt] < np.float32(THRE), 100000, 0)
        px, py = ((i_t % W - sh_t).astype(np.float64)[:, :, None, :], (i_t // W - sh_t).astype(np.float64)[:, :, None, :])
        a4, a2 = squares(px, py).argmin(-1), squares(px, py, 2).argmin(-1)
        nn, cc = np.arange(limbs.shape[0])[:, None, None], np.array(jt)[None, :, None]
        s_of = lambda a: scl_hr.reshape(scl_hr.shape[0], 17, -1)[nn, cc, np.take_along_axis(i_t, a, axis=2)]  # noqa: E731
        assert (s_of(a4)[ok1 & ok2] == limbs[..., 12][ok1 & ok2]).all()
        return int((ok1 & ok2 & (a4 != a2) & (s_of(a4) != s_of(a2))).sum())
    raise KeyError(cond)


def counts(case, scores, inds, limbs, off_hr, jit_hr=None, scl_hr=None):
    return {c: count(case, c, scores, inds, limbs, off_hr, jit_hr, scl_hr) for c in conditions(case)}


# ---------------------------------------------------------------------------------- fused forms (stride-4 heat maps)
FUSED_K = (7, 33, 65)


def bump_heatmaps(K, h=16, w=16):
    """Stride-4 heat maps (4,17,h,w) of [images | other images]: single-cell bumps on a stride-2 lattice whose phase changes with the
    plane, 40 per plane, dyadic amplitudes in [1/4, 1) -- the heat maps of build_fused, for any size."""
    seed = 9500 + K
    hm = np.zeros((2 * N_IMAGES, 17, h, w), np.float32)
    for n in range(2 * N_IMAGES):
        for c in range(17):
            cells = [(y, x) for y in range(c % 2, h, 2) for x in range((c // 2) % 2, w, 2)]
            order = np.argsort(synth.HashRng(seed + 100 * n + c).uniform(len(cells)), kind='stable')
            for j, i in enumerate(order[:40]):
                hm[n, c, cells[i][0], cells[i][1]] = (32 + 2 * j + (n % 2)) / 128.0
    return hm


def build_fused(K):
    """Head outputs of [images | other images] at 64 x 64 input for the forms that start from stride-4 heat maps, where peaks cannot
    be planted exactly: single-cell bumps on a stride-2 lattice of the 16 x 16 map (corners, edges, interior; the lattice's phase
    changes with the plane so that row / column 15 are met too), 40 per plane, dyadic amplitudes in [1/4, 1).
    -> hm_pair (4,17,16,16), off_pair (4,38,16,16), scl_pair (4,17,16,16), jit_pair (4,2,16,16)"""
    seed, h = 9500 + K, 16
    hm = bump_heatmaps(K)
    off = _dyadic(seed + 1, (2 * N_IMAGES, 38, h, h), -48, 47, 4)
    scl = _dyadic(seed + 2, (2 * N_IMAGES, 17, h, h), 4, 131, 4)
    jit = _dyadic(seed + 3, (2 * N_IMAGES, 2, h, h), -16, 15, 8)
    return hm, off, scl, jit


# ---------------------------------------------------------------------------------- the stored reference output
def modes(case):
    """The x4 resize modes of the scale maps the case is stored for ('none': no scale head)."""
    return ('bicubic', 'bilinear') if case.heads in ('scale', 'both') else ('none',)


def exact_digest(limbs):
    """SHA-256 of the EXACT_LIMB_COLS of (N,L,K,13) limbs, what the fixture holds of a DIGEST case."""
    from helpers import EXACT_LIMB_COLS, sha
    return sha(np.asarray(limbs, np.float32)[..., EXACT_LIMB_COLS])


def lists_digest(scores, inds):
    from helpers import sha
    return sha(np.asarray(scores, np.float32)) + sha(np.asarray(inds, np.int64))


def oracle_rows(case, scene):
    """The C oracle on the case: its lists and, per mode of `modes`, its pairing on the stride-4 offsets."""
    import oracle
    sc, idx, _, _ = oracle.nms_topk(scene['hm_hr'], case.K)
    jit_hr = oracle.bilinear4(scene['jit_lr']) if scene['jit_lr'] is not None else None
    exp = dict(scores=sc, inds=idx)
    for mode in modes(case):
        scl_hr = None if mode == 'none' else (oracle.bicubic4 if mode == 'bicubic' else oracle.bilinear4)(scene['scl_lr'])
        exp['limbs' if mode == 'none' else f'limbs_{mode}'] = oracle.collect_limbs(
            sc, idx, scene['off_lr'], True, (case.H, case.W), skeleton(case), THRE, MIN_LEN, vector_nd=case.nd, scales_hr=scl_hr,
            jitter_hr=jit_hr)
    return exp


def load(name):
    """-> case, scene (inputs regenerated, sha-guarded), expected dict(scores, inds, limbs (N,L,K,13); with a scale head: limbs_bicubic,
    limbs_bilinear instead of limbs) from tests/golden/pairing_edges.npz (tools/gen_golden_pairing.py).  A STORED case: the reference's
    own arrays.  A DIGEST case: the C oracle's rows, computed once per process and held here to the stored SHA-256 of the reference's
    lists and of its EXACT_LIMB_COLS (the generator also held the oracle's score column within 1e-4 of the reference's); read-only."""
    import os
    from helpers import GOLDEN, sha
    global _FIXTURE
    if _FIXTURE is None:
        _FIXTURE = np.load(os.path.join(GOLDEN, 'pairing_edges.npz'))
    g, case = _FIXTURE, BY_NAME[name]
    if name in _LOADED:
        return _LOADED[name]
    scene = build(case)
    if case in DIGEST:
        d = dict(line.decode().split(' ', 1) for line in g['digests'])
        assert [sha(a) for a in input_arrays(scene)] == d[f'{name}/in_sha'].split(','), "scene generator drifted (not a parity failure)"
        exp = oracle_rows(case, scene)
        assert lists_digest(exp['scores'], exp['inds']) == d[f'{name}/lists_sha'], "the oracle's lists are not the reference's"
        for mode in modes(case):
            key = 'limbs' if mode == 'none' else f'limbs_{mode}'
            assert exact_digest(exp[key]) == d[f'{name}/{key}_sha'], f"the oracle's rows are not the reference's ({mode})"
        if case.heads in ('scale', 'both'):   # the scene of a STORED case + scale maps: every column but 11 / 12 is the REFERENCE's own
            #                                   stored one, its score column included (the generator asserts that only 11 / 12 differ)
            base = np.ascontiguousarray(np.moveaxis(g[f"{'cat' if case.nd == 4 else 'jitter'}_k{case.K}/limbs"], 0, -1))
            for mode in modes(case):
                rows, ref = exp[f'limbs_{mode}'], base.copy()
                assert (np.delete(rows, [10, 11, 12], -1) == np.delete(base, [10, 11, 12], -1)).all()
                ref[..., 11:13] = rows[..., 11:13]                     # bit-equal to the reference's: held by the digest above
                if name in SCALES_STORED:
                    ref[..., 11:13] = np.moveaxis(g[f'{name}/scales_{mode}'], 0, -1)
                    assert (ref[..., 11:13] == rows[..., 11:13]).all()
                exp[f'limbs_{mode}'] = ref
        for a in exp.values():
            a.flags.writeable = False
        _LOADED[name] = case, scene, exp
        return _LOADED[name]
    assert [sha(a) for a in input_arrays(scene)] == list(g[f'{name}/in_sha']), "scene generator drifted (not a parity failure)"
    src = name if case.heads != 'scale' else f'plain_k{case.K}'
    limbs = np.ascontiguousarray(np.moveaxis(g[f'{src}/limbs'], 0, -1))
    exp = dict(scores=g[f'{src}/scores'], inds=g[f'{src}/inds'].astype(np.int64))
    if case.heads == 'scale':
        for mode in ('bicubic', 'bilinear'):
            exp[f'limbs_{mode}'] = limbs.copy()
            exp[f'limbs_{mode}'][..., 11:13] = np.moveaxis(g[f'{name}/scales_{mode}'], 0, -1)
    else:
        exp['limbs'] = limbs
    return case, scene, exp


_FIXTURE, _LOADED = None, {}
