"""The pose painter's specification (og_draw_poses_u8, include/og_decoder.h) restated in numpy, and the cases the CPU and GPU tests share.

`draw_reference` is written from the specification, not from the kernel: no tiles, no culling -- every primitive is evaluated on the
whole image -- and ONE numpy operation per arithmetic operation, so that dtype=np.float32 reproduces every rounding of the kernel
(numpy's +, -, *, / and sqrt are correctly rounded, as the kernel's are) and dtype=np.float64 is the check of the restatement itself.
`skeleton` is given as draw_poses takes it (config.COCO_PERSON_SKELETON: index pairs from 0)."""
import numpy as np

from offsetguided_amd.config import coco_data as cd

COCO = [tuple(c) for c in cd.COCO_PERSON_SKELETON]      # K = 17, L = 19
TOY = [(0, 1), (1, 2)]                                  # K = 3, L = 2
LIST_CAP = 512                                          # entries of the kernel's LDS list (csrc/draw.hip)


def draw_reference(images, poses, n_persons, skeleton, palette, line_width, marker_radius, alpha, dtype):
    """images (N,H,W,3) uint8, poses (N,P,K,>=3) float32 rows x, y, v, n_persons (N), palette (n_colors,3) uint8 -> painted copy."""
    T = dtype
    images, poses, palette = np.asarray(images), np.asarray(poses, dtype=np.float32), np.asarray(palette, dtype=np.uint8)
    N, H, W, _ = images.shape
    K = poses.shape[2]
    out = images.copy()
    PX = np.broadcast_to(np.arange(W, dtype=T)[None, :], (H, W))     # the centre of the pixel in column i, row j is (i, j)
    PY = np.broadcast_to(np.arange(H, dtype=T)[:, None], (H, W))
    half, zero, one, alpha = T(0.5), T(0), T(1), T(np.float32(alpha))
    r_line, r_mark = T(np.float32(line_width)) / T(2), T(np.float32(marker_radius))
    with np.errstate(all='ignore'):
        for n in range(N):
            c = [images[n, :, :, ch].astype(T) for ch in range(3)]
            touched = np.zeros((H, W), bool)
            for p in range(int(n_persons[n])):
                colour = palette[p % len(palette)].astype(T)
                prims = [(a, b, r_line) for a, b in skeleton] + [(k, k, r_mark) for k in range(K)]
                for a, b, r in prims:
                    ax, ay, av = (T(v) for v in poses[n, p, a, :3])
                    bx, by, bv = (T(v) for v in poses[n, p, b, :3])
                    if not (av > 0 and bv > 0 and np.isfinite(ax) and np.isfinite(ay) and np.isfinite(bx) and np.isfinite(by)):
                        continue
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


def _base(N, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (N, H, W, 3), dtype=np.uint8)


def _random_poses(rng, N, P, K, H, W, margin=10.0):
    """Poses spread over the image and up to `margin` px outside it on every side; every keypoint visible."""
    xy = rng.uniform([-margin, -margin], [W - 1 + margin, H - 1 + margin], (N, P, K, 2))
    return np.concatenate([xy, rng.uniform(0.1, 1.0, (N, P, K, 1))], axis=3).astype(np.float32)


def cases():
    """name -> dict(images, poses, n_persons, skeleton, palette, line_width, marker_radius, alpha): the smallest shapes at which the
    kernel can go wrong (32 x 8 tiles, 64-lane waves, a 512-entry list filled in rounds of 256)."""
    from offsetguided_amd.visualization import TAB20
    out = {}
    rng = np.random.default_rng(11)
    # partial tiles: W and H no multiples of the tile, poses reaching outside the image
    out['partial_tiles'] = dict(images=_base(2, 19, 45, 1), poses=_random_poses(rng, 2, 3, 17, 19, 45), n_persons=[3, 3], skeleton=COCO,
                                palette=TAB20, line_width=2.0, marker_radius=3.0, alpha=1.0)
    # tile and wave seams: segments exactly on tile borders, one long diagonal across every tile
    seams = np.zeros((1, 5, 3, 3), np.float32)
    seams[0, :, :, 2] = 1.0
    seams[0, 0, :, :2] = [(2.0, 7.5), (50.0, 7.5), (93.0, 7.5)]        # between tile rows 0 and 1
    seams[0, 1, :, :2] = [(3.0, 8.0), (60.0, 8.0), (95.0, 8.0)]        # on the first row of tile row 1
    seams[0, 2, :, :2] = [(31.5, 1.0), (31.5, 12.0), (31.5, 23.0)]     # between tile columns 0 and 1
    seams[0, 3, :, :2] = [(32.0, 0.0), (32.0, 15.5), (64.0, 15.5)]     # on the first column of tile column 1, then a row seam
    seams[0, 4, :, :2] = [(0.0, 0.0), (47.0, 11.0), (95.0, 23.0)]      # the diagonal
    out['seams'] = dict(images=_base(1, 24, 96, 2), poses=seams, n_persons=[5], skeleton=TOY, palette=TAB20, line_width=1.0,
                        marker_radius=0.5, alpha=0.5)
    # masked inputs: v = 0, v < 0, NaN / inf coordinates, zero-length limbs, an image without persons, garbage in unused rows
    masked = _random_poses(rng, 3, 4, 17, 19, 45)
    masked[0, 0, 3, 2] = 0.0
    masked[0, 0, 5, 2] = -1.0
    masked[0, 1, 6, 0] = np.nan
    masked[0, 1, 7, 1] = np.inf
    masked[0, 2, 8, 0] = -np.inf
    masked[0, 2, 1] = masked[0, 2, 0]                                   # limb (0, 1) of zero length
    masked[0, 3] = masked[0, 3, :1]                                     # a whole person on one point
    masked[2, 2:] = [np.nan, 1e30, 1.0]                                 # unused rows: n_persons[2] = 2
    out['masked'] = dict(images=_base(3, 19, 45, 3), poses=masked, n_persons=[4, 0, 2], skeleton=COCO, palette=TAB20, line_width=2.0,
                         marker_radius=3.0, alpha=1.0)
    # order and overflow: LIST_CAP + 70 primitives over one tile (persons stacked on one spot, jittered), alpha 0.5, 7 colours
    n_prims = LIST_CAP + 70
    P = -(-n_prims // 5)
    stack = np.zeros((1, P, 3, 3), np.float32)
    stack[0, :, :, :2] = np.array([(36.0, 2.0), (44.0, 5.0), (56.0, 3.0)]) + rng.uniform(-1.5, 1.5, (P, 3, 2))
    stack[0, :, :, 2] = 1.0
    stack[0, P - 1, :, 2] = [1.0, 0.0, 1.0]                             # the last person: two discs, no limb -> exactly n_prims
    assert 5 * (P - 1) + 2 == n_prims
    out['overflow'] = dict(images=_base(1, 16, 64, 4), poses=stack, n_persons=[P], skeleton=TOY, palette=TAB20[:7], line_width=2.0,
                           marker_radius=3.0, alpha=0.5)
    # parameters: line_width {1, 2, 5} x marker_radius {0.5, 3} x alpha {1, 0.5}, a palette of one colour, both skeletons
    toy = _random_poses(rng, 1, 3, 3, 19, 45, margin=4.0)
    coco = _random_poses(rng, 1, 2, 17, 19, 45, margin=4.0)
    one_colour = np.array([[250, 20, 130]], np.uint8)
    for lw in (1.0, 2.0, 5.0):
        for mr in (0.5, 3.0):
            for al in (1.0, 0.5):
                coco_turn = (lw, mr, al) in ((5.0, 0.5, 0.5), (1.0, 3.0, 1.0))
                out[f'params_lw{lw:g}_mr{mr:g}_a{al:g}'] = dict(
                    images=_base(1, 19, 45, 5), poses=coco if coco_turn else toy, n_persons=[2 if coco_turn else 3],
                    skeleton=COCO if coco_turn else TOY, palette=one_colour if lw == 2.0 else TAB20, line_width=lw, marker_radius=mr,
                    alpha=al)
    return out


_REFERENCE = {}


def reference(name, dtype=np.float32):
    """The restatement's result for a case, computed once per process and handed out read-only."""
    key = (name, np.dtype(dtype).name)
    if key not in _REFERENCE:
        ref = draw_reference(dtype=dtype, **CASES[name])
        ref.setflags(write=False)
        _REFERENCE[key] = ref
    return _REFERENCE[key]


CASES = cases()
