"""Numpy restatement of the augmentation kernels' specification (csrc/augment.hip header, include/og_decoder.h), written from the
specification text: integer operations in np.int32 / np.int64, float64 with explicit products and sums.  Shared by
tests/test_augment_cpu.py and tests/test_gpu_augment.py, and the cases both walk."""
import math
import os
import random

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'augment_affine.npz')
BORDER = (124, 116, 104)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
LEFT = [1, 3, 5, 7, 9, 11, 13, 15]
RIGHT = [2, 4, 6, 8, 10, 12, 14, 16]
SIZES = ((48, 80), (97, 61), (33, 35))         # (h, w) of the three sources of a GPU batch


def tap_table():
    """Specification step 2 -> (32, 4) int32: every operation one fp32 operation, left to right."""
    f = np.float32
    A, one = f(-0.75), f(1)
    table = np.zeros((32, 4), np.int32)
    for p in range(32):
        x = f(p) / f(32)
        c0 = ((A * (x + one) - f(5) * A) * (x + one) + f(8) * A) * (x + one) - f(4) * A
        c1 = ((A + f(2)) * x - (A + f(3))) * x * x + one
        c2 = ((A + f(2)) * (one - x) - (A + f(3))) * (one - x) * (one - x) + one
        c3 = one - c0 - c1 - c2
        t = [int(np.rint(c * f(2048))) for c in (c0, c1, c2, c3)]
        t[t.index(max(t))] += 2048 - sum(t)        # list.index: the first of equal taps
        table[p] = t
    return table


TAPS = tap_table()


def source_coords(D, S):
    """Specification step 1 -> (sx, px, sy, py), each (S, S) int32 indexed [y, x]."""
    D = np.asarray(D, np.float64).reshape(2, 3)
    x = np.arange(S, dtype=np.float64)
    y = np.arange(S, dtype=np.float64)
    out = []
    for m0, m1, m2 in D:
        col = np.rint((m0 * x) * 1024.0)
        row = np.rint(((m1 * y) + m2) * 1024.0)
        assert np.abs(col).max() < 2 ** 31 and np.abs(row).max() < 2 ** 31
        X = col.astype(np.int32)[None, :] + row.astype(np.int32)[:, None] + np.int32(16)
        X = X >> 5
        out += [X >> 5, X & 31]
    return out


def warp_u8(src, D, S, border):
    """src (h, w, C) or (h, w) uint8 -> (S, S, C) / (S, S) uint8: specification steps 1-4."""
    planes = src.ndim == 2
    src = src[:, :, None] if planes else src
    h, w, C = src.shape
    border = np.asarray(border, np.int64).reshape(-1)
    sx, px, sy, py = source_coords(D, S)
    wx, wy = TAPS[px].astype(np.int64), TAPS[py].astype(np.int64)          # (S, S, 4)
    acc = np.zeros((S, S, C), np.int64)
    for j in range(4):
        r = sy - 1 + j
        for i in range(4):
            q = sx - 1 + i
            inside = (r >= 0) & (r < h) & (q >= 0) & (q < w)
            val = src[np.clip(r, 0, h - 1), np.clip(q, 0, w - 1)].astype(np.int64)     # (S, S, C); replaced where outside
            val = np.where(inside[..., None], val, border[None, None, :])
            acc += val * (wx[..., i] * wy[..., j])[..., None]
    assert np.abs(acc).max() + (1 << 21) < 2 ** 31, 'the int32 sum of the specification would overflow'
    v = np.clip((acc + (1 << 21)) >> 22, 0, 255).astype(np.uint8)
    return v[:, :, 0] if planes else v


def normalize(v, mean=MEAN, std=STD):
    """(S, S, 3) uint8 -> (3, S, S) fp32 = (v / 255 - mean) / std, every operation in fp32 in this order."""
    f = v.astype(np.float32).transpose(2, 0, 1)
    m = np.asarray(mean, np.float32)[:, None, None]
    s = np.asarray(std, np.float32)[:, None, None]
    return ((f / np.float32(255)) - m) / s


def affine_joints(joints, n_persons, M, flip, scale, S_w, S_h, left=LEFT, right=RIGHT):
    """og_affine_joints_f32 for one image: joints (P, K, 4) fp32 -> (P, K, 4) fp32."""
    joints = np.asarray(joints, np.float32)
    M = np.asarray(M, np.float64).reshape(2, 3)
    out = joints.copy()
    use = joints[:n_persons]
    x, y = use[:, :, 0].astype(np.float64), use[:, :, 1].astype(np.float64)
    t = use.copy()
    t[:, :, 0] = (((M[0, 0] * x) + (M[0, 1] * y)) + M[0, 2]).astype(np.float32)
    t[:, :, 1] = (((M[1, 0] * x) + (M[1, 1] * y)) + M[1, 2]).astype(np.float32)
    t[:, :, 3] = (use[:, :, 3].astype(np.float64) * np.float64(scale)).astype(np.float32)
    if flip:
        perm = np.arange(joints.shape[1])
        perm[left], perm[right] = right, left
        t = t[:, perm]
    gone = (t[:, :, 0] <= 0) | (t[:, :, 1] <= 0) | (t[:, :, 0] > np.float32(S_w)) | (t[:, :, 1] > np.float32(S_h))
    t[:, :, 2] = np.where(gone, np.float32(0), t[:, :, 2])
    out[:n_persons] = t
    return out


def inverse_rows(M):
    return np.linalg.inv(np.asarray(M, np.float64).reshape(3, 3))[0:2]


# ---------------------------------------------------------------------------------------------------------------------- cases
def source_images(seed=5):
    """Three noise images with a gradient and their mask planes (0 / 255 blocks), sizes SIZES."""
    rng = np.random.RandomState(seed)
    images, masks = [], []
    for h, w in SIZES:
        im = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        im[h // 4:h // 2, w // 4:w // 2] = 255                       # saturated block: the cubic overshoots beside it (clamp at 255 / 0)
        im[h // 2:3 * h // 4, w // 2:3 * w // 4] = 0
        images.append(im)
        m = np.full((h, w), 255, np.uint8)
        m[h // 3:2 * h // 3, w // 5:w // 2] = 0
        masks.append(m)
    return images, masks


def _mat(flip=False, rotate=0.0, sx=1.0, sy=1.0, tx=0.0, ty=0.0, h=0, w=0, S=0):
    """Forward matrix about the centres, built here from scratch (not through the package): rotate, scale, flip, translate."""
    c, s = math.cos(rotate / 180 * math.pi), math.sin(rotate / 180 * math.pi)
    to0 = np.array([[1, 0, -(w - 1) / 2], [0, 1, -(h - 1) / 2], [0, 0, 1.]])
    rot = np.array([[c, s, 0], [-s, c, 0], [0, 0, 1.]])
    scl = np.diag([sx, sy, 1.])
    flp = np.diag([-1. if flip else 1., 1., 1.])
    back = np.array([[1, 0, (S - 1) / 2 + tx], [0, 1, (S - 1) / 2 + ty], [0, 0, 1.]])
    return back @ flp @ scl @ rot @ to0


def fixed_cases(S):
    """name -> three forward matrices (one per source of SIZES) for destination side S."""
    ident = np.eye(3)
    shift = np.array([[1, 0, 7.], [0, 1, -3.], [0, 0, 1.]])
    cases = {
        'identity': [ident] * 3,
        'integer_translation': [shift] * 3,
        'flip': [_mat(flip=True, h=h, w=w, S=S) for h, w in SIZES],
        'rotate45_scale_half': [_mat(rotate=45, sx=0.5, sy=0.5, h=h, w=w, S=S) for h, w in SIZES],
        'scale2_stretch': [_mat(sx=2.0 * 0.95, sy=2.0 * 1.05, h=h, w=w, S=S) for h, w in SIZES],
        'all_border': [np.array([[1, 0, 5000.], [0, 1, 5000.], [0, 0, 1.]])] * 3,
        # fractional shifts that put the source's left / top, then right / bottom edge inside the square: 4 x 4 windows straddle all four
        'straddle_edges': [np.array([[1, 0, 10.3], [0, 1, 9.6], [0, 0, 1.]]),
                           np.array([[1, 0, -40.7], [0, 1, -60.4], [0, 0, 1.]]),
                           _mat(rotate=13, sx=1.1, sy=0.9, tx=2.5, ty=-1.5, h=SIZES[2][0], w=SIZES[2][1], S=S)],
    }
    return cases


def random_cases(S, n=20):
    """n seeds of the default random draws -> per seed three matrices through the reference-shaped host code of the package."""
    from offsetguided_amd import transforms
    out = []
    for seed in range(n):
        rng = random.Random(1000 + seed)
        t = transforms.WarpAffineTransforms(S, aug_params=transforms.AugParams())
        mats = []
        for h, w in SIZES:
            wh = np.array([w, h])
            mats.append(t.affine_matrix(t.draw(rng), np.array([w // 2, h // 2], np.float32), wh))
        out.append(mats)
    return out
