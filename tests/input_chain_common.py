"""Cases and reference of the input chain (csrc/preprocess.hip: og_rescale_pad_normalize_u8, og_rescale_pad_normalize_batch_u8,
og_resize_cubic_u8, og_shrink_mask_miss_u8; csrc/epilogue.hip: og_center_pad_normalize_u8).  No GPU code is imported here.
Shared by tests/test_input_chain_cpu.py and tests/test_gpu_input_chain.py.

The reference of a fused launch is a composition of things pinned elsewhere: oracle.resize_cubic_u8 per image, pasted into a uint8
canvas of transforms.pad.FILL at CenterPad's (or RightDownPad's) position, then ToTensor + Normalize in fp32 torch on the CPU.  Every
comparison is bit for bit.

The fused kernel has two bodies per workgroup: taps read from an LDS image of the tile's source footprint, or straight from global
memory.  WHICH ONE A LAUNCH TOOK CANNOT BE OBSERVED FROM OUTSIDE: `takes_lds` restates the launcher's expression on the host, and
that restatement is the only evidence that a case labelled 'lds' or 'direct' covers that body.  tests/test_input_chain_cpu.py holds
its constants to the constexpr line of the source and every label of the table to it."""
import functools
from collections import namedtuple

import numpy as np
import torch

from offsetguided_amd.config import data_mean, data_std
from offsetguided_amd.transforms.pad import FILL

TILE_W, TILE_H, LDS_BYTES = 64, 4, 24 * 1024          # kPrepTW, kPrepTH, kPrepLds


# ------------------------------------------------------------------------------------------------------------- the path decision
def estimate(h, w, nh, nw):
    """(fw, fh) of the launcher: (long)(kPrepTW * sx) + 8, (long)(kPrepTH * sy) + 8 with sx = (double)w / nw, sy = (double)h / nh."""
    return int(TILE_W * (w / nw)) + 8, int(TILE_H * (h / nh)) + 8


def takes_lds(h, w, nh, nw):
    fw, fh = estimate(h, w, nh, nw)
    return fw * fh * 3 <= LDS_BYTES


def label_of(h, w, nh, nw):
    return 'lds' if takes_lds(h, w, nh, nw) else 'direct'


# -------------------------------------------------------------------------------------------------------- the staged footprint
def tap_start(d, scale):
    """cubic_taps(d, scale).i0: f = float32((d + 0.5) * scale - 0.5) (the product and the difference in double), floor(f) - 1."""
    f = ((np.asarray(d, np.float64) + 0.5) * np.float64(scale) - 0.5).astype(np.float32)
    return np.floor(f).astype(np.int64) - 1


def pad_left_top(nh, nw, TH, TW, corner):
    return (0, 0) if corner else (int((TW - nw) / 2.0), int((TH - nh) / 2.0))


def _axis_footprints(n_src, n_new, target, tile, lead):
    """Staged extent (pixels) of every tile along one axis that holds a pixel of the resized image: i0(b) + 3 - i0(a) + 1."""
    scale = n_src / n_new
    out = []
    for t in range((target + tile - 1) // tile):
        a, b = max(t * tile - lead, 0), min(t * tile + tile - 1 - lead, n_new - 1)
        if a <= b:
            out.append(int(tap_start(b, scale)) + 3 - int(tap_start(a, scale)) + 1)
    return out


def tile_footprints(h, w, nh, nw, TH, TW, corner):
    """(widths lw per tile column, heights lh per tile row) of the LDS images the kernel stages for this case; a tile (tx, ty) stages
    lh[ty] * lw[tx] * 3 bytes, so the largest image of the case is max(lh) * max(lw) * 3."""
    left, top = pad_left_top(nh, nw, TH, TW, corner)
    return _axis_footprints(w, nw, TW, TILE_W, left), _axis_footprints(h, nh, TH, TILE_H, top)


# ------------------------------------------------------------------------------------------------------------------- the images
KINDS = ('noise', 'salt', 'index')


@functools.lru_cache(maxsize=None)
def image(kind, h, w, seed=0):
    """Deterministic (h, w, 3) uint8: uniform noise; 0 / 255 salt and pepper (the cubic overshoot saturates at both ends); or channels
    x % 251, y % 251, (x + y) % 256 (an off-by-one tap or clamp reads as a coordinate).  Cached: never written to."""
    rng = np.random.default_rng([seed, h, w, KINDS.index(kind)])
    if kind == 'noise':
        im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif kind == 'salt':
        im = (rng.random((h, w, 3)) > 0.4).astype(np.uint8) * 255
    else:
        y, x = np.mgrid[:h, :w]
        im = np.stack([x % 251, y % 251, (x + y) % 256], 2).astype(np.uint8)
    return im


# ---------------------------------------------------------------------------------------------------------------- the reference
_MEAN, _STD = torch.tensor(data_mean).view(3, 1, 1), torch.tensor(data_std).view(3, 1, 1)


def normalize(canvas):
    """ToTensor + Normalize of an (H, W, 3) uint8 canvas -> (3, H, W) fp32, the arithmetic tests/test_transforms.py holds the kernels to."""
    return (torch.from_numpy(np.ascontiguousarray(canvas)).permute(2, 0, 1).float().div(255) - _MEAN) / _STD


@functools.lru_cache(maxsize=None)
def resized(kind, h, w, nh, nw, seed=0):
    import oracle
    out = oracle.resize_cubic_u8(image(kind, h, w, seed), nh, nw)
    return out


def paste(res, TH, TW, corner):
    """(normalised (3, TH, TW) tensor, [left, top, right, bottom]) of a resized image padded to the target."""
    nh, nw = res.shape[:2]
    left, top = pad_left_top(nh, nw, TH, TW, corner)
    canvas = np.empty((TH, TW, 3), np.uint8)
    canvas[:] = np.array(FILL, np.uint8)
    canvas[top:top + nh, left:left + nw] = res
    return normalize(canvas), [left, top, TW - nw - left, TH - nh - top]


def expected(kind, h, w, nh, nw, TH, TW, corner, seed=0):
    return paste(resized(kind, h, w, nh, nw, seed), TH, TW, corner)


# --------------------------------------------------------------------------------------------------------------- the case table
Case = namedtuple('Case', 'name h w nh nw TH TW corner label')

# enumerated by limit_pairs() below (tests/test_input_chain_cpu.py re-runs the search): the (source, resized) pairs with the largest
# fw * fh * 3 still <= 24 576, and for each the smallest larger source of the same aspect and target that flips to the direct path
LIMIT_BYTES = 24258                            # fw, fh = 311, 26: the most either aspect reaches
LIMIT_SQUARE = ((90, 90), (19, 19))            # 1 : 1, scale 4.7368
FLIP_SQUARE = ((91, 91), (19, 19))             # scale 4.7895: fw, fh = 314, 27 -> 25 434 bytes
LIMIT_LONG = ((270, 180), (57, 38))            # 3 : 2, the same scale
FLIP_LONG = ((273, 182), (57, 38))
LIMIT_LONG_2 = ((498, 332), (105, 70))         # another maximiser of 3 : 2, with two tile columns and 27 tile rows
FLIP_LONG_2 = ((501, 334), (105, 70))
# the bound itself is reachable only anisotropically: sx = 3.875, sy = 6 -> fw, fh = 256, 32 -> exactly 24 576 bytes, still LDS
LIMIT_EXACT = ((192, 124), (32, 32))
FLIP_EXACT = ((200, 124), (32, 32))            # sy = 6.25: fh = 33 -> 25 344 bytes

_BASE = [
    # name, (h, w), (nh, nw), (TH, TW), label                                         every entry is run centre-padded and corner-padded
    # ---- direct path: isotropic 5, 7, 12; more than one tile; anisotropic through the C entry
    ('direct x5', (120, 160), (24, 32), (64, 128), 'direct'),
    ('direct x7', (168, 224), (24, 32), (64, 128), 'direct'),
    ('direct x12', (288, 384), (24, 32), (40, 72), 'direct'),
    ('direct x7 many tiles', (675, 900), (96, 128), (128, 128), 'direct'),
    ('direct x7 residues 1, 1', (600, 900), (86, 126), (128, 256), 'direct'),
    ('direct sx 20 sy 0.5', (16, 640), (32, 32), (64, 64), 'direct'),
    ('direct sy 52 sx 0.5', (1664, 16), (32, 32), (64, 64), 'direct'),
    ('direct sx 52 sy 0.5', (16, 1664), (32, 32), (64, 64), 'direct'),
    # ---- LDS path at its limit, and the neighbours across it
    ('limit square', LIMIT_SQUARE[0], LIMIT_SQUARE[1], (64, 128), 'lds'),
    ('limit square flipped', FLIP_SQUARE[0], FLIP_SQUARE[1], (64, 128), 'direct'),
    ('limit long', LIMIT_LONG[0], LIMIT_LONG[1], (128, 128), 'lds'),
    ('limit long flipped', FLIP_LONG[0], FLIP_LONG[1], (128, 128), 'direct'),
    ('limit long 2', LIMIT_LONG_2[0], LIMIT_LONG_2[1], (128, 128), 'lds'),
    ('limit long 2 flipped', FLIP_LONG_2[0], FLIP_LONG_2[1], (128, 128), 'direct'),
    ('limit exact', LIMIT_EXACT[0], LIMIT_EXACT[1], (36, 64), 'lds'),
    ('limit exact flipped', FLIP_EXACT[0], FLIP_EXACT[1], (36, 64), 'direct'),
    ('lds wide sx 10 sy 0.31', (20, 640), (64, 64), (64, 64), 'lds'),
    ('lds tall sy 20 sx 0.5', (640, 16), (32, 32), (64, 64), 'lds'),
    ('lds x4.5 many tiles', (432, 864), (96, 192), (128, 256), 'lds'),
    # ---- enlargement: the first tap index is -2
    ('3x5 to 128', (3, 5), (76, 128), (128, 128), 'lds'),
    ('17x31 to 128', (17, 31), (70, 128), (128, 128), 'lds'),
    ('31x17 to 128', (31, 17), (128, 70), (128, 128), 'lds'),
    ('exactly x2', (32, 48), (64, 96), (64, 128), 'lds'),
    ('exactly x4', (16, 24), (64, 96), (64, 128), 'lds'),
    ('identity', (64, 96), (64, 96), (64, 128), 'lds'),
    ('identity odd target', (64, 96), (64, 96), (70, 130), 'lds'),
    # ---- sources narrower than the four taps: both clamps act on one pixel
    ('1x1 up', (1, 1), (16, 24), (32, 64), 'lds'),
    ('1x1 same', (1, 1), (1, 1), (8, 64), 'lds'),
    ('1x7 up', (1, 7), (9, 70), (12, 128), 'lds'),
    ('1x7 down', (1, 7), (1, 3), (4, 64), 'lds'),
    ('7x1 up', (7, 1), (70, 9), (128, 64), 'lds'),
    ('7x1 down', (7, 1), (3, 1), (4, 64), 'lds'),
    ('2x2 up', (2, 2), (37, 41), (64, 64), 'lds'),
    ('2x2 down', (2, 2), (1, 1), (4, 64), 'lds'),
    ('3x3 up', (3, 3), (20, 67), (64, 128), 'lds'),
    ('3x3 down', (3, 3), (2, 2), (4, 64), 'lds'),
    ('3x3 to one', (3, 3), (1, 1), (5, 3), 'lds'),
    # ---- resized images of 1x1, 1xN, Nx1 inside a larger target
    ('9x9 to 1x1', (9, 9), (1, 1), (16, 128), 'direct'),
    ('5x40 to 1x20', (5, 40), (1, 20), (16, 128), 'lds'),
    ('40x5 to 20x1', (40, 5), (20, 1), (32, 64), 'lds'),
    ('4x300 to 1x60', (4, 300), (1, 60), (9, 70), 'lds'),
    # ---- padding residues (centre): left % 64 in {0, 1, 63}, top % 4 in {0, 1, 2, 3}; edges on a tile's last / first column and row
    ('left 0 top 0, full', (150, 300), (128, 256), (128, 256), 'lds'),
    ('left 64 top 4, ends on last col, last row', (90, 97), (120, 64), (128, 192), 'lds'),
    ('left 63 top 5, ends on first col', (200, 100), (118, 66), (128, 192), 'lds'),
    ('left 65 top 6', (151, 163), (116, 126), (128, 256), 'lds'),
    ('left 63 top 7', (171, 169), (114, 130), (128, 256), 'lds'),
    ('top 2, ends on first row', (160, 80), (123, 61), (128, 128), 'lds'),
    ('corner: ends on last col, last row', (83, 85), (64, 64), (128, 128), 'lds'),
    ('corner: ends on first col, first row', (84, 86), (65, 65), (128, 128), 'lds'),
    ('direct: ends on last col, first row', (330, 320), (65, 64), (72, 192), 'direct'),
    # ---- targets that are no multiple of the 64 x 4 tile: the X >= TW || Y >= TH exit
    ('target 70x130', (100, 180), (61, 110), (70, 130), 'lds'),
    ('target 130x70', (180, 100), (110, 61), (130, 70), 'lds'),
    ('target 70x130 filled', (75, 140), (70, 130), (70, 130), 'lds'),
    ('target 70x130 direct', (366, 660), (61, 110), (70, 130), 'direct'),
    ('target 1x1', (6, 6), (1, 1), (1, 1), 'direct'),
    ('target 3x65', (20, 400), (3, 65), (3, 65), 'direct'),
]

CASES = [Case(name + (' corner' if corner else ' centre'), h, w, nh, nw, TH, TW, corner, label)
         for name, (h, w), (nh, nw), (TH, TW), label in _BASE for corner in (0, 1)]


def pairs():
    """The table's distinct (h, w, nh, nw), in table order."""
    return list(dict.fromkeys((c.h, c.w, c.nh, c.nw) for c in CASES))


def limit_pairs(aspect_h, aspect_w, max_side=1300, max_target=256):
    """Search of the restatement: sources (aspect_h k, aspect_w k) up to max_side per side, resized to (aspect_h m, aspect_w m) up to
    max_target per side.  -> (best bytes, [(h, w, nh, nw)] that reach it, smallest source first)."""
    best, found = -1, []
    for m in range(1, max_target // max(aspect_h, aspect_w) + 1):
        nh, nw = aspect_h * m, aspect_w * m
        for k in range(1, max_side // max(aspect_h, aspect_w) + 1):
            h, w = aspect_h * k, aspect_w * k
            fw, fh = estimate(h, w, nh, nw)
            b = fw * fh * 3
            if b <= LDS_BYTES and b >= best:
                if b > best:
                    best, found = b, []
                found.append((h, w, nh, nw))
    return best, sorted(found, key=lambda p: (p[0] * p[1], p[2] * p[3]))


def flip_neighbour(h, w, nh, nw, aspect_h, aspect_w):
    """The smallest larger source of the same aspect and resized size that the restatement sends down the direct path."""
    while takes_lds(h, w, nh, nw):
        h, w = h + aspect_h, w + aspect_w
    return h, w


# ------------------------------------------------------------------------------------------------------------------ batch launches
def pack_reversed(images, poison):
    """The images of a launch packed LAST FIRST into one uint8 buffer, with gaps of odd lengths between them and at both ends, every
    byte outside an image = poison.  -> (buffer, byte offsets in image order)."""
    gaps = [777] + [1 + (37 * i) % 101 for i in range(len(images))]
    total = sum(im.size for im in images) + sum(gaps)
    buf = np.full(total, poison, np.uint8)
    offs, o = [0] * len(images), gaps[0]
    for i in reversed(range(len(images))):
        offs[i] = o
        buf[o:o + images[i].size] = images[i].ravel()
        o += images[i].size + gaps[i + 1]
    assert o == total
    return buf, offs


def mixed_launch():
    """One launch's worth of the table: every distinct pair that fits a 250 x 250 target (no multiple of the tile), with its label."""
    return [(h, w, nh, nw, label_of(h, w, nh, nw)) for h, w, nh, nw in pairs() if nh <= 250 and nw <= 250]


def seventy():
    """70 images for a 130 x 200 target: small ones of changing size, and around the 64-descriptor boundary a large LDS image (63), a
    direct one (64) and a single pixel (65)."""
    sizes = [(9 + i % 13, 7 + i % 11, 11 + (5 * i) % 23, 13 + (7 * i) % 29) for i in range(70)]
    sizes[63], sizes[64], sizes[65] = (260, 398, 130, 199), (675, 900, 96, 128), (1, 1, 1, 1)
    return sizes


# ------------------------------------------------------------------------------------------------------------------- mask shrink
# (stride, (h, w), kind): N planes are seeds 0 .. N-1 of the kind
MASK_CASES = [
    (4, (130, 134), 'grey'),       # exact halves: 32.5 -> 32, 33.5 -> 34
    (4, (130, 134), 'binary'),
    (4, (37, 53), 'near'),
    (4, (4, 4), 'grey'),           # a mask as small as the stride: 1 x 1
    (4, (6, 3), 'grey'),           # 1.5 -> 2, 0.75 -> 1
    (1, (19, 23), 'near'),
    (2, (33, 47), 'grey'),         # 16.5 -> 16, 23.5 -> 24
    (2, (2, 2), 'binary'),
    (8, (100, 61), 'grey'),        # 12.5 -> 12, 7.625 -> 8
    (8, (8, 8), 'near'),
    (16, (40, 72), 'binary'),      # 2.5 -> 2, 4.5 -> 4
    (16, (200, 137), 'grey'),
    (16, (16, 16), 'grey'),
    (4, (40, 52), 'const178'),
    (4, (41, 50), 'const179'),
    (4, (42, 51), 'const180'),
    (1, (5, 5), 'const179'),
]


def mask(kind, n, h, w):
    """(n, h, w) uint8 planes, each different: uniform grey; grey within 150 .. 210 (around the 179 threshold); 0 / 255; a constant."""
    rng = np.random.default_rng([7, n, h, w])
    if kind == 'grey':
        return rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    if kind == 'near':
        return rng.integers(150, 211, (n, h, w), dtype=np.uint8)
    if kind == 'binary':
        return (rng.random((n, h, w)) > 0.3).astype(np.uint8) * 255
    return np.full((n, h, w), int(kind[5:]), np.uint8)
