"""Numpy restatement of the photometric augmentation's specification (csrc/photometric.h, csrc/jpeg_sim.hip, the jitter of
csrc/augment.hip), written from the specification text: integer operations in np.int64 with the int32 bounds asserted, the jitter in
fp32 one operation at a time.  Shared by tests/test_photometric_cpu.py and tests/test_gpu_photometric.py."""
import os

import numpy as np

import augment_common as ac

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'augment_photometric.npz')
MODE_TINT, MODE_GRAY = 1, 2
TINT_BOUND = 6          # csrc/photometric.h: |tint(0, 0, 0)(rgb) - rgb| per channel

# ---- tint: RGB -> HSV (H in [0, 180)), add, clamp, HSV -> RGB ----
_I = np.arange(1, 256, dtype=np.int64)
SDIV = np.concatenate([[0], (2 * (255 << 12) + _I) // (2 * _I)])          # rint((255 << 12) / i): no ties for i < 2^13
HDIV = np.concatenate([[0], (2 * (180 << 12) + 6 * _I) // (12 * _I)])     # rint((180 << 12) / (6 i)): no ties for i < 2^14


def rgb_to_hsv(rgb):
    r, g, b = (rgb[..., c].astype(np.int64) for c in range(3))
    v = np.maximum(np.maximum(r, g), b)
    diff = v - np.minimum(np.minimum(r, g), b)
    s = (diff * SDIV[v] + (1 << 11)) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * HDIV[diff] + (1 << 11)) >> 12
    h = h + np.where(h < 0, 180, 0)
    return h, s, v


def hsv_to_rgb(h, s, v):
    sector, f = h // 30, h % 30
    p = (v * (255 - s) + 127) // 255
    q = (v * (7650 - s * f) + 3825) // 7650
    t = (v * (7650 - s * (30 - f)) + 3825) // 7650
    assert (v * 7650 + 3825).max() < 2 ** 31
    table = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    out = np.zeros(h.shape + (3,), np.int64)
    for k, chans in enumerate(table):
        for c in range(3):
            out[..., c] = np.where(sector == k, chans[c], out[..., c])
    return out


def tint(rgb, dh, ds, dv):
    h, s, v = rgb_to_hsv(rgb)
    h = np.clip(h + dh, 0, 179)
    s = np.clip(s + ds, 0, 255)
    v = np.clip(v + dv, 0, 255)
    out = hsv_to_rgb(h, s, v)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def gray(rgb):
    r, g, b = (rgb[..., c].astype(np.int64) for c in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16
    return np.stack([y, y, y], axis=-1).astype(np.uint8)


def epilogue(rgb, desc):
    """desc = (mode bits, dh, ds, dv): tint, then gray."""
    mode, dh, ds, dv = (int(x) for x in desc)
    if mode & MODE_TINT:
        rgb = tint(rgb, dh, ds, dv)
    if mode & MODE_GRAY:
        rgb = gray(rgb)
    return rgb


# ---- JPEG round trip ----
DCT = np.array([[2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896],
                [4017, 3406, 2276, 799, -799, -2276, -3406, -4017],
                [3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784],
                [3406, -799, -4017, -2276, 2276, 4017, 799, -3406],
                [2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896],
                [2276, -4017, 799, 3406, -3406, -799, 4017, -2276],
                [1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567],
                [799, -2276, 3406, -4017, 4017, -3406, 2276, -799]], np.int64)
QUANT_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                       14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                       49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
QUANT_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                         47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)


def quant_tables(quality):
    """(luma, chroma), each (64,) int64 in row-major order, scaled the libjpeg way."""
    assert 1 <= quality <= 100
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * scale + 50) // 100, 1, 255) for base in (QUANT_LUMA, QUANT_CHROMA))


def _blocks(plane):
    """(H, W) with H, W multiples of 8 -> (H/8, W/8, 8, 8)."""
    H, W = plane.shape
    return plane.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)


def _unblocks(b):
    nby, nbx = b.shape[:2]
    return b.transpose(0, 2, 1, 3).reshape(nby * 8, nbx * 8)


def _roundtrip_plane(plane, q):
    """Level shift, forward DCT, quantise, dequantise, inverse DCT, clamp: blocks [y][x] -> [v][u] -> [y][x]."""
    p = _blocks(plane.astype(np.int64)) - 128
    q = q.reshape(8, 8)
    t = (np.einsum('ux,...yx->...yu', DCT, p) + (1 << 9)) >> 10
    assert np.abs(t).max() <= 2896
    F = (np.einsum('vy,...yu->...vu', DCT, t) + (1 << 15)) >> 16
    assert np.abs(F).max() <= 1024
    k = np.sign(F) * ((np.abs(F) + (q >> 1)) // q)
    F = k * q
    assert np.abs(F).max() <= 1151
    t = (np.einsum('vy,...vu->...yu', DCT, F) + (1 << 9)) >> 10
    assert np.abs(t).max() * 23168 + (1 << 15) < 2 ** 31
    p = (np.einsum('ux,...yu->...yx', DCT, t) + (1 << 15)) >> 16
    return _unblocks(np.clip(p + 128, 0, 255))


def jpeg_roundtrip(rgb, quality):
    """(S, S, 3) uint8 -> (S, S, 3) uint8."""
    S = rgb.shape[0]
    P = (S + 15) // 16 * 16
    idx = np.minimum(np.arange(P), S - 1)
    r, g, b = (rgb[idx][:, idx][..., c].astype(np.int64) for c in range(3))       # the last row and column replicated
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    sub = lambda c: (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2  # noqa: E731
    ql, qc = quant_tables(quality)
    y = _roundtrip_plane(y, ql)
    cb, cr = (np.repeat(np.repeat(_roundtrip_plane(sub(c), qc), 2, axis=0), 2, axis=1) - 128 for c in (cb, cr))
    out = np.stack([y + ((91881 * cr + 32768) >> 16),
                    y + ((-22554 * cb - 46802 * cr + 32768) >> 16),
                    y + ((116130 * cb + 32768) >> 16)], axis=-1)
    return np.clip(out, 0, 255).astype(np.uint8)[:S, :S]


# ---- keypoint jitter ----
def jitter_joints(out, n_persons, noise, eps, shift):
    """The jitter step of og_affine_joints_jitter_f32 on one gated image: out (P, K, 4) the plain transform's result, noise (P, K, 2)."""
    f = np.float32
    out = np.asarray(out, f).copy()
    u = np.asarray(noise, f)[:n_persons]
    t = u - f(0.5)
    t = t + f(shift)
    t = t * f(2)
    t = f(eps) * t
    out[:n_persons, :, :2] = out[:n_persons, :, :2] + t
    return out


# ---- cases ----
PHOTO_MIX = ((0, 0, 0, 0), (MODE_TINT, 10, -40, 30), (MODE_GRAY, 0, 0, 0))     # per image of the GPU batch: none / tint(+jpeg) / gray
TINT_CORNERS = [(dh, ds, dv) for dh in (-10, 10) for ds in (-40, 40) for dv in (-30, 30)] + [(0, 0, 0)]


def lattice():
    """17^3 colours (steps of 16, 255 at the end) plus the 256 greys -> (n, 3) uint8."""
    a = np.minimum(np.arange(17) * 16, 255)
    cube = np.stack(np.meshgrid(a, a, a, indexing='ij'), axis=-1).reshape(-1, 3)
    greys = np.repeat(np.arange(256)[:, None], 3, axis=1)
    return np.concatenate([cube, greys]).astype(np.uint8)


def structured_images():
    """Two 64 x 64 images: a two-way gradient, flat shapes and mild noise (not white noise)."""
    rs = np.random.RandomState(3)
    yy, xx = np.mgrid[0:64, 0:64]
    a = np.stack([xx * 3 + 20, yy * 3 + 30, (xx + yy) * 1.5 + 10], axis=-1).astype(np.float64)
    a[10:30, 12:40] = (200, 60, 40)
    a[36:56, 30:60] = (30, 140, 210)
    b = np.stack([128 + 90 * np.sin(xx / 9.0), 128 + 90 * np.cos(yy / 7.0), 128 + 60 * np.sin((xx + yy) / 11.0)], axis=-1)
    b[(xx - 40) ** 2 + (yy - 24) ** 2 < 150] = (240, 230, 60)
    b[44:60, 6:26] = (20, 30, 40)
    return [np.clip(im + rs.normal(0, 3, im.shape), 0, 255).astype(np.uint8) for im in (a, b)]


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float('inf') if mse == 0 else float(10 * np.log10(255.0 ** 2 / mse))


normalize = ac.normalize
