"""Detected poses painted over the images on the device (reference package `visualization/`: what evaluate.py:267-284 shows through
show.py:KeypointPainter.keypoints -- one colour per person, skeleton lines with round caps, a marker per visible keypoint, no box).

`draw_poses` is one launch of og_draw_poses_u8 (csrc/draw.hip; the semantics are spelled out in include/og_decoder.h): a capsule / disc
rasteriser of this package's own with the painter's defaults, not matplotlib's renderer.  The batch stays on the device; `save_ppm` is the
host copy, taken only when somebody asks for a file.  Neither matplotlib nor cv2 is used."""
import numpy as np
import torch

from .. import _lib
from ..config import data_mean, data_std

# matplotlib's "tab20" colours as 8-bit RGB (plain colour data): person p is painted in TAB20[p % 20] (show.py:244-245)
TAB20 = np.array([
    [31, 119, 180], [174, 199, 232], [255, 127, 14], [255, 187, 120], [44, 160, 44], [152, 223, 138], [214, 39, 40], [255, 152, 150],
    [148, 103, 189], [197, 176, 213], [140, 86, 75], [196, 156, 148], [227, 119, 194], [247, 182, 210], [127, 127, 127],
    [199, 199, 199], [188, 189, 34], [219, 219, 141], [23, 190, 207], [158, 218, 229]], dtype=np.uint8)

_palettes = {}


def _palette_table(palette, device):
    """(n_colors, 3) uint8 device table, cached per (colours, device)."""
    pal = np.ascontiguousarray(TAB20 if palette is None else palette)
    if pal.dtype != np.uint8 or pal.ndim != 2 or pal.shape[1] != 3:
        raise ValueError(f'palette: expected (n_colors, 3) uint8, got {pal.dtype} {pal.shape}')
    key = (pal.tobytes(), device.index)
    t = _palettes.get(key)
    if t is None:
        t = _palettes[key] = torch.from_numpy(pal.copy()).to(device)
    return t


def draw_poses(images, poses, skeleton, *, n_persons=None, line_width=2.0, marker_radius=3.0, alpha=1.0, palette=None):
    """Paint poses over `images`, a contiguous (N, H, W, 3) uint8 RGB device tensor, IN PLACE; returns `images`.
    poses: a list of N arrays (P_n, K, >= 3) with rows x, y, v in pixel coordinates of `images` (what PostProcess.generate_poses /
    PendingPoses.result() hand out; columns beyond the third are ignored), or a padded (N, P, K, >= 3) array / tensor with `n_persons`
    (N) persons in use per image (None: all P).  skeleton: (L, 2) keypoint index pairs as `processor.skeleton` and the reference's
    painter take them (config.COCO_PERSON_SKELETON: indices into the K keypoints, from 0).  line_width / marker_radius default to KeypointPainter's linewidth=2 / markersize=3 (a marker is a disc of that radius in
    pixels); palette: (n_colors, 3) uint8, person p gets colour p % n_colors (default TAB20).  Stream-ordered on the current stream."""
    if not isinstance(images, torch.Tensor):
        raise TypeError(f'images: expected a torch.Tensor, got {type(images).__name__}')
    if not images.is_cuda:
        raise _lib.OgError(f'images: tensor is on {images.device}; draw_poses paints on the GPU (offsetguided_amd has no CPU path)')
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3 or not images.is_contiguous():
        raise ValueError(f'images: expected a contiguous (N, H, W, 3) uint8 tensor, got {images.dtype} {tuple(images.shape)}')
    dev = images.device
    N, H, W = (int(v) for v in images.shape[:3])
    if isinstance(poses, (list, tuple)):
        if n_persons is not None:
            raise ValueError('n_persons goes with a padded (N, P, K, 3) table, not with a list of per-image arrays')
        per_image = [np.asarray(p, dtype=np.float32) for p in poses]
        if len(per_image) != N:
            raise ValueError(f'poses: {len(per_image)} arrays for {N} images')
        shaped = [p for p in per_image if p.size]          # (an image without detections may come as any empty array)
        if not shaped:                                     # nobody detected anywhere: nothing to paint
            return images
        K = int(shaped[0].shape[1]) if shaped[0].ndim == 3 else 0
        if any(p.ndim != 3 or p.shape[1] != K or p.shape[2] < 3 for p in shaped):
            raise ValueError(f'poses: expected arrays (P_n, K, >= 3) with one K, got {[p.shape for p in per_image]}')
        counts = np.array([p.shape[0] if p.size else 0 for p in per_image], dtype=np.int32)
        table = np.zeros((N, int(counts.max()), K, 3), dtype=np.float32)
        for i, p in enumerate(per_image):
            if counts[i]:
                table[i, :counts[i]] = p[:, :, :3]
        table = torch.from_numpy(table).to(dev)
    else:
        table = poses.to(dev) if isinstance(poses, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float32)).to(dev)
        if table.dim() != 4 or table.shape[0] != N or table.shape[3] < 3:
            raise ValueError(f'poses: expected (N, P, K, >= 3) with N = {N}, got {tuple(table.shape)}')
        table = _lib.require_device(table[..., :3], 'poses')
        if table.shape[1] == 0:
            return images
        K = int(table.shape[2])
        counts = np.full(N, table.shape[1], dtype=np.int32) if n_persons is None else n_persons
    P = int(table.shape[1])
    if isinstance(counts, torch.Tensor):      # a device table is taken as it is: the kernel clamps every count to [0, P]
        if counts.numel() != N:
            raise ValueError(f'n_persons: expected {N} entries, got {counts.numel()}')
        counts = _lib.require_device(counts, 'n_persons', torch.int32)
    else:
        counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
        if counts.shape[0] != N or (counts < 0).any() or (counts > P).any():
            raise ValueError(f'n_persons: expected {N} entries in [0, {P}], got {counts.tolist()}')
        counts = torch.from_numpy(counts).to(dev)
    limbs = np.asarray(skeleton, dtype=np.int64).reshape(-1, 2)
    if limbs.shape[0] == 0 or (limbs < 0).any() or (limbs >= K).any():     # on the host, before the copy: nothing launches
        raise ValueError(f'skeleton: keypoint indices must lie in [0, {K}) (and at least one limb), got {limbs.tolist()}')
    lib = _lib.load()
    pal = _palette_table(palette, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.og_draw_poses_u8(_lib.ptr(images), _lib.ptr(table), _lib.ptr(counts), _lib.ptr(_lib.int_table(limbs.reshape(-1), dev)),
                                        _lib.ptr(pal), int(pal.shape[0]), N, H, W, P, K, int(limbs.shape[0]), float(line_width),
                                        float(marker_radius), float(alpha), _lib.stream_ptr(dev)), lib)
    return images


def denormalise_u8(images, mean=data_mean, std=data_std):
    """(N, 3, H, W) fp32 device batch as the input chain wrote it, (v / 255 - mean) / std, back to the (N, H, W, 3) uint8 pixels v it
    normalised (the chain rescales, pads and normalises in one launch and keeps no uint8 batch).  Exact: the round trip is off by
    ~1e-5 of a level before the rounding."""
    x = _lib.require_device(images, 'images')
    m = torch.tensor(mean, dtype=torch.float32, device=x.device).view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32, device=x.device).view(1, 3, 1, 1)
    v = ((x * s + m) * 255.0 + 0.5).floor_().clamp_(0, 255)
    return v.to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def save_ppm(path, image):
    """One (H, W, 3) uint8 RGB image (device or host tensor, or array) as a binary PPM (P6, maxval 255)."""
    if isinstance(image, torch.Tensor):
        image = image.detach().cpu().numpy()
    image = np.ascontiguousarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError(f'save_ppm: expected (H, W, 3) uint8, got {image.dtype} {image.shape}')
    with open(path, 'wb') as f:
        f.write(b'P6\n%d %d\n255\n' % (image.shape[1], image.shape[0]))
        f.write(image.tobytes())
    return path
