"""Detected poses and the model-inspection views painted over the images on the device (reference package `visualization/`: what
evaluate.py:267-284 shows through show.py:KeypointPainter.keypoints -- one colour per person, skeleton lines with round caps, a marker
per visible keypoint, no box -- and the heat-map, candidate-limb and offset-arrow figures of demo_batch.py:215-317).

`draw_poses` is one launch of og_draw_poses_u8 (csrc/draw.hip; the semantics are spelled out in include/og_decoder.h): a capsule / disc
rasteriser of this package's own with the painter's defaults, not matplotlib's renderer.  The batch stays on the device; `save_ppm` is the
host copy, taken only when somebody asks for a file.  `draw_heatmap`, `draw_segments`, `draw_limbs` and `draw_offsets` are the other
three views of demo_batch.py (csrc/views.hip: og_draw_heatmap_u8, og_draw_segments_u8 fed by og_limbs_to_segments_f32 /
og_offsets_to_segments_f32), specified the same way.  Neither matplotlib nor cv2 is used."""
import numpy as np
import torch

from .. import _lib
from ..config import data_mean, data_std

# matplotlib's "tab20" colours as 8-bit RGB (plain colour data): person p is painted in TAB20[p % 20] (show.py:244-245)
TAB20 = np.array([
    [31, 119, 180], [174, 199, 232], [255, 127, 14], [255, 187, 120], [44, 160, 44], [152, 223, 138], [214, 39, 40], [255, 152, 150],
    [148, 103, 189], [197, 176, 213], [140, 86, 75], [196, 156, 148], [227, 119, 194], [247, 182, 210], [127, 127, 127],
    [199, 199, 199], [188, 189, 34], [219, 219, 141], [23, 190, 207], [158, 218, 229]], dtype=np.uint8)

# matplotlib's "viridis" at nine evenly spaced positions (the published 9-colour viridis palette; plain colour data) and the 256-entry
# table interpolated linearly between them: the default colour map of draw_heatmap, as imshow's is
VIRIDIS_ANCHORS = np.array([[68, 1, 84], [71, 45, 123], [59, 82, 139], [44, 114, 142], [33, 144, 140], [39, 173, 129], [93, 200, 99],
                            [170, 220, 50], [253, 231, 37]], dtype=np.uint8)
VIRIDIS_ANCHOR_POSITIONS = np.array([0, 32, 64, 96, 128, 159, 191, 223, 255])       # round(255 i / 8)
VIRIDIS = np.stack([np.interp(np.arange(256), VIRIDIS_ANCHOR_POSITIONS, VIRIDIS_ANCHORS[:, ch].astype(np.float64))
                    for ch in range(3)], axis=1).round().astype(np.uint8)

_palettes = {}


def _palette_table(palette, device, default=TAB20, what='palette'):
    """(n_colors, 3) uint8 device table, cached per (colours, device)."""
    pal = np.ascontiguousarray(default if palette is None else palette)
    if pal.dtype != np.uint8 or pal.ndim != 2 or pal.shape[1] != 3 or pal.shape[0] == 0:
        raise ValueError(f'{what}: expected (n_colors, 3) uint8, got {pal.dtype} {pal.shape}')
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


def _canvas(images, who):
    """The checks every painter makes on its canvas -> (N, H, W)."""
    if not isinstance(images, torch.Tensor):
        raise TypeError(f'images: expected a torch.Tensor, got {type(images).__name__}')
    if not images.is_cuda:
        raise _lib.OgError(f'images: tensor is on {images.device}; {who} paints on the GPU (offsetguided_amd has no CPU path)')
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3 or not images.is_contiguous():
        raise ValueError(f'images: expected a contiguous (N, H, W, 3) uint8 tensor, got {images.dtype} {tuple(images.shape)}')
    return tuple(int(v) for v in images.shape[:3])


def _maps(t, name, images, channels=None):
    """A stride-4 fp32 map batch (N, C, H / 4, W / 4) on the canvas's device (no conversion: a wrong dtype is the caller's mistake)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'{name}: expected a torch.Tensor, got {type(t).__name__}')
    if not t.is_cuda:
        raise _lib.OgError(f'{name}: tensor is on {t.device}; the views paint on the GPU (offsetguided_amd has no CPU path)')
    N, H, W = (int(v) for v in images.shape[:3])
    if (t.dtype != torch.float32 or t.dim() != 4 or t.device != images.device or t.shape[0] != N or 4 * t.shape[2] != H
            or 4 * t.shape[3] != W or (channels is not None and t.shape[1] != channels)):
        raise ValueError(f'{name}: expected a float32 (N = {N}, {"C" if channels is None else channels}, {H} / 4, {W} / 4) tensor on '
                         f'{images.device}, got {t.dtype} {tuple(t.shape)} on {t.device}')
    return t.contiguous()


def _rgb(colour, name):
    c = np.asarray(colour)
    if c.shape != (3,) or not np.issubdtype(c.dtype, np.integer) or (c < 0).any() or (c > 255).any():
        raise ValueError(f'{name}: expected three integers in [0, 255], got {colour!r}')
    return int(c[0]) | int(c[1]) << 8 | int(c[2]) << 16


def draw_heatmap(images, hmps, channel, *, nms=False, vmin=0.0, vmax=1.0, alpha=0.8, colormap=None):
    """Paint channel `channel` of the stride-4 heat maps hmps (N, C, H / 4, W / 4) float32 over `images`, a contiguous (N, H, W, 3)
    uint8 RGB device tensor, IN PLACE; returns `images`.  The x4 bicubic value of every pixel -- with nms=True what hmp_NMS leaves of
    it (the 3 x 3 peaks, zero elsewhere) -- goes through the colour table: [vmin, vmax] is spread over `colormap`, (n, 3) uint8
    (default VIRIDIS), values outside clamp, a NaN leaves its pixel alone, and the colour is blended over the pixel with `alpha`
    (default: the reference's imshow(alpha=0.8)).  One launch of og_draw_heatmap_u8 on the current stream; no synchronisation."""
    N, H, W = _canvas(images, 'draw_heatmap')
    hm = _maps(hmps, 'hmps', images)
    if not 0 <= int(channel) < hm.shape[1]:
        raise ValueError(f'channel: {channel} outside [0, {hm.shape[1]})')
    if not (np.isfinite(vmin) and np.isfinite(vmax) and np.float32(vmax) > np.float32(vmin)):
        raise ValueError(f'vmin / vmax: expected finite vmin < vmax, got {vmin} / {vmax}')
    dev = images.device
    lut = _palette_table(colormap, dev, VIRIDIS, 'colormap')
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.og_draw_heatmap_u8(_lib.ptr(images), _lib.ptr(hm), _lib.ptr(lut), int(lut.shape[0]), N, int(hm.shape[1]), H // 4,
                                          W // 4, int(channel), float(vmin), float(vmax), float(alpha), int(bool(nms)),
                                          _lib.stream_ptr(dev)), lib)
    return images


def draw_segments(images, segs, n_segs=None, *, line_color=(255, 0, 0), marker_color=(0, 128, 0), line_width=2.0, start_radius=3.0,
                  end_radius=3.0, alpha=1.0):
    """Paint line segments with end markers over `images`, a contiguous (N, H, W, 3) uint8 RGB device tensor, IN PLACE; returns
    `images`.  segs: (N, S, 4) float32 device tensor, rows x1, y1, x2, y2 in pixel coordinates of `images`; n_segs: (N) int32 device
    tensor, rows in use per image (None: all S; the kernel clamps a count to [0, S]).  Per segment, in row order: the line (a capsule
    `line_width` wide in line_color), a disc of start_radius at (x1, y1) and one of end_radius at (x2, y2) in marker_color (radius 0:
    none) -- default colours matplotlib's 'r' and 'g', as the reference plots its limbs.  One launch of og_draw_segments_u8 on the
    current stream; no synchronisation."""
    N, H, W = _canvas(images, 'draw_segments')
    dev = images.device
    if not isinstance(segs, torch.Tensor):
        raise TypeError(f'segs: expected a torch.Tensor, got {type(segs).__name__}')
    if not segs.is_cuda:
        raise _lib.OgError(f'segs: tensor is on {segs.device}; draw_segments paints on the GPU (offsetguided_amd has no CPU path)')
    if segs.dtype != torch.float32 or segs.dim() != 3 or segs.shape[0] != N or segs.shape[2] != 4 or segs.device != dev:
        raise ValueError(f'segs: expected a float32 (N = {N}, S, 4) tensor on {dev}, got {segs.dtype} {tuple(segs.shape)} on {segs.device}')
    S = int(segs.shape[1])
    if n_segs is None:
        n_segs = _full_counts(N, S, dev)
    elif not isinstance(n_segs, torch.Tensor):
        raise TypeError(f'n_segs: expected a torch.Tensor (the counts stay on the device), got {type(n_segs).__name__}')
    elif not n_segs.is_cuda:
        raise _lib.OgError(f'n_segs: tensor is on {n_segs.device}; the counts stay on the GPU')
    elif n_segs.dtype != torch.int32 or n_segs.numel() != N or n_segs.device != dev:
        raise ValueError(f'n_segs: expected {N} int32 entries on {dev}, got {n_segs.dtype} {tuple(n_segs.shape)} on {n_segs.device}')
    line, marker = _rgb(line_color, 'line_color'), _rgb(marker_color, 'marker_color')
    if S == 0:
        return images
    segs, n_segs = segs.contiguous(), n_segs.contiguous()
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.og_draw_segments_u8(_lib.ptr(images), _lib.ptr(segs), _lib.ptr(n_segs), N, H, W, S, line, marker, float(line_width),
                                           float(start_radius), float(end_radius), float(alpha), _lib.stream_ptr(dev)), lib)
    return images


_counts = {}


def _full_counts(N, S, device):
    key = (N, S, device.index)
    t = _counts.get(key)
    if t is None:
        t = _counts[key] = torch.full((N,), S, dtype=torch.int32, device=device)
    return t


def limbs_to_segments(limbs, *, limb=None, dist_max=20.0):
    """The candidate limbs (N, L, K, 13) float32 of PostProcess.generate_limbs as segments: rows of limb type `limb` (None: all) with
    both ends found (x1 > 0, x2 > 0) whose guided end misses its keypoint by at most dist_max (demo_batch.py:272), in (l, i) order ->
    (segs (N, L * K, 4), n_segs (N) int32), both on the device (rows past a count are uninitialised).  og_limbs_to_segments_f32."""
    if not isinstance(limbs, torch.Tensor):
        raise TypeError(f'limbs: expected a torch.Tensor, got {type(limbs).__name__}')
    if not limbs.is_cuda:
        raise _lib.OgError(f'limbs: tensor is on {limbs.device}; the views run on the GPU (offsetguided_amd has no CPU path)')
    if limbs.dtype != torch.float32 or limbs.dim() != 4 or limbs.shape[3] != 13 or 0 in limbs.shape:
        raise ValueError(f'limbs: expected a float32 (N, L, K, 13) tensor, got {limbs.dtype} {tuple(limbs.shape)}')
    N, L, K = (int(v) for v in limbs.shape[:3])
    if limb is not None and not 0 <= int(limb) < L:
        raise ValueError(f'limb: {limb} outside [0, {L})')
    dev = limbs.device
    limbs = limbs.contiguous()
    segs = torch.empty((N, L * K, 4), dtype=torch.float32, device=dev)
    n_segs = torch.empty((N,), dtype=torch.int32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.og_limbs_to_segments_f32(_lib.ptr(limbs), N, L, K, -1 if limb is None else int(limb), float(dist_max),
                                                _lib.ptr(segs), _lib.ptr(n_segs), _lib.stream_ptr(dev)), lib)
    return segs, n_segs


def draw_limbs(images, limbs, *, limb=None, dist_max=20.0, **painter_kwargs):
    """Every candidate limb the pairing stage produced, painted over `images` IN PLACE (demo_batch.py --show-all-limbs): limbs_to_segments
    and then draw_segments with `painter_kwargs`; the counts stay on the device.  Returns `images`."""
    N, _, _ = _canvas(images, 'draw_limbs')
    if isinstance(limbs, torch.Tensor) and limbs.dim() == 4 and limbs.shape[0] != N:
        raise ValueError(f'limbs: {limbs.shape[0]} images of limbs for {N} images')
    segs, n_segs = limbs_to_segments(limbs, limb=limb, dist_max=dist_max)
    return draw_segments(images, segs, n_segs, **painter_kwargs)


def offsets_to_segments(hmps, offs, limb, skeleton, *, step=7, thre=0.2):
    """The guiding offsets of limb type `limb` as arrows: at every `step`-th pixel of the x4 grid where the heat map of the limb's first
    keypoint (skeleton[limb][0], an index from 0) reaches `thre`, the segment from the pixel to pixel + offset (show.py:52-64) ->
    (segs (N, S, 4), n_segs (N) int32) on the device.  og_offsets_to_segments_f32."""
    for t, name in ((hmps, 'hmps'), (offs, 'offs')):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f'{name}: expected a torch.Tensor, got {type(t).__name__}')
        if not t.is_cuda:
            raise _lib.OgError(f'{name}: tensor is on {t.device}; the views run on the GPU (offsetguided_amd has no CPU path)')
        if t.dtype != torch.float32 or t.dim() != 4 or 0 in t.shape:
            raise ValueError(f'{name}: expected a float32 (N, C, h, w) tensor, got {t.dtype} {tuple(t.shape)}')
    pairs = np.asarray(skeleton, dtype=np.int64).reshape(-1, 2)
    N, C, h, w = (int(v) for v in hmps.shape)
    L = int(pairs.shape[0])
    if tuple(offs.shape) != (N, 2 * L, h, w) or offs.device != hmps.device:
        raise ValueError(f'offs: expected {(N, 2 * L, h, w)} (two channels per limb of the skeleton) on {hmps.device}, got '
                         f'{tuple(offs.shape)} on {offs.device}')
    if not 0 <= int(limb) < L:
        raise ValueError(f'limb: {limb} outside [0, {L})')
    joint_from = int(pairs[int(limb), 0])
    if not 0 <= joint_from < C:
        raise ValueError(f'skeleton: keypoint index {joint_from} outside [0, {C})')
    if int(step) != step or int(step) <= 0:
        raise ValueError(f'step: expected a positive integer, got {step!r}')
    dev = hmps.device
    lib = _lib.load()
    S = int(lib.og_offsets_segments_capacity(h, w, int(step)))
    hmps, offs = hmps.contiguous(), offs.contiguous()
    segs = torch.empty((N, S, 4), dtype=torch.float32, device=dev)
    n_segs = torch.empty((N,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.og_offsets_to_segments_f32(_lib.ptr(hmps), _lib.ptr(offs), N, C, L, h, w, joint_from, int(limb), int(step),
                                                  float(thre), _lib.ptr(segs), _lib.ptr(n_segs), _lib.stream_ptr(dev)), lib)
    return segs, n_segs


def draw_offsets(images, hmps, offs, limb, skeleton, *, step=7, thre=0.2, start_radius=0.0, end_radius=1.5, **painter_kwargs):
    """The offset field of limb type `limb` as arrows over `images` IN PLACE (demo_batch.py --show-limb-idx, show.py:draw_limb_offset
    with its s=7, thre=0.2): offsets_to_segments and then draw_segments; the end disc marks the arrow head.  hmps (N, C, H / 4, W / 4)
    and offs (N, 2 L, H / 4, W / 4) are the stride-4 maps; `skeleton` as draw_poses takes it.  Returns `images`."""
    _canvas(images, 'draw_offsets')
    hmps = _maps(hmps, 'hmps', images)
    offs = _maps(offs, 'offs', images)
    segs, n_segs = offsets_to_segments(hmps, offs, limb, skeleton, step=step, thre=thre)
    return draw_segments(images, segs, n_segs, start_radius=start_radius, end_radius=end_radius, **painter_kwargs)


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
