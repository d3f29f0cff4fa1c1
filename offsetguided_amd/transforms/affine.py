"""WarpAffineTransforms (transforms/affine.py:71-278) with the image work on the device.

Host side, restated from the reference: the seven random parameters in its draw order (`WarpAffineTransforms.draw`, :114-126), the
centre of the annotated area (`roi_center`, :14-25) and the one 3x3 matrix that flips, rotates, scales, stretches and translates
(`affine_matrix`, :229-278), all in float64.  Device side (`DeviceAugment`, csrc/augment.hip): ONE launch warps a batch of raw uint8
images of any sizes into the normalised fp32 NCHW crop (og_warp_affine_batch_u8), one warps `mask_miss` (og_warp_affine_mask_u8), one
transforms the keypoints with the same matrices (og_affine_joints_f32).  The warp is an integer specification of this package's own
(32 sub-pixel phases, 4-tap cubic, 2^11 fixed-point taps), held bit for bit to a numpy restatement; like the evaluation chain's resize
it does NOT claim bit parity with cv2.warpAffine(INTER_CUBIC): cv2 is not available offline."""
import ctypes as C
import math
import random

import numpy as np
import torch

from .. import _lib
from ..config import data_mean, data_std
from ..config.coco_data import LEFT_INDEX, RIGHT_INDEX
from .pad import FILL
from .photometric import draw_photo, photo_table

COORD_LIMIT = float(1 << 20)   # the device kernel computes source coordinates in int32 with 10 + 5 fractional bits


class AugParams:
    """Augmentation parameters with the training defaults of the reference's command line (data/factory.py:84-104)."""

    def __init__(self, flip_prob=0.5, max_rotate=45, min_scale=0.5, max_scale=2.0, min_stretch=0.95, max_stretch=1.05,
                 max_translate=150):
        self.flip_prob, self.max_rotate = flip_prob, max_rotate
        self.min_scale, self.max_scale = min_scale, max_scale
        self.min_stretch, self.max_stretch = min_stretch, max_stretch
        self.max_translate = max_translate


class FixedAugParams(AugParams):
    """No randomness: the transform only crops round the annotated area (transforms/affine.py:28-68)."""

    def __init__(self):
        super().__init__(flip_prob=0, max_rotate=0, min_scale=1., max_scale=1., min_stretch=1., max_stretch=1., max_translate=0.)


def roi_center(joints, n_persons, width_height):
    """Centre (x, y) of the area filled with visible keypoints, fp32, floor-divided as the reference does (_roi_center); the image
    centre when there is no person -- or, where the reference would fail on an empty minimum, no visible keypoint."""
    joints = np.asarray(joints, np.float32)[:int(n_persons)]
    vis = joints[:, :, 2] > 0 if len(joints) else np.zeros((0, 0), bool)
    if not vis.any():
        return np.asarray(width_height).astype(np.float32) // 2
    xs, ys = joints[vis, 0], joints[vis, 1]
    return np.array([(xs.min() + xs.max()) // 2, (ys.min() + ys.max()) // 2]).astype(np.float32)


def affine_matrix(params, roi_center, width_height, dst_size, crop_roi=True):
    """The 3x3 float64 matrix of _get_affine_mat for drawn `params` = (flip, rotate, scale, x_stretch, y_stretch, x_offset, y_offset):
    translate . to-crop-centre . flip . scale . rotate . image-centre-to-origin, composed in that order.  The image centre and the
    move to the ROI are fp32 values, and the product move * scale is rounded to fp32, as NumPy >= 2 evaluates the reference's
    expression (fp32 scalar times Python float)."""
    flip, rotate, scale, x_stretch, y_stretch, x_offset, y_offset = params
    in_size = dst_size if isinstance(dst_size, (list, tuple)) else [dst_size] * 2
    cangle, sangle = math.cos(rotate / 180. * math.pi), math.sin(rotate / 180. * math.pi)
    scale_x, scale_y = x_stretch * scale, y_stretch * scale
    center = (np.asarray(width_height) - 1).astype(np.float32) / 2
    move = center - np.asarray(roi_center, np.float32)
    translate_x = x_offset + (move[0] * np.float32(scale_x) if crop_roi else 0)
    translate_y = y_offset + (move[1] * np.float32(scale_y) if crop_roi else 0)
    center2zero = np.array([[1., 0., -center[0]], [0., 1., -center[1]], [0., 0., 1.]])
    rot = np.array([[cangle, sangle, 0.], [-sangle, cangle, 0.], [0., 0., 1.]])
    scl = np.array([[scale_x, 0., 0.], [0., scale_y, 0.], [0., 0., 1.]])
    flp = np.array([[-1. if flip else 1., 0., 0.], [0., 1., 0.], [0., 0., 1.]])
    zero2center = np.array([[1., 0., (in_size[0] - 1) / 2], [0., 1., (in_size[1] - 1) / 2], [0., 0., 1.]])
    center2center = np.array([[1., 0., translate_x], [0., 1., translate_y], [0., 0., 1.]])
    return center2center.dot(zero2center).dot(flp).dot(scl).dot(rot).dot(center2zero)


def inverse_rows(mat, dst_size):
    """D = inv(M)[0:2] in float64: the destination -> source map the warp kernel walks.  ValueError if M is singular or if a source
    coordinate over the destination square could reach 2^20 in magnitude (|D00| S + |D01| S + |D02| >= 2^20, likewise row 1): the
    kernel may then assume that everything fits int32."""
    mat = np.asarray(mat, np.float64)
    S = max(dst_size) if isinstance(dst_size, (list, tuple)) else dst_size
    det = mat[0, 0] * mat[1, 1] - mat[0, 1] * mat[1, 0]
    if not np.isfinite(mat).all() or det == 0.0 or not np.isfinite(1.0 / det):
        raise ValueError(f'affine matrix is singular or not finite:\n{mat}')
    D = np.linalg.inv(mat)[0:2]
    reach = np.abs(D[:, 0]) * S + np.abs(D[:, 1]) * S + np.abs(D[:, 2])
    if not (reach < COORD_LIMIT).all():
        raise ValueError(f'affine matrix maps the {S} x {S} crop to source coordinates of magnitude {reach.max():.3g} >= 2^20')
    return np.ascontiguousarray(D)


class WarpAffineTransforms:
    """The reference's names, signature and defaults; the parameters are drawn here, the pixels move in DeviceAugment."""

    def __init__(self, dst_size, *, aug_params, crop_roi=True):
        assert isinstance(dst_size, (int, list)), dst_size
        self.in_size = dst_size if isinstance(dst_size, list) else [dst_size] * 2
        self.flip_prob, self.max_rotate = aug_params.flip_prob, aug_params.max_rotate
        self.min_scale, self.max_scale = aug_params.min_scale, aug_params.max_scale
        self.min_stretch, self.max_stretch = aug_params.min_stretch, aug_params.max_stretch
        self.max_translate = aug_params.max_translate
        self.crop_roi = crop_roi

    def draw(self, rng=random):
        """(flip, rotate, scale, x_stretch, y_stretch, x_offset, y_offset): seven rng.uniform calls in the reference's order."""
        flip = rng.uniform(0., 1.) < self.flip_prob
        rotate = rng.uniform(-1., 1.) * self.max_rotate
        scale = (self.max_scale - self.min_scale) * rng.uniform(0., 1.) + self.min_scale
        x_stretch = (self.max_stretch - self.min_stretch) * rng.uniform(0., 1.) + self.min_stretch
        y_stretch = (self.max_stretch - self.min_stretch) * rng.uniform(0., 1.) + self.min_stretch
        x_offset = int(rng.uniform(-1., 1.) * self.max_translate)
        y_offset = int(rng.uniform(-1., 1.) * self.max_translate)
        return flip, rotate, scale, x_stretch, y_stretch, x_offset, y_offset

    def affine_matrix(self, params, roi_center, width_height):
        return affine_matrix(params, roi_center, width_height, self.in_size, self.crop_roi)


def _align16(v):
    return (v + 15) // 16 * 16


class DeviceAugment:
    """Batched WarpAffineTransforms + ToTensor + Normalize.  Called as (raw_images, joints, n_persons, mask_miss=None, rng=random):
    raw_images a list of (h, w, 3) uint8 arrays of any sizes, joints (N,P,17,4) fp32 rows [x, y, v, scale] in source pixels,
    n_persons (N,) int32, mask_miss a list of (h, w) uint8 arrays of the images' sizes, or a data.DeviceMasks (the planes
    og_coco_masks_u8 left in device memory: warped straight from there, nothing of them is staged) -> (images (N,3,S,S) fp32 normalised, joints
    (N,P,17,4), mask (N,S,S) uint8 or None, all on the device; mats (N,3,3) float64 numpy).  Images, masks and annotations are packed
    into one pinned staging buffer and copied once; everything is queued on the current stream and the call never waits for the
    device (a staging buffer whose last copy is still in flight is left alone and a new one is taken).
    photo_params (transforms.PhotoParams): the reference's RandomApply steps behind the warp -- AnnotationJitter, JpegCompression,
    ColorTint, Gray --, drawn per image after the matrices in the order transforms/photometric.py documents (gates from `rng`, the
    tint's deltas from `np_rng`, default numpy.random, the jitter's noise from torch's CPU generator) and kept in `last_photo`.  With
    every probability 0 (the default) nothing is drawn and the launches are the ones above.  Otherwise the image launch is
    og_warp_affine_photo_batch_u8 (tint and gray between the warp and the normalisation, still ONE launch), images with a JPEG
    round trip are redone from the warped bytes by og_jpeg_roundtrip_batch_u8, and the keypoints go through
    og_affine_joints_jitter_f32, the noise riding in the same staging buffer."""

    def __init__(self, dst_size, aug_params, crop_roi=True, device='cuda:0', mean=data_mean, std=data_std, border=FILL, mask_border=255,
                 photo_params=None, np_rng=None):
        assert isinstance(dst_size, int), 'the device warp writes a square crop'
        self.transform = WarpAffineTransforms(dst_size, aug_params=aug_params, crop_roi=crop_roi)
        self.size, self.device = dst_size, torch.device(device)
        f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])  # noqa: E731
        self._mean, self._std = f3(mean), f3(std)
        self._border, self.mask_border = (C.c_ubyte * 3)(*[int(x) for x in border]), int(mask_border)
        n_lr = len(LEFT_INDEX)
        self._left, self._right = (C.c_int * n_lr)(*LEFT_INDEX), (C.c_int * n_lr)(*RIGHT_INDEX)
        self._stage, self._turn = [None, None, None], 0
        self.last_params = None
        self.photo_params, self.np_rng, self.last_photo = photo_params, np_rng, None

    def _staging(self, nbytes):
        buf = self._stage[self._turn]
        if buf is None or buf[0].numel() < nbytes or (buf[1] is not None and not buf[1].query()):
            buf = self._stage[self._turn] = [torch.empty(max(nbytes, 1 << 22), dtype=torch.uint8).pin_memory(), None]
        self._turn = (self._turn + 1) % len(self._stage)
        return buf

    def matrices(self, joints, n_persons, sizes, rng=random):
        """One draw and one matrix per image -> (params list, mats (N,3,3) float64)."""
        params = [self.transform.draw(rng) for _ in sizes]
        mats = np.stack([self.transform.affine_matrix(p, roi_center(joints[i], n_persons[i], np.array([w, h])), np.array([w, h]))
                         for i, (p, (h, w)) in enumerate(zip(params, sizes))])
        return params, mats

    def __call__(self, raw_images, joints, n_persons, mask_miss=None, rng=random):
        joints = np.ascontiguousarray(joints, np.float32)
        n_persons = np.ascontiguousarray(n_persons, np.int32)
        n, S = len(raw_images), self.size
        assert joints.ndim == 4 and joints.shape[0] == n and joints.shape[3] == 4 and n_persons.shape == (n,)
        sizes = [(int(im.shape[0]), int(im.shape[1])) for im in raw_images]
        self.last_params, mats = self.matrices(joints, n_persons, sizes, rng)
        self.last_photo = None
        if self.photo_params is not None and self.photo_params.steps():
            self.last_photo = draw_photo(self.photo_params, n_persons, joints.shape[2], rng, self.np_rng)
        return self.apply(raw_images, joints, n_persons, mats, self.last_params, mask_miss, self.last_photo)

    def apply(self, raw_images, joints, n_persons, mats, params, mask_miss=None, photo=None):
        """The device work for given matrices (and the draws they came from: flip and the scales go to the keypoints) and, if any,
        the photometric draws (draw_photo's list of dicts)."""
        lib = _lib.load()
        n, S, dev = len(raw_images), self.size, self.device
        if dev.type != 'cuda':
            raise _lib.OgError(f'DeviceAugment: device is {dev}; the HIP kernels need a GPU (offsetguided_amd has no CPU path)')
        sizes = [(int(im.shape[0]), int(im.shape[1])) for im in raw_images]
        D = np.stack([inverse_rows(m, S) for m in mats])                       # raises before anything is queued
        M = np.ascontiguousarray(np.asarray(mats, np.float64)[:, 0:2])
        img_bytes = sum(h * w * 3 for h, w in sizes)
        mask_at = _align16(img_bytes)
        on_device = hasattr(mask_miss, 'buffer') and hasattr(mask_miss, 'offsets')          # data.DeviceMasks
        mask_bytes = sum(h * w for h, w in sizes) if mask_miss is not None and not on_device else 0
        joints_at = _align16(mask_at + mask_bytes)
        np_at = _align16(joints_at + joints.nbytes)
        total = np_at + n_persons.nbytes
        table = photo_table(photo) if photo else None
        jpeg = sorted({d['jpeg'] for d in photo if d['jpeg'] is not None}) if photo else []
        jittered = [i for i, d in enumerate(photo) if d['jitter'] is not None] if photo else []
        noise_at, noise_bytes = _align16(total), joints.nbytes // 2
        if jittered:
            total = noise_at + noise_bytes
        stage = self._staging(total)
        stage_np = stage[0].numpy()
        offs, hw4, o = (C.c_long * n)(), (C.c_int * (4 * n))(), 0
        for i, (im, (h, w)) in enumerate(zip(raw_images, sizes)):
            assert im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3, 'images are (h, w, 3) uint8 RGB'
            np.copyto(stage_np[o:o + h * w * 3].reshape(h, w, 3), im)
            offs[i] = o
            hw4[4 * i:4 * i + 4] = [h, w, 0, 0]
            o += h * w * 3
        moffs, o = (C.c_long * n)(), 0
        if on_device:
            assert list(mask_miss.sizes) == sizes, 'mask_miss: the planes of a DeviceMasks have the images\' sizes'
            assert mask_miss.buffer.device == dev, 'mask_miss: the DeviceMasks lives on another device'
            moffs[:] = [int(o) for o in mask_miss.offsets]
        elif mask_miss is not None:
            assert len(mask_miss) == n
            for i, (m, (h, w)) in enumerate(zip(mask_miss, sizes)):
                assert m.dtype == np.uint8 and m.shape == (h, w), 'mask_miss: (h, w) uint8 of the image\'s size'
                np.copyto(stage_np[mask_at + o:mask_at + o + h * w].reshape(h, w), m)
                moffs[i] = o
                o += h * w
        stage_np[joints_at:joints_at + joints.nbytes] = joints.reshape(-1).view(np.uint8)
        stage_np[np_at:np_at + n_persons.nbytes] = n_persons.view(np.uint8)
        if jittered:
            noise = stage_np[noise_at:noise_at + noise_bytes].view(np.float32).reshape(joints.shape[:3] + (2,))
            noise[:] = 0
            for i in jittered:
                noise[i, :int(n_persons[i])] = photo[i]['jitter']
        dev_raw = torch.empty(total, dtype=torch.uint8, device=dev)
        dev_raw.copy_(stage[0][:total], non_blocking=True)
        stage[1] = torch.cuda.Event()
        stage[1].record(torch.cuda.current_stream(dev))
        stream = _lib.stream_ptr(dev)
        Dc = D.ctypes.data_as(C.c_void_p)
        images = torch.empty((n, 3, S, S), dtype=torch.float32, device=dev)
        if table is not None and (table[:, 0].any() or jpeg):
            warped = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev) if jpeg else None
            tc = table.ctypes.data_as(C.c_void_p)
            _lib.check(lib.og_warp_affine_photo_batch_u8(_lib.ptr(dev_raw), offs, hw4, n, Dc, S, self._border, self._mean, self._std,
                                                         _lib.ptr(images), _lib.ptr(warped) if jpeg else None, tc, stream), lib)
            for quality in jpeg:
                sel = [i for i, d in enumerate(photo) if d['jpeg'] == quality]
                _lib.check(lib.og_jpeg_roundtrip_batch_u8(_lib.ptr(warped), n, S, (C.c_int * len(sel))(*sel), len(sel), int(quality), tc,
                                                          self._mean, self._std, _lib.ptr(images), stream), lib)
        else:
            _lib.check(lib.og_warp_affine_batch_u8(_lib.ptr(dev_raw), offs, hw4, n, Dc, S, self._border, self._mean, self._std,
                                                   _lib.ptr(images), None, stream), lib)
        mask = None
        if mask_miss is not None:
            mask = torch.empty((n, S, S), dtype=torch.uint8, device=dev)
            planes = mask_miss.buffer if on_device else dev_raw[mask_at:]
            _lib.check(lib.og_warp_affine_mask_u8(_lib.ptr(planes), moffs, hw4, n, Dc, S, self.mask_border, _lib.ptr(mask), stream), lib)
        joints_dev = dev_raw[joints_at:joints_at + joints.nbytes].view(torch.float32).view(joints.shape)
        np_dev = dev_raw[np_at:np_at + n_persons.nbytes].view(torch.int32)
        out_joints = torch.empty(joints.shape, dtype=torch.float32, device=dev)
        if joints.shape[1] > 0:
            flips = (C.c_int * n)(*[int(bool(p[0])) for p in params])
            scales = (C.c_double * n)(*[math.sqrt((p[3] * p[2]) * (p[4] * p[2])) for p in params])
            jargs = (_lib.ptr(joints_dev), _lib.ptr(np_dev), n, joints.shape[1], joints.shape[2], M.ctypes.data_as(C.c_void_p), flips,
                     scales, float(self.transform.in_size[0]), float(self.transform.in_size[1]), self._left, self._right, len(self._left))
            if jittered:
                pp = self.photo_params
                gate = (C.c_int * n)(*[int(d['jitter'] is not None) for d in photo])
                eps, shift = (C.c_float * n)(*[float(pp.jitter_epsilon)] * n), (C.c_float * n)(*[float(pp.jitter_shift)] * n)
                _lib.check(lib.og_affine_joints_jitter_f32(*jargs, _lib.ptr(dev_raw[noise_at:]), gate, eps, shift, _lib.ptr(out_joints),
                                                           stream), lib)
            else:
                _lib.check(lib.og_affine_joints_f32(*jargs, _lib.ptr(out_joints), stream), lib)
        return images, out_joints, mask, np.asarray(mats, np.float64)
