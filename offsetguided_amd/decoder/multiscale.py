"""Multi-scale test (beyond the reference, which reserves --two-scale / --multi-scale as "to be implemented", models/factory.py:21-24):
the network runs at several input scales, the head outputs of every scale are resampled onto the grid of scale 1 and averaged there,
and the averaged maps are decoded once by the unchanged PostProcess (flip_test=False: a flip pair is merged per scale, before the
resample).

scale_affines: the per-image table (Ax, Bx, Ay, By, inv_ax, inv_ay) that maps a base grid cell onto the grid of one scale, from the
metas the input chain wrote (transforms.EvalPreprocess.multi_scale): base cell centre -> original image (annotations_inverse) ->
scale-s input (rescale + pad) -> scale-s grid.  merge_scales: one og_scale_accumulate_f32 launch per scale into base-grid accumulators.

scored_off (--scored-off) composes: after the merge the decode is the ordinary one, refinement inside the pairing included.
The keypoint-scale and jitter-offset heads ride in the same launch (og_scale_accumulate_heads_f32): a jitter offset changes units as
the guiding offsets do (inv_ax, inv_ay), a keypoint scale is a length in scale-s input pixels and is multiplied by
sqrt(inv_ax * inv_ay), the convention evaluate.annotations_inverse applies to column 3.
Not served together with more than one scale: cat_flip_offs and --fixed-height (RightDownPad metas)."""
import numpy as np
import torch

from .. import _lib
from ..config import heatmap_hflip, offset_hflip
from ..config.coco_data import COCO_KEYPOINTS, COCO_PERSON_SKELETON

MODE_WRITE, MODE_ADD, MODE_ADD_SCALE = 0, 1, 2


def scale_affines(base_metas, scale_metas, base_hw, scale_hw, stride=4, dtype=np.float32):
    """(N, 6) table of base-grid -> scale-grid maps, one row per image: Ax, Bx, Ay, By, inv_ax, inv_ay.

    Per axis, with c = stride/2 - 0.5 (the encoder's cell centre) and the metas' (offset, scale):
      X_b = stride*j + c;  x = (X_b + off_b) / sc_b;  X_s = x*sc_s - off_s;  u = (X_s - c) / stride
    folded into u = A*j + B with A = sc_s/sc_b, B = (c*(A - 1) + off_b*A - off_s) / stride (float64, rounded to `dtype` once:
    the table of a scale whose metas ARE the base metas is exactly (1, 0, 1, 0, 1, 1)).  inv_a = sc_b/sc_s turns an offset measured
    on the scale-s grid into one on the base grid.  base_hw / scale_hw: the (h, w) grids, checked against the metas' padded sizes."""
    if len(base_metas) != len(scale_metas):
        raise ValueError(f'{len(base_metas)} base metas, {len(scale_metas)} scale metas')
    c = stride / 2 - 0.5
    rows = []
    for mb, ms in zip(base_metas, scale_metas):
        for m, (gh, gw) in ((mb, base_hw), (ms, scale_hw)):
            wh = m.get('width_height')
            if wh is not None and (int(wh[0]) != gw * stride or int(wh[1]) != gh * stride):
                raise ValueError(f'meta of padded size {tuple(int(v) for v in wh)} does not give the grid {(gh, gw)} at stride {stride}')
        row = []
        for ax in (0, 1):
            sb, ss = float(mb['scale'][ax]), float(ms['scale'][ax])
            ob, os_ = float(mb['offset'][ax]), float(ms['offset'][ax])
            a = ss / sb
            row += [a, (c * (a - 1.0) + ob * a - os_) / stride]
        row += [float(mb['scale'][0]) / float(ms['scale'][0]), float(mb['scale'][1]) / float(ms['scale'][1])]
        rows.append(row)
    return np.array(rows, np.float64).astype(dtype)


def merge_scales(outputs_per_scale, affines_per_scale, flip_test, out=None, base_hw=None, keypoints=COCO_KEYPOINTS,
                 skeleton=COCO_PERSON_SKELETON, n_stacks=1):
    """Average the head outputs of several scales on the base grid.

    outputs_per_scale: per scale (hm (F*N, C, hs, ws), off (F*N, 2L, hs, ws)) fp32 device tensors (InferenceEngine.forward_raw), F = 2
    with flip_test ([images | mirrored images], merged as og_flip_merge_f32 merges them), else 1; or 4-tuples (hm, off, scl, jit) with
    the keypoint-scale maps scl (F*N, C, hs, ws) and the jitter maps jit (F*N, 2, hs, ws), each a tensor or None, the same heads at
    every scale (merged under flip_test as og_flip_merge_heads_f32 merges them).  affines_per_scale: per scale the
    (N, 6) table of scale_affines (device fp32 tensor, or a host array that is copied over).  out: caller-owned accumulators
    (hm (N, C, h, w), off (N, 2L, h, w)) fp32 -- with heads (hm, off, scl (N, C, h, w) | None, jit (N, 2, h, w) | None) -- or None for
    new ones of base_hw = (h, w).  The sum follows the order of the list; the last
    launch multiplies by 1/S.  One launch per scale on the current stream.

    Returns the reference nesting [(hms, jomps, ...), (offs, ...)] at the base grid for PostProcess.submit(..., flip_test=False): hms /
    offs are lists of n_stacks entries that all hold the merged map; with heads the merged jitter map fills slot 2 of the heatmap
    tuple and the merged scale map slot 2 of the offset tuple, as PostProcess.generate_limbs unpacks them."""
    S = len(outputs_per_scale)
    if S == 0 or S != len(affines_per_scale):
        raise ValueError(f'{S} outputs for {len(affines_per_scale)} affine tables')
    if any(len(o) not in (2, 4) for o in outputs_per_scale):
        raise ValueError('every scale gives (hm, off) or (hm, off, scl, jit) with scl / jit a tensor or None')
    heads = [tuple(isinstance(t, torch.Tensor) for t in (tuple(o) + (None, None))[2:4]) for o in outputs_per_scale]
    if any(hd != heads[0] for hd in heads):
        raise ValueError(f'the keypoint-scale / jitter heads must be the same at every scale, got {heads}')
    has_scl, has_jit = heads[0]
    hm0 = _lib.require_device(outputs_per_scale[0][0], 'hm')
    dev = hm0.device
    F = 2 if flip_test else 1
    N, C = hm0.shape[0] // F, hm0.shape[1]
    L = outputs_per_scale[0][1].shape[1] // 2
    if out is None:
        if base_hw is None:
            raise ValueError('merge_scales needs the base grid: out=(hm, off) accumulators or base_hw=(h, w)')
        h, w = base_hw
        out = (torch.empty((N, C, h, w), dtype=torch.float32, device=dev), torch.empty((N, 2 * L, h, w), dtype=torch.float32, device=dev))
        if has_scl or has_jit:
            out += (torch.empty((N, C, h, w), dtype=torch.float32, device=dev) if has_scl else None,
                    torch.empty((N, 2, h, w), dtype=torch.float32, device=dev) if has_jit else None)
    hm_acc, off_acc, scl_acc, jit_acc = (tuple(out) + (None, None))[:4]
    if (scl_acc is not None) != has_scl or (jit_acc is not None) != has_jit:
        raise ValueError('accumulators and outputs disagree about the keypoint-scale / jitter heads')
    h, w = hm_acc.shape[2:]
    if (tuple(hm_acc.shape) != (N, C, h, w) or tuple(off_acc.shape) != (N, 2 * L, h, w) or hm_acc.dtype != torch.float32
            or off_acc.dtype != torch.float32 or not hm_acc.is_contiguous() or not off_acc.is_contiguous()):
        raise ValueError(f'accumulators {tuple(hm_acc.shape)} / {tuple(off_acc.shape)} do not fit N={N}, C={C}, L={L}')
    inv = float(np.float32(1.0) / np.float32(S))
    for s, (o, aff) in enumerate(zip(outputs_per_scale, affines_per_scale)):
        mode = MODE_WRITE if s == 0 else (MODE_ADD_SCALE if s == S - 1 else MODE_ADD)
        scl, jit = (tuple(o) + (None, None))[2:4]
        accumulate_scale(o[0], o[1], aff, out, mode, inv, flip_test, keypoints, skeleton, scl=scl, jit=jit)
    return merged_features(out, n_stacks)


def merged_features(out, n_stacks=1):
    """The reference nesting [(hms, [], jomps), (offs, [], scmps)] over accumulators (hm, off[, scl | None, jit | None])."""
    hm_acc, off_acc, scl_acc, jit_acc = (tuple(out) + (None, None))[:4]
    empty = [[] for _ in range(n_stacks)]
    return [([hm_acc] * n_stacks, list(empty), [jit_acc] * n_stacks if jit_acc is not None else list(empty)),
            ([off_acc] * n_stacks, list(empty), [scl_acc] * n_stacks if scl_acc is not None else list(empty))]


def accumulate_scale(hm, off, aff, out, mode, inv_count, flip_test, keypoints=COCO_KEYPOINTS, skeleton=COCO_PERSON_SKELETON, scl=None,
                     jit=None):
    """ONE launch on the current stream: the maps of one scale (hm (F*N, C, hs, ws), off (F*N, 2L, hs, ws), F = 2 with flip_test)
    resampled with the (N, 6) table `aff` into out = (hm_acc (N, C, h, w), off_acc (N, 2L, h, w)); mode MODE_WRITE / MODE_ADD /
    MODE_ADD_SCALE (the last scale: the sum times inv_count).  og_scale_accumulate_f32, or with scl (F*N, C, hs, ws) and / or jit
    (F*N, 2, hs, ws) og_scale_accumulate_heads_f32 into out = (hm_acc, off_acc, scl_acc | None, jit_acc | None)."""
    lib = _lib.load()
    hm_acc, off_acc, scl_acc, jit_acc = (tuple(out) + (None, None))[:4]
    if (scl is None) != (scl_acc is None) or (jit is None) != (jit_acc is None):
        raise ValueError('every keypoint-scale / jitter map needs its accumulator in `out`, and no accumulator goes without its map')
    hm, off = _lib.require_device(hm, 'hm'), _lib.require_device(off, 'off')
    dev = hm.device
    F = 2 if flip_test else 1
    N, C, h, w = hm_acc.shape
    L = off_acc.shape[1] // 2
    if (hm.shape[0] != F * N or hm.shape[1] != C or off.shape[0] != F * N or off.shape[1] != 2 * L or hm.shape[2:] != off.shape[2:]
            or tuple(off_acc.shape) != (N, 2 * L, h, w)):
        raise ValueError(f'maps {tuple(hm.shape)} / {tuple(off.shape)} do not fit the accumulators {tuple(hm_acc.shape)} / '
                         f'{tuple(off_acc.shape)} (flip: {flip_test})')
    scl = _lib.require_device(scl, 'scl') if scl is not None else None
    jit = _lib.require_device(jit, 'jit') if jit is not None else None
    for name, t, acc, ch in (('keypoint-scale', scl, scl_acc, C), ('jitter', jit, jit_acc, 2)):
        if t is not None and (tuple(t.shape) != (F * N, ch) + tuple(hm.shape[2:]) or tuple(acc.shape) != (N, ch, h, w)):
            raise ValueError(f'{name} maps {tuple(t.shape)} / accumulator {tuple(acc.shape)} do not fit N={N}, {ch} channels '
                             f'(flip: {flip_test})')
    for t in (hm_acc, off_acc, scl_acc, jit_acc):
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            raise ValueError('accumulators must be contiguous fp32 device tensors')
    if not isinstance(aff, torch.Tensor):
        aff = torch.from_numpy(np.ascontiguousarray(aff, np.float32)).pin_memory().to(dev, non_blocking=True)
    aff = _lib.require_device(aff, 'aff')
    if tuple(aff.shape) != (N, 6):
        raise ValueError(f'affine table {tuple(aff.shape)}, expected {(N, 6)}')
    kp = lp = keep = None
    if flip_test:
        limb_perm, reserve = offset_hflip(keypoints, skeleton)
        if len(keypoints) != C or len(limb_perm) != L:
            raise ValueError(f'skeleton of {len(limb_perm)} limbs / {len(keypoints)} keypoints for maps of {L} limbs / {C} keypoints')
        kp = _lib.int_table(heatmap_hflip(keypoints), dev)
        lp = _lib.int_table(limb_perm, dev)
        keep = _lib.int_table([1 if l in reserve else 0 for l in range(L)], dev)
    hs, ws = hm.shape[2:]
    ptr = lambda t: _lib.ptr(t) if t is not None else None  # noqa: E731
    with _lib.stage_timer('scale_merge', dev):        # (HIP events around the launch while _lib.profile_start() is on)
        if scl is not None or jit is not None:
            _lib.check(lib.og_scale_accumulate_heads_f32(_lib.ptr(hm), _lib.ptr(off), ptr(scl), ptr(jit), N, F - 1, C, L, hs, ws, ptr(kp),
                                                         ptr(lp), ptr(keep), _lib.ptr(aff), h, w, int(mode), float(inv_count),
                                                         _lib.ptr(hm_acc), _lib.ptr(off_acc), ptr(scl_acc), ptr(jit_acc),
                                                         _lib.stream_ptr(dev)), lib)
            return
        _lib.check(lib.og_scale_accumulate_f32(_lib.ptr(hm), _lib.ptr(off), N, F - 1, C, L, hs, ws, ptr(kp), ptr(lp), ptr(keep),
                                               _lib.ptr(aff), h, w, int(mode), float(inv_count), _lib.ptr(hm_acc), _lib.ptr(off_acc),
                                               _lib.stream_ptr(dev)), lib)
