#!/usr/bin/env python3
"""Golden vectors for the training augmentation from the imported reference (transforms/affine.py; build container only):
tests/golden/augment_affine.npz.  cv2 is stubbed -- its warpAffine hands the image back untouched --, so WarpAffineTransforms.__call__
runs its own parameter draws, _roi_center, _get_affine_mat and _affine_keypoints, none of which touches cv2.  64 cases, each under
random.seed(case): the command line's default parameters, FixedAugParams and crop_roi=False in turn; three source sizes; 1-6 persons
with mixed visibility and one image without any person.  Arrays only: per case the source size, the input annotations, the seven drawn
parameters, roi_center, the 3x3 matrix, the transformed annotations and the joint_channel_ind permutation, stacked over the cases
(annotations padded to six persons, `n_persons` says how many are real).

    usage: python tools/gen_golden_augment.py        (OG_REFERENCE = the reference checkout)"""
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

GOLD = os.path.join(ROOT, 'tests', 'golden')
CASES, S, MARGIN = 64, 512, 1e-3
SOURCES = ((640, 480), (427, 640), (333, 500))      # (width, height)


def load_reference_affine():
    """The reference's transforms/affine.py from its checkout, imported when the fixture is generated (nothing at module level needs
    it).  Its package __init__ wants torchvision: an empty stand-in package with the checkout's path loads the one module."""
    from tools.gen_golden import REF
    cv2 = types.ModuleType('cv2')
    cv2.warpAffine = lambda image, *a, **k: image
    cv2.INTER_CUBIC, cv2.BORDER_CONSTANT = 2, 0
    saved = {k: sys.modules.get(k) for k in ('cv2', 'transforms')}
    sys.modules['cv2'] = cv2
    pkg = types.ModuleType('transforms')
    pkg.__path__ = [os.path.join(REF, 'transforms')]
    sys.modules['transforms'] = pkg
    sys.path.insert(0, REF)
    try:
        import importlib
        mod = importlib.import_module('transforms.affine')
    finally:
        sys.path.remove(REF)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def default_params():
    """The training defaults of the reference's command line (data/factory.py:84-104)."""
    return types.SimpleNamespace(flip_prob=0.5, max_rotate=45, min_scale=0.5, max_scale=2.0, min_stretch=0.95, max_stretch=1.05,
                                 max_translate=150)


def random_annotations(rs, persons, w, h):
    """(P,17,4) fp32 [x, y, v, scale]: people inside the source, a quarter of the keypoints unannotated, quarter-pixel coordinates."""
    j = np.zeros((persons, 17, 4), np.float32)
    cx, cy = rs.uniform(0.2 * w, 0.8 * w, persons), rs.uniform(0.2 * h, 0.8 * h, persons)
    ext = rs.uniform(20, 0.35 * min(w, h), persons)
    j[:, :, 0] = np.clip(cx[:, None] + rs.uniform(-1, 1, (persons, 17)) * ext[:, None], 1, w - 2)
    j[:, :, 1] = np.clip(cy[:, None] + rs.uniform(-1, 1, (persons, 17)) * ext[:, None], 1, h - 2)
    j[:, :, :2] = np.round(j[:, :, :2] * 4) / 4
    j[:, :, 2] = (rs.uniform(0, 1, (persons, 17)) > 0.25) * rs.randint(1, 3, (persons, 17))
    j[:, :, 3] = rs.uniform(0.8, 22, (persons, 17))
    return j


def run_case(ref, case, attempt):
    kind = case % 3                                      # 0: default draws, 1: FixedAugParams, 2: default draws, crop_roi=False
    w, h = SOURCES[(case // 3) % 3]
    persons = 0 if case == 63 else 1 + case % 6
    rs = np.random.RandomState(7000 + 64 * attempt + case)
    anns = random_annotations(rs, persons, w, h)
    t = ref.WarpAffineTransforms(S, aug_params=ref.FixedAugParams() if kind == 1 else default_params(), crop_roi=kind != 2)
    meta = {'width_height': np.array([w, h]), 'scale': np.array([1., 1.]), 'rotate': 0., 'hflip': False,
            'affine3×3mat': np.eye(3), 'joint_channel_ind': np.arange(17)}
    roi = ref._roi_center(anns, meta)
    random.seed(case)
    _, out, meta2, _ = t(np.zeros((h, w, 3), np.uint8), anns, meta, None)
    xy = out[:, :, :2].astype(np.float64)
    ok = bool((np.abs(xy) >= MARGIN).all() and (np.abs(xy - S) >= MARGIN).all())
    params = np.array([float(t.flip), t.rotate, t.scale, t.x_stretch, t.y_stretch, float(t.x_offset), float(t.y_offset)], np.float64)
    return ok, {'wh': np.array([w, h], np.int32), 'kind': np.int32(kind), 'joints': anns, 'params': params,
                'roi': np.asarray(roi, np.float32), 'mat': np.asarray(meta2['affine3×3mat'], np.float64),
                'out': np.asarray(out, np.float32), 'perm': np.asarray(meta2['joint_channel_ind'], np.int32)}


def main():
    ref = load_reference_affine()
    out = {}
    for case in range(CASES):
        for attempt in range(50):                        # new annotations until no coordinate sits within MARGIN of 0 or S
            ok, arrays = run_case(ref, case, attempt)
            if ok:
                break
        assert ok, f'case {case}: a transformed coordinate within {MARGIN} of 0 or {S}: the visibility flags would hinge on rounding'
        for k, v in arrays.items():
            out.setdefault(k, []).append(v)
    # one array per field (a zip member per case and field would be mostly zip headers): annotations padded to 6 persons
    out['n_persons'] = np.array([len(j) for j in out['joints']], np.int32)
    for k in ('joints', 'out'):
        out[k] = np.stack([np.concatenate([j, np.zeros((6 - len(j), 17, 4), np.float32)]) for j in out[k]])
    out = {k: np.stack(v) if isinstance(v, list) else v for k, v in out.items()}
    path = os.path.join(GOLD, 'augment_affine.npz')
    np.savez_compressed(path, **out)
    flips = int(out['params'][:, 0].sum())
    print(f'{path}: {CASES} cases, {flips} flipped, {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
