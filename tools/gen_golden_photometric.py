#!/usr/bin/env python3
"""Golden vectors for the photometric training augmentation from the imported reference (transforms/random.py, transforms/image.py;
build container only): tests/golden/augment_photometric.npz.  cv2 is stubbed -- its cvtColor hands the image back untouched --, so
ColorTint on a constant-128 image yields its three deltas directly (128 - 40 ... 128 + 40 never clamps).  64 cases, each under
random.seed(case); np.random.seed(case):
  * `prob`, `gate`, `deltas`: RandomApply(ColorTint(), prob) with prob 0.2 / 0.5 / 0.9 in turn: whether the step ran, and (dh, ds, dv)
    (zeros where it did not);
  * `chain_gates`, `chain_deltas`: after a new seeding, RandomApply(JpegCompression(), 0.5) then RandomApply(ColorTint(), 0.5) on one
    image, the order of the reference's training chain (data/factory.py:250-265): both gates and the tint's deltas.
Arrays only.

    usage: python tools/gen_golden_photometric.py        (OG_REFERENCE = the reference checkout)"""
import importlib
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

GOLD = os.path.join(ROOT, 'tests', 'golden')
CASES = 64
PROBS = (0.2, 0.5, 0.9)


def load_reference_transforms():
    """The reference's transforms/random.py and transforms/image.py from its checkout.  Its package __init__ is not run (an empty
    stand-in package with the checkout's path loads the two modules); cv2 is a stub, and so is whatever else image.py imports at
    module level and this machine lacks (scipy, torchvision: neither is used by the steps run here)."""
    from tools.gen_golden import REF
    cv2 = types.ModuleType('cv2')
    cv2.cvtColor = lambda image, code: image
    cv2.COLOR_RGB2HSV, cv2.COLOR_HSV2RGB, cv2.COLOR_RGB2GRAY = 41, 55, 7
    stubs = {'cv2': cv2}
    for name in ('scipy', 'scipy.ndimage', 'torchvision'):
        try:
            importlib.import_module(name)
        except ImportError:
            stubs[name] = types.ModuleType(name)
    if 'scipy' in stubs:
        stubs['scipy'].ndimage = stubs['scipy.ndimage']
    pkg = types.ModuleType('transforms')
    pkg.__path__ = [os.path.join(REF, 'transforms')]
    stubs['transforms'] = pkg
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    sys.path.insert(0, REF)
    try:
        rnd = importlib.import_module('transforms.random')
        img = importlib.import_module('transforms.image')
    finally:
        sys.path.remove(REF)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return rnd, img


def seed(case):
    random.seed(case)
    np.random.seed(case)


def main():
    rnd, img = load_reference_transforms()
    out = {k: [] for k in ('prob', 'gate', 'deltas', 'chain_gates', 'chain_deltas')}
    for case in range(CASES):
        prob = PROBS[case % 3]
        flat = np.full((16, 16, 3), 128, np.uint8)
        seed(case)
        res = rnd.RandomApply(img.ColorTint(), prob)(flat, None, None, None)[0]
        ran = res is not flat
        out['prob'].append(prob)
        out['gate'].append(ran)
        out['deltas'].append(res[0, 0].astype(np.int32) - 128 if ran else np.zeros(3, np.int32))
        seed(case)
        a = rnd.RandomApply(img.JpegCompression(), 0.5)(flat, None, None, None)[0]
        b = rnd.RandomApply(img.ColorTint(), 0.5)(a, None, None, None)[0]
        out['chain_gates'].append([a is not flat, b is not a])
        out['chain_deltas'].append(b[0, 0].astype(np.int32) - a[0, 0].astype(np.int32) if b is not a else np.zeros(3, np.int32))
    arrays = {'prob': np.array(out['prob'], np.float64), 'gate': np.array(out['gate'], bool),
              'deltas': np.stack(out['deltas']).astype(np.int32), 'chain_gates': np.array(out['chain_gates'], bool),
              'chain_deltas': np.stack(out['chain_deltas']).astype(np.int32)}
    path = os.path.join(GOLD, 'augment_photometric.npz')
    np.savez_compressed(path, **arrays)
    print(f"{path}: {CASES} cases, {int(arrays['gate'].sum())} tinted, chain gates {arrays['chain_gates'].sum(axis=0).tolist()}, "
          f'{os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
