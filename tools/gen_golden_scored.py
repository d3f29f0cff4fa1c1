#!/usr/bin/env python3
"""Generate the scored_off fixtures (tests/golden/scored256_flip.npz, scored_fn.npz) by running the IMPORTED reference.

  scored256_flip.npz  reference generate_poses(flip_test=True, scored_off=True) on synth.synth_batch(seed, 2, 256, 256, flip=True,
                      n_persons=6): seed, input shas, sha of the reference's refined offsets (scored_offset on the maps its
                      flip_augment merged), poses.  Asserted while generating: every image yields >= 3 poses and the poses differ
                      from the same call with scored_off=False (a keypoint coordinate or a limb score), so the fixture is not vacuous.
                      The same two conditions are checked (and printed, not asserted) for the inputs of the existing scored256.npz.
  scored_fn.npz       sha256 of the reference function's output for kernel_size 1 / 5 / 7 on two odd shapes (synth.noise_batch
                      inputs; the heat maps carry negative values, as the network produces them, and an all-zero plane).

Needs the reference checkout (OG_REFERENCE); the GPU machine never sees it.   usage: python tools/gen_golden_scored.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FN_SHAPES = [(2, 17, 7, 61), (3, 17, 24, 40)]      # (N, C, h, w), 19 limbs of the COCO skeleton; N >= 2: the reference squeezes batch 1 away
FN_KS = [1, 5, 7]
FLIP_SEED, FLIP_PERSONS = 511, 6


def fn_inputs(shape, seed):
    """Heat maps (negative values included, plane 5 all zero) and offsets of one scored_fn case."""
    from offsetguided_amd import synth
    n, c, h, w = shape
    hm = synth.noise_batch(seed, shape, 0.3)
    hm[:, 5] = 0.0
    off = synth.noise_batch(seed + 1, (n, 38, h, w), 4.0)
    return hm, off


def poses_differ(a, b):
    return any(x.shape != y.shape or not np.array_equal(x[..., [0, 1, 4]], y[..., [0, 1, 4]]) for x, y in zip(a, b))


def main():
    import torch
    from tools import gen_golden as G
    from offsetguided_amd import synth
    from offsetguided_amd.config.coco_data import COCO_PERSON_SKELETON
    from offsetguided_amd.decoder.offset import scored_offset as mine
    decoder = G.load_reference()
    jf, jt = decoder.offset.pack_jtypes(COCO_PERSON_SKELETON)

    # ---- the function itself, other windows and odd shapes
    out = {}
    for i, shape in enumerate(FN_SHAPES):
        hm, off = fn_inputs(shape, 700 + 10 * i)
        out[f'in_sha_{i}'] = np.array([G.sha(hm), G.sha(off)])
        for ks in FN_KS:
            ref = decoder.scored_offset(torch.from_numpy(hm), torch.from_numpy(off), jf, jt, kernel_size=ks)
            assert torch.equal(ref, mine(torch.from_numpy(hm), torch.from_numpy(off), jf, jt, kernel_size=ks)), (shape, ks)
            out[f'sha_{i}_k{ks}'] = np.array(G.sha(ref.numpy()))
    np.savez_compressed(os.path.join(G.GOLD, 'scored_fn.npz'), shapes=np.array(FN_SHAPES), ks=np.array(FN_KS), **out)
    print('scored_fn: reference == CPU formulation for', FN_SHAPES, FN_KS)

    # ---- the existing fixture's inputs: is scored256.npz vacuous?
    hm, off = synth.synth_batch(501, 2, 256, 256, n_persons=6)
    proc = G.ref_processor(decoder, 2)
    on = proc.generate_poses(G.features(hm, off), scored_off=True)
    plain = proc.generate_poses(G.features(hm, off), scored_off=False)
    print(f'scored256 inputs: poses/img {[len(q) for q in on]}, every image >= 3 poses: {all(len(q) >= 3 for q in on)}, '
          f'differs from scored_off=False: {poses_differ(on, plain)}')

    # ---- flip-test + scored_off
    hm, off = synth.synth_batch(FLIP_SEED, 2, 256, 256, flip=True, n_persons=FLIP_PERSONS)
    on = proc.generate_poses(G.features(hm, off), flip_test=True, scored_off=True)
    plain = proc.generate_poses(G.features(hm, off), flip_test=True, scored_off=False)
    proc.worker_pool.close()
    assert all(len(q) >= 3 for q in on), [len(q) for q in on]
    assert poses_differ(on, plain), 'scored_off changes nothing on these inputs: pick another seed / n_persons'
    m_hm, _, m_off, _, _ = proc.flip_augment(torch.from_numpy(hm), [], torch.from_numpy(off), [], False, 2)
    ref = decoder.scored_offset(m_hm, m_off, jf, jt, kernel_size=3)
    np.savez_compressed(os.path.join(G.GOLD, 'scored256_flip.npz'), seed=FLIP_SEED, batch=2, size=256, n_persons=FLIP_PERSONS,
                        in_sha=np.array([G.sha(hm), G.sha(off)]), scored_sha=np.array(G.sha(ref.numpy())),
                        n_poses=np.array([len(q) for q in on]), poses=np.concatenate(on, 0))
    print(f'scored256_flip: poses/img {[len(q) for q in on]}, differs from scored_off=False')


if __name__ == '__main__':
    main()
