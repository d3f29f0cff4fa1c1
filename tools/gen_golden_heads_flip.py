#!/usr/bin/env python3
"""Generate tests/golden/heads_flip.npz by running the IMPORTED reference decoder: flip-test with BOTH optional heads at once
(keypoint-scale and jitter-offset), which no other fixture covers.

Runs only where the reference checkout is available (the same import shim as tools/gen_golden.py).  Stored: the reference's
flip_augment outputs for the scale and jitter maps (bit-exact targets of og_flip_merge_heads_f32) and the poses of
generate_poses(flip_test=True) with both heads and use_scale=True.  The inputs come from the portable generator
offsetguided_amd/synth.py through heads_flip_inputs below (the one function tests share with this tool) and are not stored;
their sha256 is.

Conditions on the inputs, asserted here before the file is written: every image yields at least one pose, and the poses differ
between use_scale on and off -- otherwise the merged scale head would never be observed in the result.

usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_heads_flip.py
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from offsetguided_amd import synth  # noqa: E402

SEED, BATCH, SIZE, PERSONS = 811, 2, 192, 6
FLAGS = dict(topk=32, thre_hmp=0.04, person_thre=0.04, dist_max=6.0, min_len=0.5)


def heads_flip_inputs(seed=SEED, batch=BATCH, size=SIZE, n_persons=PERSONS):
    """(hm, off, scl, jit) for [images | mirrored images]: synthetic persons plus a keypoint-scale head of 5..45 px and a jitter head of
    +-1.5 px (the ranges of gen_golden.py's scale_case / jitter_case)."""
    hm, off = synth.synth_batch(seed, batch, size, size, flip=True, n_persons=n_persons)
    nb = hm.shape[0]
    scl = (synth.noise_batch(seed + 5, (nb, 17, size // 4, size // 4)) * 20 + 25).astype(np.float32)
    jit = ((synth.noise_batch(seed + 9, (nb, 2, size // 4, size // 4)) - 0.5) * 3.0).astype(np.float32)
    return hm, off, scl, jit


def main():
    import gen_golden as G
    decoder = G.load_reference()

    def processor(use_scale):
        p = argparse.ArgumentParser()
        decoder.decoder_cli(p)
        a = p.parse_args(['--topk', str(FLAGS['topk']), '--thre-hmp', str(FLAGS['thre_hmp']), '--person-thre', str(FLAGS['person_thre']),
                          '--dist-max', str(FLAGS['dist_max']), '--min-len', str(FLAGS['min_len']), '--use-scale', str(use_scale),
                          '--use-jitter-offset', 'True'])
        a.headnets, a.strides, a.batch_size = ['hmp', 'omp'], [4, 4], BATCH
        a.include_scale = a.include_jitter_offset = True
        return decoder.decoder_factory(a)

    hm, off, scl, jit = heads_flip_inputs()
    t = torch.from_numpy
    feats = [([t(hm) * 0, t(hm)], [[], []], [t(jit) * 0, t(jit)]), ([t(off) * 0, t(off)], [[], []], [t(scl) * 0, t(scl)])]
    proc = processor(True)
    _, jomps, _, scmps, _ = proc.flip_augment(t(hm), t(jit), t(off), t(scl), False, 2)
    poses = proc.generate_poses(feats, flip_test=True)
    proc.worker_pool.close()
    plain = processor(False)
    poses_off = plain.generate_poses(feats, flip_test=True)
    plain.worker_pool.close()
    assert all(len(q) >= 1 for q in poses), f'an image without a pose: {[len(q) for q in poses]}'
    assert any(a.shape != b.shape or not np.array_equal(a, b) for a, b in zip(poses, poses_off)), \
        'use_scale on / off give the same poses: the scale head is not observed'
    out = os.path.join(G.GOLD, 'heads_flip.npz')
    np.savez_compressed(out, seed=SEED, batch=BATCH, size=SIZE, n_persons=PERSONS, flags=np.array(sorted(FLAGS.items()), dtype=object).astype(str),
                        in_sha=np.array([G.sha(hm), G.sha(off), G.sha(scl), G.sha(jit)]), scmps_merged=scmps.numpy(), jomps_merged=jomps.numpy(),
                        n_poses=np.array([len(q) for q in poses]), poses=np.concatenate(poses, 0).astype(np.float32),
                        n_poses_no_scale=np.array([len(q) for q in poses_off]))
    print(f'heads_flip: poses/img {[len(q) for q in poses]} (use_scale off: {[len(q) for q in poses_off]}), {os.path.getsize(out)} bytes')


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
