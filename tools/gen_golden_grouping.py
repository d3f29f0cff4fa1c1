#!/usr/bin/env python3
"""Generate tests/golden/grouping_edges.npz by running the IMPORTED reference's GreedyGroup.group_skeletons on the directed cases of
tests/grouping_cases.py (planted limbs: rank ties on every body of the rank passes, validity limits, merges across the 64- and 16-row
seams, every configuration on every placement of the table, overflow, the _delete_sort threshold and ties, n_kp < 17).

Per case and image the reference runs with the case's configuration (and its keypoints / skeleton).  Asserted on the spot: the C
oracle and the traced restatement (oracle/restatement.py, trace=) give the reference's poses bit for bit, every coverage count of
grouping_cases.conditions is >= 1, and oracle.group_stats() over the whole set has every counter > 0.  Stored per case: the sha256
of the planted limbs (the tests rebuild them), per image the pose count and the sha256 of the pose bytes, and the poses themselves
for the images of fewer than 64 poses (float32, as they are).  Fixed zip time stamps: a second run gives the same bytes.

Reference pinning: _delete_reconns sorts with np.argsort's default kind.  In the numpy the reference targets (1.17) that is an
insertion sort up to 16 elements -- stable, the rule the oracle and K3 keep at every size; numpy 2 sorts float32 with a SIMD network
that is not stable even at 8 elements.  The generator hands the reference's module a numpy whose argsort defaults to kind='stable',
and the cases keep equal limb scores to limb types of at most 16 valid rows (grouping_cases.TIE_ROWS, 'ties_in_contract'), where
the two numpys agree by specification.

Needs the reference checkout (OG_REFERENCE); the GPU machine never sees it.   usage: python tools/gen_golden_grouping.py
"""
import contextlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

STORE_BELOW = 64      # poses per image


class PinnedNumpy:
    """numpy with argsort's default kind = 'stable' (see the module docstring)"""

    def __init__(self, np_):
        self._np = np_

    def __getattr__(self, name):
        return getattr(self._np, name)

    def argsort(self, a, *args, **kw):
        kw.setdefault('kind', 'stable')
        return self._np.argsort(a, *args, **kw)


def main():
    import oracle
    import grouping_cases as gc
    from tools import gen_golden as G
    from tools.gen_golden_pairing import save_npz
    decoder = G.load_reference()
    import decoder.group as reference_group
    reference_group.np = PinnedNumpy(np)
    out = {'names': np.array([c.name for c in gc.CASES])}
    oracle.group_stats(True)
    for case in gc.CASES:
        limbs, (sk, n_kp), cfg = gc.build(case), gc.skeleton(case), gc.CFGS[case.cfg]
        ref_group = decoder.GreedyGroup(cfg[0], sort_dim=int(cfg[3]), dist_max=cfg[1], use_scale=bool(cfg[2]),
                                        keypoints=[f'kp{j}' for j in range(n_kp)], skeleton=sk)
        traces, n_poses, shas = [], [], []
        for i, img in enumerate(limbs):
            with contextlib.redirect_stdout(io.StringIO()):          # ('usually this never happens ...' on cross3)
                ref = ref_group.group_skeletons(img.copy())
            mine = oracle.greedy_group(img, sk, n_kp, cfg[0], cfg[1], bool(cfg[2]), int(cfg[3]))
            restated, tr = gc.trace(img, sk, n_kp, cfg)
            assert ref.dtype == np.float32 and ref.shape == mine.shape and (ref == mine).all(), f'{case.name}/{i}: oracle != reference'
            assert ref.shape == restated.shape and (ref == restated).all(), f'{case.name}/{i}: restatement != reference'
            traces.append(tr)
            n_poses.append(len(ref))
            shas.append(G.sha(ref))
            if len(ref) < STORE_BELOW:
                out[f'{case.name}/poses_{i}'] = ref
        cnt = gc.counts(case, traces)
        assert all(v >= 1 for v in cnt.values()), f'{case.name}: a condition the case is built for does not occur: {cnt}'
        out[f'{case.name}/in_sha'] = np.array(gc.input_sha(case))
        out[f'{case.name}/n_poses'], out[f'{case.name}/poses_sha'] = np.array(n_poses), np.array(shas)
        print(f'{case.name}: reference == oracle == restatement, {n_poses} poses, coverage {cnt}')
    stats = oracle.group_stats()
    assert all(v > 0 for v in stats.values()), stats
    print('oracle coverage over the set:', stats)
    path = os.path.join(G.GOLD, 'grouping_edges.npz')
    save_npz(path, out)
    print(f'{path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
