"""The directed pairing cases (tests/pairing_cases.py) on the CPU: the inputs regenerate to the stored hashes, the C oracle and
oracle/restatement.py reproduce the reference's lists and limbs (tests/golden/pairing_edges.npz, tools/gen_golden_pairing.py), and
every condition a case is built for occurs in them."""
import os

import numpy as np
import pytest
import torch

import oracle
import pairing_cases as pc
from helpers import GOLDEN, assert_limbs_match
from oracle import restatement

SCORE_TOL = 1e-4
NAMES = [c.name for c in pc.CASES]


def test_fixture_lists_every_case_and_stays_small():
    g = np.load(os.path.join(GOLDEN, 'pairing_edges.npz'))
    assert list(g['names']) == NAMES
    size = os.path.getsize(os.path.join(GOLDEN, 'pairing_edges.npz'))
    assert size < max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f != 'pairing_edges.npz')
    ks = lambda heads, nd=2: {c.K for c in pc.CASES if c.heads == heads and c.nd == nd}  # noqa: E731
    assert ks('none') >= {1, 3, 7, 31, 32, 33, 63, 64, 65, 100} and ks('none', 4) >= {32, 48, 65}
    assert ks('scale') >= {7, 32, 33, 65} and ks('jitter') >= {7, 32, 33, 65}
    assert any(len(pc.skeleton(c)) == 44 for c in pc.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_the_reference(name):
    case, scene, exp = pc.load(name)                       # (asserts the input hashes)
    sk, K, hw = pc.skeleton(case), case.K, (case.H, case.W)
    sc, idx, _, _ = oracle.nms_topk(scene['hm_hr'], K)
    assert (sc == exp['scores']).all() and (idx == exp['inds']).all() and (sc > 0).all()
    off_hr = oracle.bilinear4(scene['off_lr'])
    jit_hr = oracle.bilinear4(scene['jit_lr']) if scene['jit_lr'] is not None else None
    for mode in (('bicubic', 'bilinear') if case.heads == 'scale' else ('none',)):
        ref = exp['limbs' if mode == 'none' else f'limbs_{mode}']
        scl_hr = None if mode == 'none' else (oracle.bicubic4 if mode == 'bicubic' else oracle.bilinear4)(scene['scl_lr'])
        for lowres in (True, False):
            got = oracle.collect_limbs(sc, idx, scene['off_lr'] if lowres else off_hr, lowres, hw, sk, pc.THRE, pc.MIN_LEN,
                                       vector_nd=case.nd, scales_hr=scl_hr, jitter_hr=jit_hr)
            assert_limbs_match(ref, got, SCORE_TOL)
    ref = exp['limbs' if case.heads != 'scale' else 'limbs_bicubic']
    cnt = pc.counts(case, exp['scores'], exp['inds'], ref, off_hr, jit_hr)
    assert cnt and all(v >= 1 for v in cnt.values()), cnt


@pytest.mark.parametrize("name", [c.name for c in pc.CASES if c.heads == 'none' and c.nd == 2])
def test_restatement_reproduces_the_reference(name):
    case, scene, exp = pc.load(name)
    off_hr = torch.from_numpy(oracle.bilinear4(scene['off_lr']))
    got = restatement.generate_limbs(torch.from_numpy(scene['hm_hr']), off_hr, pc.skeleton(case), case.K, pc.THRE, pc.MIN_LEN).numpy()
    assert_limbs_match(exp['limbs'], got, SCORE_TOL)


@pytest.mark.parametrize("K", pc.FUSED_K)
def test_fused_scenes_have_enough_valid_rows(K):
    """The scenes of the forms that start from stride-4 heat maps: at least a quarter of the oracle's rows have both ends above the
    threshold (the rows tests/test_gpu_pairing.py compares), and peaks sit on the border of the upsampled plane."""
    hm, off, _, _ = pc.build_fused(K)
    hr = oracle.bicubic4(hm[:pc.N_IMAGES])
    sc, idx, ys, xs = oracle.nms_topk(hr, K)
    limbs = oracle.collect_limbs(sc, idx, off[:pc.N_IMAGES], True, hr.shape[2:], pc.SKELETONS['omp19'], pc.THRE, pc.MIN_LEN)
    valid = (limbs[..., 2] >= pc.THRE) & (limbs[..., 5] >= pc.THRE)
    assert valid.mean() >= 0.25
    ok = sc >= pc.THRE
    assert (ok & ((ys == 0) | (ys == 63) | (xs == 0) | (xs == 63))).any()
