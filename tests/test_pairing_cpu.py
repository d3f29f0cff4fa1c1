"""The directed pairing cases (tests/pairing_cases.py) on the CPU: the inputs regenerate to the stored hashes, the C oracle and
oracle/restatement.py reproduce the reference's lists and limbs (tests/golden/pairing_edges.npz, tools/gen_golden_pairing.py), and
every condition a case is built for occurs in them.  The cases past the stored ones (pairing_cases.DIGEST) are held to the SHA-256
of the reference's lists and EXACT_LIMB_COLS; the route og_generate_limbs_f32 takes with a shape (pairing_cases.plan) is held to the
library's own workspace size on both sides of the collect fallback."""
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
DIGESTS = dict(line.decode().split(' ', 1) for line in np.load(os.path.join(GOLDEN, 'pairing_edges.npz'))['digests'])


def test_fixture_lists_every_case_and_stays_small():
    g = np.load(os.path.join(GOLDEN, 'pairing_edges.npz'))
    assert list(g['names']) == NAMES
    size = os.path.getsize(os.path.join(GOLDEN, 'pairing_edges.npz'))
    assert size < max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f != 'pairing_edges.npz')
    ks = lambda heads, nd=2: {c.K for c in pc.CASES if c.heads == heads and c.nd == nd}  # noqa: E731
    assert ks('none') >= {1, 3, 7, 31, 32, 33, 63, 64, 65, 100} and ks('none', 4) >= {32, 48, 65}
    assert ks('scale') >= {7, 32, 33, 65} and ks('jitter') >= {7, 32, 33, 65}
    assert any(len(pc.skeleton(c)) == 44 for c in pc.CASES)
    assert ks('scale', 4) >= {32, 65} and ks('both') >= {7, 33, 65}
    assert {c.K for c in pc.CASES if c.skeleton == 'omp44'} >= {7, 33, 65, 100}
    assert {c.K for c in pc.CASES if c.name.startswith('fallback')} == {pc.IN_LAUNCH_K, pc.FALLBACK_K, pc.LARGEST_K}
    assert len(pc.STORED) == 22 and len(pc.DIGEST) == 11 and len(pc.CASES) == 33
    readme = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, 'README.md')).read()
    assert f'held on {len(pc.CASES)} directed cases' in readme, "README.md states another number of pairing cases"
    d = dict(line.decode().split(' ', 1) for line in g['digests'])
    for c in pc.DIGEST:     # nothing but digests and counts is stored of them (columns 11 / 12 of the SCALES_STORED ones besides)
        own = [k for k in g.files if k.startswith(c.name + '/')]
        assert own == ([f'{c.name}/scales_bicubic', f'{c.name}/scales_bilinear'] if c.name in pc.SCALES_STORED else [])
        keys = ['limbs_sha'] if pc.modes(c) == ('none',) else [f'limbs_{m}_sha' for m in pc.modes(c)]
        assert all(len(d[f'{c.name}/{k}']) == 64 for k in keys) and len(d[f'{c.name}/lists_sha']) == 128
        cnt = dict(kv.split('=') for kv in d[f'{c.name}/counts'].split(','))
        assert sorted(cnt) == sorted(pc.conditions(c)) and all(int(v) >= 1 for v in cnt.values())


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_the_reference(name):
    case, scene, exp = pc.load(name)                       # (asserts the input hashes)
    sk, K, hw = pc.skeleton(case), case.K, (case.H, case.W)
    sc, idx, _, _ = oracle.nms_topk(scene['hm_hr'], K)
    assert (sc == exp['scores']).all() and (idx == exp['inds']).all() and (sc > 0).all()
    off_hr = oracle.bilinear4(scene['off_lr'])
    jit_hr = oracle.bilinear4(scene['jit_lr']) if scene['jit_lr'] is not None else None
    for mode in pc.modes(case):
        ref = exp['limbs' if mode == 'none' else f'limbs_{mode}']
        scl_hr = None if mode == 'none' else (oracle.bicubic4 if mode == 'bicubic' else oracle.bilinear4)(scene['scl_lr'])
        for lowres in (True, False):
            got = oracle.collect_limbs(sc, idx, scene['off_lr'] if lowres else off_hr, lowres, hw, sk, pc.THRE, pc.MIN_LEN,
                                       vector_nd=case.nd, scales_hr=scl_hr, jitter_hr=jit_hr)
            assert_limbs_match(ref, got, SCORE_TOL)
            if case in pc.DIGEST:        # `ref` is the oracle's own stride-4 run: what holds it is the reference's digest
                assert pc.exact_digest(got) == DIGESTS[f"{name}/{'limbs' if mode == 'none' else 'limbs_' + mode}_sha"]
    ref = exp['limbs' if pc.modes(case) == ('none',) else 'limbs_bicubic']
    cnt = pc.counts(case, exp['scores'], exp['inds'], ref, off_hr, jit_hr, None if scene['scl_lr'] is None else oracle.bicubic4(scene['scl_lr']))
    assert cnt and all(v >= 1 for v in cnt.values()), cnt
    if case in pc.DIGEST:
        assert pc.lists_digest(sc, idx) == DIGESTS[f'{name}/lists_sha']
        assert ','.join(f'{k}={v}' for k, v in sorted(cnt.items())) == DIGESTS[f'{name}/counts']      # the reference's own counts


@pytest.mark.parametrize("name", [c.name for c in pc.CASES if c.heads == 'none' and c.nd == 2])
def test_restatement_reproduces_the_reference(name):
    case, scene, exp = pc.load(name)
    off_hr = torch.from_numpy(oracle.bilinear4(scene['off_lr']))
    got = restatement.generate_limbs(torch.from_numpy(scene['hm_hr']), off_hr, pc.skeleton(case), case.K, pc.THRE, pc.MIN_LEN).numpy()
    assert_limbs_match(exp['limbs'], got, SCORE_TOL)
    if case in pc.DIGEST:
        assert pc.exact_digest(got) == DIGESTS[f'{name}/limbs_sha']


def test_plan_restates_the_fallback_switch():
    """pairing_cases.plan against the library on both sides of the switch: og_generate_limbs_workspace_bytes is the one number of the
    plan the host can ask for without a device; the route itself is asserted on the device (tests/test_gpu_pairing.py: the lists of a
    fallback launch lie in the workspace).  A moved LDS limit, band height or panel width changes the cases' K here, not silently.
    The switch is that of (H, W, k) under pairing_cases.smallest_plane, not of k alone.  Needs the built library (no device): without
    libog_decoder.so _lib.load raises ImportError, as for every test that goes through the C ABI."""
    from offsetguided_amd import _lib
    lib = _lib.load()
    n = pc.N_IMAGES
    for k, route in ((pc.IN_LAUNCH_K, 'in_launch'), (pc.FALLBACK_K, 'fallback'), (pc.LARGEST_K, 'fallback'), (pc.LARGEST_K + 1, 'merge_refused')):
        h, w = pc.smallest_plane(k)
        assert 2 * (h + w) - 4 >= k > 2 * (h + w - 4) - 4 and h % 4 == 0 and w % 4 == 0      # admits k; four less on H + W does not
        p = pc.plan(n, 17, h, w, k)
        assert p.route == route, (k, p)
        assert p.workspace == lib.og_generate_limbs_workspace_bytes(n, 17, h, w, k) > 0
    assert pc.plan(n, 17, *pc.smallest_plane(pc.IN_LAUNCH_K), pc.IN_LAUNCH_K).lds <= pc.LDS_LIMIT < pc.plan(n, 17, *pc.smallest_plane(pc.FALLBACK_K), pc.FALLBACK_K).lds
    for k in range(8, pc.FALLBACK_K):        # FALLBACK_K is the SMALLEST k that leaves the merge-and-pair launch on its smallest plane
        assert pc.plan(n, 17, *pc.smallest_plane(k), k).route == 'in_launch', k
    for c in pc.CASES:                       # every other directed case pairs in the launch
        assert (pc.plan(n, 17, c.H, c.W, c.K).route == 'fallback') == (c.name in ('fallback_k645', 'fallback_k1020')), c.name
        assert pc.plan(n, 17, c.H, c.W, c.K).workspace == lib.og_generate_limbs_workspace_bytes(n, 17, c.H, c.W, c.K)
    # no plane takes a k past 1888 (make_plan), so can_pair's `k <= 2048` is never the deciding half; a second wave panel stops at 928
    for h, w, k, ok in ((700, 248, 1888, True), (704, 248, 1889, False), (516, 516, 2049, False), (216, 252, 928, True), (216, 252, 929, False)):
        p = pc.plan(n, 17, h, w, k)
        assert (p.route is not None) == ok and p.workspace == lib.og_generate_limbs_workspace_bytes(n, 17, h, w, k), (h, w, k)


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
