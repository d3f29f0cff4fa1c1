"""K3 (og_greedy_group_f32, csrc/group.hip, behind decoder/group.py) on the directed cases of tests/grouping_cases.py against the
reference's stored output (tests/golden/grouping_edges.npz) and the oracle, bit for bit: shape and == on every element, status and
counts exact.  Cases of equal shape, configuration and final table size go through GreedyGroup.group_batch as ONE batch in shuffled
order (neighbours differ); the overflow cases with a table size of their own through group_device; the batch cases of the overflow
group as they are (only the middle image overflows).  A mismatch names the case, the first differing (row, keypoint, field) and the
limb types at which the trace shows that table row created and touched."""
import functools

import numpy as np
import pytest
import torch

import grouping_cases as gc
import oracle
from helpers import sha
from offsetguided_amd import _lib, decoder, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> case, limbs, per image (poses, trace): the stored reference poses (their sha256 where only that is stored) == the oracle
    here; every condition the case is built for occurs."""
    case, limbs, exp = gc.load(name)
    (sk, n_kp), cfg = gc.skeleton(case), gc.CFGS[case.cfg]
    out = []
    for i, img in enumerate(limbs):
        ref = oracle.greedy_group(img, sk, n_kp, cfg[0], cfg[1], bool(cfg[2]), int(cfg[3]))
        assert len(ref) == exp['n_poses'][i] and sha(ref) == exp['poses_sha'][i], f'{name}/{i}: oracle != stored reference'
        if exp['poses'][i] is not None:
            assert (ref == exp['poses'][i]).all()
        out.append((ref, gc.trace(img, sk, n_kp, cfg)[1]))
    cnt = gc.counts(case, [t for _, t in out])
    assert cnt and all(v >= 1 for v in cnt.values()), (name, cnt)
    return case, limbs, out


def grouper(case):
    (sk, n_kp), cfg = gc.skeleton(case), gc.CFGS[case.cfg]
    return decoder.GreedyGroup(cfg[0], sort_dim=int(cfg[3]), dist_max=cfg[1], use_scale=bool(cfg[2]),
                               keypoints=[f'kp{j}' for j in range(n_kp)], skeleton=sk)


def check(name, i, got, ref, tr):
    assert got.dtype == np.float32 and got.shape == ref.shape and (got == ref).all(), f'{name}/{i}: {gc.first_difference(ref, got, tr)}'


def run_batch(names, dev, seed=0):
    """The images of `names` (equal shape and configuration) as one batch in shuffled order -> checked against `expected`"""
    items = [(n, i, img, *expected(n)[2][i]) for n in names for i, img in enumerate(expected(n)[1])]
    if seed:
        items = [items[j] for j in np.argsort(synth.HashRng(seed).uniform(len(items)), kind='stable')]
    got = grouper(gc.BY_NAME[names[0]]).group_batch(torch.from_numpy(np.stack([it[2] for it in items])).to(dev))
    assert len(got) == len(items)
    for (n, i, _, ref, tr), p in zip(items, got):
        check(n, i, p, ref, tr)


SHAPES = sorted({(c.sk, c.K, c.cfg) for c in gc.CASES if c.via == 'batch' and len(gc.build(c)) == 1})


@pytest.mark.parametrize("sk,K,cfg", SHAPES)
def test_cases_of_one_shape_as_a_shuffled_batch(dev, sk, K, cfg):
    names = [c.name for c in gc.CASES if (c.sk, c.K, c.cfg, c.via) == (sk, K, cfg, 'batch') and len(gc.build(c)) == 1]
    by_mmax = {}
    for n in names:                                        # an image that overflows would move its neighbours' tables too
        case, _, out = expected(n)
        by_mmax.setdefault(gc.launch_mmax(case, [t for _, t in out]), []).append(n)
    for mmax, group in sorted(by_mmax.items()):
        run_batch(group, dev, seed=1000 + K + mmax)


@pytest.mark.parametrize("name", [c.name for c in gc.CASES if c.via == 'batch' and c.group == 'overflow'])
def test_only_the_middle_image_overflows(dev, name):
    run_batch([name], dev)


@pytest.mark.parametrize("name", [c.name for c in gc.CASES if c.via == 'device'])
def test_group_device_at_a_given_table_size(dev, name):
    case, limbs, out = expected(name)
    (ref, tr), = out
    poses, meta = grouper(case).group_device(torch.from_numpy(limbs.copy()).to(dev), case.mmax)
    count, status = (int(v) for v in meta.cpu().numpy())
    assert poses.shape == (1, case.mmax, gc.skeleton(case)[1], 6)
    if tr[-2]['P'] > case.mmax:                            # rows ever created, not live ones
        assert (status, count) == (1, 0), (name, status, count)
    else:
        assert (status, count) == (0, len(ref)), (name, status, count)
        check(name, 0, poses[0, :count].cpu().numpy(), ref, tr)


def test_stale_workspace(dev):
    """The tables and staged rows in the caller's workspace are never cleared: K3 on a workspace full of NaN, then on what larger and
    differently shaped launches left there, then a small K = 32 launch (table in the workspace after its retry) on the same bytes."""
    lib = _lib.load()
    sizes = []
    for name in ('seams_k128', 'cfg_d_k64', 'ds_ties257_d'):
        case = gc.BY_NAME[name]
        sk, n_kp = gc.skeleton(case)
        assert gc.plan(len(sk), case.K, n_kp, 512 if name == 'ds_ties257_d' else gc.MMAX).variant != 'lds'
        sizes.append(lib.og_group_workspace_bytes(4, len(sk), case.K, n_kp, 512))
    ws = _lib.workspace(dev, max(sizes), 'group')          # the buffer every launch below gets
    ws.view(torch.float32).fill_(float('nan'))
    for names in (['seams_k128'], ['cfg_d_k64'], ['seams_k128'] * 3, ['cfg_l_k64'], ['seams_k128'], ['ds_ties257_d'], ['cfg_g_k64']):
        run_batch(names, dev)
        assert _lib.workspace(dev, 1, 'group').data_ptr() == ws.data_ptr()
