"""The directed grouping cases (tests/grouping_cases.py) on the CPU: the planted limbs rebuild to the stored hashes, the C oracle and
the traced restatement (oracle/restatement.py) reproduce the reference's poses (tests/golden/grouping_edges.npz,
tools/gen_golden_grouping.py) bit for bit, every condition a case is built for occurs in the trace, and `plan` -- the host restatement
of og_greedy_group_f32's placement of the table and the staged rows -- agrees with the library and with INTEGRATION.md."""
import os

import numpy as np
import pytest

import grouping_cases as gc
import oracle
from helpers import GOLDEN, sha
from offsetguided_amd import _lib
from offsetguided_amd.config import coco_data as cd

NAMES = [c.name for c in gc.CASES]


def test_fixture_lists_every_case_and_stays_small():
    path = os.path.join(GOLDEN, 'grouping_edges.npz')
    assert list(np.load(path)['names']) == NAMES
    assert os.path.getsize(path) < 128 * 1024
    groups = {c.group for c in gc.CASES}
    assert groups == {'rank', 'validity', 'seams', 'configs', 'overflow', 'delete_sort', 'n_kp'}
    assert {c.cfg for c in gc.CASES if c.group == 'configs'} == set('dgsl')
    assert gc.CFGS['d'] == (0.04, 40.0, 0, 2) and gc.CFGS['g'] == (0.02, 25.0, 1, 4)      # grouping_adversarial.npz's cfg_table
    table = np.load(os.path.join(GOLDEN, 'grouping_adversarial.npz'))['cfg_table']
    assert [tuple(r) for r in table] == [gc.CFGS['d'], gc.CFGS['g']]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_and_restatement_reproduce_the_reference(name):
    case, limbs, exp = gc.load(name)                       # (asserts the input hash)
    (sk, n_kp), cfg = gc.skeleton(case), gc.CFGS[case.cfg]
    traces = []
    for i, img in enumerate(limbs):
        got = oracle.greedy_group(img, sk, n_kp, cfg[0], cfg[1], bool(cfg[2]), int(cfg[3]))
        restated, tr = gc.trace(img, sk, n_kp, cfg)
        traces.append(tr)
        for tag, p in (('oracle', got), ('restatement', restated)):
            assert p.dtype == np.float32 and len(p) == exp['n_poses'][i] and sha(p) == exp['poses_sha'][i], (tag, i)
            if exp['poses'][i] is not None:
                assert p.shape == exp['poses'][i].shape and (p == exp['poses'][i]).all(), (tag, i, gc.first_difference(exp['poses'][i], p, tr))
    cnt = gc.counts(case, traces)
    assert cnt and all(v >= 1 for v in cnt.values()), cnt


def test_plan_labels_every_variant_and_rank_body():
    """The table of the issue, through `plan` on the launch whose result is returned (a label that does not hold is an error)."""
    want = {'rank_k32': ('lds', 'k32'), 'rank_k32_m127': ('lds', 'scalar'), 'rank_k12': ('lds', 'wide'), 'rank_k48': ('lds', 'wide'),
            'rank_k7': ('lds', 'scalar'), 'rank_k33': ('lds', 'scalar'), 'seams_k72': ('lds', 'wide'), 'seams_k128': ('gsub', 'wide'),
            'ovf_batch_k32': ('gsub', 'k32'), 'ovf_batch_k45': ('gsub', 'scalar'), 'ds_ties65_d': ('lds', 'k32'), 'ds_ties257_d': ('gsub', 'k32')}
    for cfg in 'dgsl':
        want.update({f'cfg_{cfg}_k32': ('lds', 'k32'), f'cfg_{cfg}_k48': ('gsub', 'wide'), f'cfg_{cfg}_k64': ('glim', 'wide')})
    for name, (variant, body) in want.items():
        case = gc.BY_NAME[name]
        (sk, n_kp), limbs = gc.skeleton(case), gc.build(case)
        traces = [gc.trace(img, sk, n_kp, gc.CFGS[case.cfg])[1] for img in limbs]
        pl = gc.plan(len(sk), case.K, n_kp, gc.launch_mmax(case, traces), len(limbs))
        assert (pl.variant, pl.body) == (variant, body), (name, pl)
    assert gc.launch_mmax(gc.BY_NAME['seams_k72'], [[{'P': 98}, None]]) == gc.MMAX
    assert gc.batch_mmax(19, 45, [600]) == 855 and gc.batch_mmax(19, 32, [129]) == 512 and gc.batch_mmax(19, 32, [128]) == 128


def test_plan_agrees_with_the_library_and_the_documented_capacity():
    lib = _lib.load()                                      # host entry point: needs no device
    shapes = [(n, len(sk), k, n_kp, mmax) for n in (1, 3, 8) for sk, n_kp in gc.SKELETONS.values() for k in (7, 32, 45, 72, 128)
              for mmax in (6, 127, 128, 512, 855)]
    for n, L, k, n_kp, mmax in shapes:
        assert gc.plan(L, k, n_kp, mmax, n).workspace_bytes == lib.og_group_workspace_bytes(n, L, k, n_kp, mmax), (n, L, k, n_kp, mmax)
    # what must stay in LDS is 16 B per candidate + 108 B per table row (+ the fixed parts: per-limb-type and
    # per-column counters, the scoring scratch, 64 B of slack, at most 12 B of rounding per wide array)
    for L, k, mmax in ((44, 64, 128), (44, 128, 128), (31, 128, 128), (19, 128, 512), (16, 200, 128)):
        pl = gc.plan(L, k, 17, mmax)
        fixed = (L + 5 * k + gc.K_SCORE_THREADS * 17) * 4 + 64
        assert pl.variant == 'glim' and 0 <= pl.lds_bytes - (16 * L * k + 108 * mmax + fixed) <= 36, (L, k, mmax, pl)
    assert gc.plan(len(cd.DENSER_COCO_PERSON_SKELETON), 256, 17, 128).variant is None       # the K = 256 DENSER refusal
    for sk in (cd.COCO_PERSON_SKELETON, cd.COCO_PERSON_WITH_REDUNDANT_SKELETON, cd.DENSER_COCO_PERSON_SKELETON, cd.KINEMATIC_TREE_SKELETON):
        assert all(gc.plan(len(sk), k, 17, 128).variant for k in (1, 32, 48, 64, 128))       # any skeleton at k <= 128
