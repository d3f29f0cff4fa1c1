"""Directed cases for the greedy grouping (K3: og_greedy_group_f32, csrc/group.hip, behind decoder/group.py) -- shared by
tools/gen_golden_grouping.py, tests/test_grouping_cpu.py and tests/test_gpu_grouping.py.  No GPU code, no reference import.

A case PLANTS its limbs straight into (L, K, 13) float32 arrays (columns as in decoder/group.py: x1 y1 v1 x2 y2 v2 ind1 ind2 len_delta
len_limb limb_score scale1 scale2).  A person is a dict keypoint -> (x, y, v, global index) with integer coordinates; limb scores and
keypoint scores sit on a dyadic grid (multiples of 1/256 and 1/128), so planned ties are exact and sums of them carry no rounding
-- except where a case is about fp32 rounding itself (the threshold rows and the np_sum17 rows of the delete_sort group).  A case
says which limb types every person contributes and towards whose keypoint:

  * a limb type whose two keypoints are both new to a person starts a second row for that person; the later limb type that joins the
    two rows is a MERGE (phase C);
  * two persons that share a peak (same global index) give phase A / phase B on several rows, duplicate partners, cross3;
  * the rows without a planted limb are fillers moved off the image (x < 0), like the production's sub-threshold candidates.

`plan` restates, on the host, staging_bytes and the GSUB / GLIM choice of og_greedy_group_f32 and which body of rank_pass / urank_pass
runs.  `trace` is oracle/restatement.py:group_skeletons with its per-limb-type record.  Each case names the conditions it is built for
(`conditions`); `count` counts their occurrences FROM THE TRACE and the planted values (never from the builder's intent), and the
generator, the CPU test and the GPU test all assert every count >= 1.

A row without a positive entry in the sort column scores NaN; where the reference puts it is an artefact of Python's sort, outside the
contract: no case holds one, and `count` asserts that ('no_nan_score', part of every case)."""
from collections import namedtuple

import numpy as np

from offsetguided_amd import synth
from offsetguided_amd.config import coco_data as cd

HW = 4096                                    # global index = keypoint * HW + peak: exact in fp32
MMAX = 128                                   # GreedyGroup.MMAX
TIE_ROWS = 16                                # equal limb scores only among <= 16 valid rows of a limb type: the reference sorts with
#                                              np.argsort's default kind, which is an insertion sort (stable) up to 16 elements and
#                                              whatever the platform's quicksort gives beyond -- ties there are outside the contract
F32_THRE = float(np.float32(0.04))           # 0.03999999910593033 < 0.04
# (person_thre, dist_max, use_scale, sort_dim): the two rows of grouping_adversarial.npz's cfg_table and two more
CFGS = {'d': (0.04, 40.0, 0, 2), 'g': (0.02, 25.0, 1, 4), 's': (0.04, 40.0, 1, 2), 'l': (0.02, 25.0, 0, 4), 'f': (F32_THRE, 40.0, 0, 2)}

# 16 limb types over 17 keypoints with ONE cycle (1-3-5-6-4-2-0): (5, 6) starts a second row, (4, 6) or (3, 5) merges it.  At 16 limb
# types K = 72 leaves the table in LDS and K = 128 moves only the table out (19 limb types would not: see `plan`)
SEAM16 = [c for c in cd.COCO_PERSON_SKELETON if c not in ((1, 2), (11, 12), (14, 16))]
CHAIN5 = [(0, 1), (2, 3), (1, 2), (3, 4), (0, 2)]                              # a chain, (2, 3) before (1, 2): a merge; (0, 2) redundant
CHAIN16 = [(0, 1), (2, 3), (1, 2)] + [(j, j + 1) for j in range(3, 15)] + [(0, 2)]
SKELETONS = {'omp19': (cd.COCO_PERSON_SKELETON, 17), 'omp44': (cd.DENSER_COCO_PERSON_SKELETON, 17), 'seam16': (SEAM16, 17),
             'chain5': (CHAIN5, 5), 'chain16': (CHAIN16, 16)}

# via: 'batch' = GreedyGroup.group_batch (retries on overflow), 'device' = GreedyGroup.group_device(limbs, mmax) once
Case = namedtuple('Case', 'name group sk K cfg via mmax build args conds')
Plan = namedtuple('Plan', 'variant lds_bytes body workspace_bytes')


# ---------------------------------------------------------------------------------- the launch, restated
K_SCORE_THREADS, ID_PITCH, LDS_LIMIT = 256, 20, 159 * 1024


def staging_bytes(L, K, mmax, glim):
    lk = L * K
    lk4 = (lk + 3) & ~3
    words = (0 if glim else ((lk * 11 + 3) & ~3)) + 3 * lk4 + lk + L + 5 * K + 5 * mmax + K_SCORE_THREADS * 17
    return mmax * ID_PITCH * 4 + mmax * 8 + words * 4 + 64


def plan(L, K, n_kp, mmax, N=1):
    """What og_greedy_group_f32 does with this shape: variant 'lds' (all in LDS) / 'gsub' (table in the workspace) / 'glim' (table and
    staged rows in the workspace) / None (refused), the dynamic LDS bytes, the body of the rank passes, og_group_workspace_bytes."""
    table = mmax * n_kp * 6 * 4
    variant, lds = 'lds', staging_bytes(L, K, mmax, False) + table
    if lds > LDS_LIMIT:
        variant, lds = 'gsub', lds - table
    if lds > LDS_LIMIT:
        variant, lds = 'glim', staging_bytes(L, K, mmax, True)
    if lds > LDS_LIMIT:
        variant = None
    wide = K % 4 == 0 and mmax % 2 == 0
    up = lambda v: (v + 255) // 256 * 256  # noqa: E731
    return Plan(variant, lds, 'k32' if K == 32 and wide else 'wide' if wide else 'scalar', up(N * table) + up(N * L * K * 11 * 4))


def batch_mmax(L, K, created):
    """The table size of group_batch's last launch for images that create `created` rows each."""
    mmax = MMAX
    while max(created) > mmax and mmax < L * K:
        mmax = min(mmax * 4, L * K)
    return mmax


# ---------------------------------------------------------------------------------- builder
def person(p, n_kp=17, v=None):
    """keypoint -> (x, y, v, global index): integer coordinates > 0, v on the 1/128 grid unless given"""
    return {j: (float(3 + 5 * p + j), float(2 + 3 * j + p % 7), (24 + (37 * p + 11 * j) % 97) / 128.0 if v is None else v,
                float(j * HW + p)) for j in range(n_kp)}


class Scene:
    def __init__(self, sk, K, seed):
        self.sk, self.K, self.seed = sk, K, seed
        self.rows = [[] for _ in sk]

    def add(self, pair, src, dst, score, delta=3.0, s1=4.0, s2=4.0):
        (x1, y1, v1, i1), (x2, y2, v2, i2) = src[pair[0]], dst[pair[1]]
        self.rows[self.sk.index(pair)].append([x1, y1, v1, x2, y2, v2, i1, i2, delta, 10.0, score, s1, s2])

    def limbs(self):
        """The planted rows of a limb type keep their order, on pseudo-randomly chosen slots: fillers lie between them."""
        out = np.zeros((len(self.sk), self.K, 13), np.float32)
        for l, (a, b) in enumerate(self.sk):
            rows = self.rows[l]
            assert len(rows) <= self.K, (l, len(rows), self.K)
            for k in range(self.K):
                out[l, k] = [-99990.0, -99980.0, 1 / 1024, -99970.0, -99960.0, 1 / 512, a * HW + 3000 + k, b * HW + 3000 + k, 5.0, 10.0,
                             (k + 1) / 65536.0, 4.0, 4.0]
            perm = np.argsort(synth.HashRng(self.seed + l).uniform(self.K), kind='stable')
            for k, r in zip(sorted(perm[:len(rows)].tolist()), rows):
                out[l, k] = r
        return out


def _grid(seed, n, lo, hi, den):
    return synth.HashRng(seed).integers(n, lo, hi).astype(np.float64) / den


def rank_scene(K):
    """omp19, every keypoint score 1/2 (all person scores tie: the output order IS the table order, so the order of the columns shows)"""
    sc = Scene(cd.COCO_PERSON_SKELETON, K, 100 + K)
    P = [person(p, v=0.5) for p in range(K)]
    order = np.argsort(synth.HashRng(7 + K).uniform(K), kind='stable')
    for p in range(K):                                         # (1, 2): all K rows valid, distinct scores and to-indices -> kk = K
        sc.add((1, 2), P[p], P[p], (32 + 3 * int(order[p])) / 256)
    for p, s in enumerate([0.5, 0.25, 0.5, 0.25, 0.5]):        # (1, 3): three and two equal scores at distinct to-indices
        sc.add((1, 3), P[p], P[p], s)
    for p in range(5, min(K - 2, TIE_ROWS)):                  # (the rest distinct, interleaved with fillers)
        sc.add((1, 3), P[p], P[p], (8 + 4 * int(order[p])) / 256)
    sc.add((2, 4), P[0], P[0], 0.375)                          # (2, 4): equal scores sharing a to-index: the earlier row survives
    sc.add((2, 4), P[1], P[0], 0.375)
    sc.add((2, 4), P[2], P[2], 0.125)                          #         a better score later in the list owns the to-index
    sc.add((2, 4), P[3], P[2], 0.75)
    for p in range(4, min(K - 2, TIE_ROWS)):
        sc.add((2, 4), P[p], P[p], (9 + 4 * int(order[p])) / 256)
    for i, pair in enumerate([(4, 6), (3, 5), (5, 7)]):        # (5, 6) stays empty between (2, 4) and (4, 6); (0, 1), (0, 2) lead empty
        for p in range(K - 1):
            sc.add(pair, P[p], P[p], (8 + 4 * int(order[(p + 5 * i + 1) % K])) / 256)
    return [sc.limbs()]


def validity_scene(K, dist):
    d, below = np.float32(dist), np.nextafter(np.float32(dist), np.float32(0))
    sc = Scene(cd.COCO_PERSON_SKELETON, K, 200 + int(dist))
    P = [person(p) for p in range(16)]
    g = _grid(17 + int(dist), 64, 16, 240, 256)
    sc.add((0, 1), P[0], P[0], g[0], delta=d)                  # len_delta == dist_max: out
    sc.add((0, 1), P[1], P[1], g[1], delta=below)              # one fp32 step below: in
    for i, (kp, f) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):       # x1, y1, x2, y2 exactly 0: out
        q = dict(P[2 + i])
        t = list(q[kp])
        t[f] = 0.0
        q[kp] = tuple(t)
        sc.add((0, 1), q, q, g[2 + i])
    # scale2 above / equal to / below dist_max, len_delta between the two limits and on them
    for i, (s2, dl) in enumerate([(d + 5, d + 2), (d + 5, d + 5), (d, d), (d, below), (d - 5, d - 3), (d - 5, d), (d - 5, below)]):
        sc.add((0, 1), P[6 + i], P[6 + i], g[6 + i], delta=dl, s2=s2)
    sc.add((0, 1), P[13], P[13], g[13])
    for i, pair in enumerate([(0, 2), (1, 2), (1, 3), (2, 4)]):          # the persons whose (0, 1) is out start their row later
        for p in range(14):
            sc.add(pair, P[p], P[p], g[16 + 14 * (i % 3) + p])
    return [sc.limbs()]


SEAM_P, SEAM_X, SEAM_Y, SEAM_NOSE = 70, 10, 5, ((20, 21), (66, 67))


def seam_scene(K):
    """70 persons on SEAM16.  Most drop (5, 6) and stay one row.  The mergers (p % 5 == 2, p >= 62) keep it: a second row behind the 70
    heads, merged by (4, 6) -- a < 64 <= b, 64 <= a < b, b - a >= 16.  X: two (5, 6) limbs from one peak, no (4, 6): (3, 5) gives X's
    head two partners, which are partners of each other.  Y: a second (5, 7) limb from Y's peak with the lowest score of all: two
    matching columns in one row, one on each side of column 64.  The pairs of SEAM_NOSE share a nose and one (0, 2) limb: two heads
    merge, below and above row 64 in the same limb type.  A ghost with the lowest (0, 2) score starts a row from a column >= 64."""
    sc = Scene(SEAM16, K, 300 + K)
    P = [person(p) for p in range(SEAM_P)]
    for p, q in SEAM_NOSE:
        P[q][0] = P[p][0]
    ghost = [person(900 + i) for i in range(3)]
    g = np.stack([40 + 2 * np.argsort(synth.HashRng(19 + l).uniform(SEAM_P), kind='stable') for l in range(16)], 1) / 256   # distinct per limb type
    g[:, 0] = (240 - 2 * np.arange(SEAM_P)) / 256              # (0, 1): rank = person, so table row p is person p's head
    second = {q for _, q in SEAM_NOSE}
    for p in range(SEAM_P):
        merger = (p % 5 == 2 or p >= 62) and p not in (SEAM_X, SEAM_Y) and p not in second
        for l, pair in enumerate(SEAM16):
            if pair == (5, 6) and not (merger or p == SEAM_X):
                continue
            if (pair == (4, 6) and p == SEAM_X) or (pair == (0, 2) and p in second):
                continue
            sc.add(pair, P[p], P[p], g[p, l])
    sc.add((5, 6), P[SEAM_X], ghost[0], 113 / 256)
    sc.add((5, 7), P[SEAM_Y], ghost[1], 1 / 256)
    sc.add((0, 2), ghost[2], ghost[2], 1 / 256)
    return [sc.limbs()]


def collision_scene(sk, K, seed, n_persons=14, pool=5):
    """Collision-heavy: persons draw their peaks from a small pool per keypoint, limbs cross to other persons; scores, keypoint scores,
    len_delta and the scales on grids that straddle every threshold of the four configurations."""
    rng = synth.HashRng(seed)
    xy = rng.integers(17 * pool * 2, 1, 400).reshape(17, pool, 2)
    v = rng.integers(17 * pool, 3, 127).reshape(17, pool) / 128.0
    v[rng.uniform(17 * pool).reshape(17, pool) < 0.25] /= 8
    pid = rng.integers(n_persons * 17, 0, pool - 1).reshape(n_persons, 17)
    peak = lambda j, i: (float(xy[j, i, 0]), float(xy[j, i, 1]), float(v[j, i]), float(j * HW + i))  # noqa: E731
    sc = Scene(sk, K, seed)
    for l, (a, b) in enumerate(sk):
        order = np.argsort(rng.uniform(n_persons), kind='stable')
        take, cross, other = rng.uniform(n_persons) < 0.8, rng.uniform(n_persons) < 0.3, rng.integers(n_persons, 0, n_persons - 1)
        score = rng.integers(n_persons, 4, 255) / 256.0
        score[rng.uniform(n_persons) < 0.3] /= 8
        delta, s2 = rng.integers(n_persons, 0, 45), np.array([4.0, 30.0, 50.0])[rng.integers(n_persons, 0, 2)]
        for p in order[:K]:
            if take[p]:
                q = other[p] if cross[p] else p
                sc.add((a, b), {a: peak(a, pid[p, a])}, {b: peak(b, pid[q, b])}, float(score[p]), delta=float(delta[p]), s2=float(s2[p]))
    return sc.limbs()


def config_scene(sk_name, K):
    return [collision_scene(SKELETONS[sk_name][0], K, 400 + K)]


def isolated_scene(sk, K, n_types, seed, tie_types=()):
    """Every row of the first `n_types` limb types is a skeleton of its own (n_types * K rows ever created).  In the limb types of
    `tie_types` one row has keypoint scores 1/2, 1/2 and limb score 1/2: equal person scores under sort_dim 2 and 4.  Within a limb
    type the limb scores are distinct."""
    sc = Scene(sk, K, seed)
    for l in range(n_types):
        g = (16 + 5 * np.argsort(synth.HashRng(seed + 50 + l).uniform(K), kind='stable')) / 256
        for k in range(K):
            tie = l in tie_types and k == 3
            q = person(l * K + k, v=0.5 if tie else None)
            sc.add(sk[l], q, q, 0.5 if tie else float(g[k]))
    return sc.limbs()


def overflow_scene(K):
    """Persons 0-2: (5, 6) starts a second row, (4, 6) merges it (6 rows created, 3 live).  Persons 3-5 begin at (5, 7): 9 rows created,
    never more than 6 live."""
    sk = cd.COCO_PERSON_SKELETON
    sc = Scene(sk, K, 500)
    g = _grid(23, 6 * 19, 40, 240, 256).reshape(6, 19)
    for p in range(6):
        q = person(p)
        for l, pair in enumerate(sk):
            if p < 3 or pair in ((5, 7), (7, 9), (5, 11), (11, 13), (13, 15)):
                sc.add(pair, q, q, g[p, l])
    return [sc.limbs()]


def overflow_batch_scene(K, n_types):
    sk = cd.COCO_PERSON_SKELETON
    return [collision_scene(sk, K, 510 + K), isolated_scene(sk, K, n_types, 520 + K), collision_scene(sk, K, 530 + K)]


def threshold_scene(K):
    """(0, 1) rows of two keypoints with the same score t: the fp32 sum 2t and the mean t are exact.  t = float32(0.04) and its neighbours."""
    t = np.float32(0.04)
    sc = Scene(cd.COCO_PERSON_SKELETON, K, 600)
    for p, v in enumerate([0.5, t, np.nextafter(t, np.float32(1)), 0.25, np.nextafter(t, np.float32(0)), t, 0.75]):
        q = person(p, v=float(v))
        sc.add((0, 1), q, q, (200 - 8 * p) / 256)
    return [sc.limbs()]


NPOS = (1, 7, 8, 9, 16, 17)


def npos_scene(K):
    """Persons with 1, 7, 8, 9, 16 and 17 positive keypoint scores (every branch of np_sum17), two of each; the scores have full
    fp32 mantissas, so the order of the additions shows in the sum."""
    sk = cd.COCO_PERSON_SKELETON
    sc = Scene(sk, K, 610)
    u = synth.HashRng(611).uniform(12 * 17, 0.3, 0.9).astype(np.float32).reshape(12, 17)
    g = _grid(612, 12 * 19, 40, 240, 256).reshape(12, 19)
    for i in range(12):
        n, q = NPOS[i % 6], person(i)
        q = {j: (q[j][0], q[j][1], float(u[i, j]), q[j][3]) for j in q}
        if n == 1:
            q[1] = (q[1][0], q[1][1], 0.0, q[1][3])
            sc.add((0, 1), q, q, g[i, 0])
            continue
        for l, pair in enumerate(sk):
            if max(pair) < n:
                sc.add(pair, q, q, g[i, l])
    return [sc.limbs()]


def ties_scene(K, n_types):
    return [isolated_scene(cd.COCO_PERSON_SKELETON, K, n_types, 620 + n_types, tie_types=(0, n_types // 2, n_types - 1))]


def chain_scene(sk_name, K):
    sk, n_kp = SKELETONS[sk_name]
    sc = Scene(sk, K, 700 + n_kp)
    g = _grid(29 + n_kp, 6 * len(sk), 40, 240, 256).reshape(6, len(sk))
    for p in range(6):
        q = person(p, n_kp)
        for l, pair in enumerate(sk):
            if not (p == 4 and pair == (2, 3)) and not (p == 5 and pair == (0, 2)):
                sc.add(pair, q, q, g[p, l])
    return [sc.limbs()]


# ---------------------------------------------------------------------------------- the cases
RANK_CONDS = ['tie2', 'tie3', 'tie_same_to', 'later_owner', 'invalid_between', 'kk_eq_K', 'empty_between', 'leading_empty']
SEAM_CONDS = ['m0_gt64_kk_gt64', 'first_new_gt64', 'merge_a_lt64_le_b', 'merge_64_le_a', 'merge_far', 'two_partners', 'deleted_is_a',
              'deleted_both_sides', 'multi_b_across_64', 'new_col_ge64_live', 'phaseA']


def _cases():
    out = []
    for K, mmax, body in ((32, None, 'k32'), (32, 127, 'scalar'), (12, None, 'wide'), (48, None, 'wide'), (7, None, 'scalar'), (33, None, 'scalar')):
        out.append(Case(f'rank_k{K}' + (f'_m{mmax}' if mmax else ''), 'rank', 'omp19', K, 'd', 'device' if mmax else 'batch', mmax,
                        rank_scene, (K,), RANK_CONDS + ['body_' + body, 'variant_lds']))
    for cfg in 'dsg':
        scale = ['scale_above', 'scale_equal', 'scale_below'] if CFGS[cfg][2] else []
        out.append(Case(f'validity_{cfg}', 'validity', 'omp19', 32, cfg, 'batch', None, validity_scene, (32, CFGS[cfg][1]),
                        ['delta_eq_dist', 'delta_below_dist', 'x1_zero', 'y1_zero', 'x2_zero', 'y2_zero', 'body_k32'] + scale))
    out.append(Case('seams_k72', 'seams', 'seam16', 72, 'd', 'batch', None, seam_scene, (72,), SEAM_CONDS + ['variant_lds', 'body_wide']))
    out.append(Case('seams_k128', 'seams', 'seam16', 128, 'd', 'batch', None, seam_scene, (128,), SEAM_CONDS + ['variant_gsub', 'body_wide']))
    for sk, K, variant, body in (('omp19', 32, 'lds', 'k32'), ('omp44', 48, 'gsub', 'wide'), ('omp44', 64, 'glim', 'wide')):
        for cfg in 'dgsl':
            out.append(Case(f'cfg_{cfg}_k{K}', 'configs', sk, K, cfg, 'batch', None, config_scene, (sk, K),
                            ['variant_' + variant, 'body_' + body, 'cfg_distinct', 'phaseB', 'merge', 'multi_b']))
    out.append(Case('ovf_exact', 'overflow', 'omp19', 8, 'd', 'device', 9, overflow_scene, (8,), ['mmax_eq_created', 'status0']))
    out.append(Case('ovf_short', 'overflow', 'omp19', 8, 'd', 'device', 8, overflow_scene, (8,), ['mmax_eq_created_minus_1', 'status1']))
    out.append(Case('ovf_reclaim', 'overflow', 'omp19', 8, 'd', 'device', 6, overflow_scene, (8,), ['live_le_mmax_lt_created', 'status1']))
    out.append(Case('ovf_batch_k32', 'overflow', 'omp19', 32, 'd', 'batch', None, overflow_batch_scene, (32, 5),
                    ['only_middle_overflows', 'variant_gsub']))
    out.append(Case('ovf_batch_k45', 'overflow', 'omp19', 45, 'd', 'batch', None, overflow_batch_scene, (45, 13),
                    ['only_middle_overflows', 'created_gt_512', 'final_mmax_odd', 'body_scalar', 'variant_gsub']))
    thre = ['mean_eq_f32_thre', 'mean_step_above', 'mean_step_below']
    out.append(Case('ds_thre_py', 'delete_sort', 'omp19', 8, 'd', 'batch', None, threshold_scene, (8,), thre + ['eq_dropped']))
    out.append(Case('ds_thre_f32', 'delete_sort', 'omp19', 8, 'f', 'batch', None, threshold_scene, (8,), thre + ['eq_kept']))
    out.append(Case('ds_npos', 'delete_sort', 'omp19', 16, 'd', 'batch', None, npos_scene, (16,), [f'npos_{n}' for n in NPOS]))
    for cfg in 'dl':
        out.append(Case(f'ds_ties65_{cfg}', 'delete_sort', 'omp19', 32, cfg, 'batch', None, ties_scene, (32, 4),
                        ['rows_gt_64', 'tie3_span_gt_64', 'fits_exactly', 'variant_lds']))
        out.append(Case(f'ds_ties257_{cfg}', 'delete_sort', 'omp19', 32, cfg, 'batch', None, ties_scene, (32, 10),
                        ['rows_gt_256', 'tie3_span_gt_256', 'variant_gsub', 'body_k32']))
    for name in ('chain5', 'chain16'):
        out.append(Case('nkp_' + name, 'n_kp', name, 8, 'd', 'batch', None, chain_scene, (name, 8), ['merge', 'phaseA', 'nkp_lt_17']))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
_BUILT = {}


def build(case):
    """-> (N, L, K, 13) float32, N = 1 but for the batch cases of the overflow group (cached: treat as read-only)"""
    key = (case.build.__name__, case.args)
    if key not in _BUILT:
        _BUILT[key] = np.ascontiguousarray(np.stack(case.build(*case.args)), np.float32)
        _BUILT[key].setflags(write=False)
    return _BUILT[key]


def skeleton(case):
    return SKELETONS[case.sk]


def conditions(case):
    return list(case.conds) + ['no_nan_score', 'ties_in_contract']


def trace(limbs, sk, n_kp, cfg):
    """The traced restatement on one image -> (poses, records): see oracle/restatement.py:group_skeletons"""
    from oracle import restatement
    rec = []
    poses = restatement.group_skeletons(limbs, sk, n_kp, cfg[0], cfg[1], bool(cfg[2]), int(cfg[3]), trace=rec)
    return poses, rec


def launch_mmax(case, traces):
    """Table size of the launch whose result is returned"""
    sk, _ = skeleton(case)
    return case.mmax if case.via == 'device' else batch_mmax(len(sk), case.K, [t[-2]['P'] for t in traces])


# ---------------------------------------------------------------------------------- coverage
def _valid(limbs_l, cfg):
    lim = np.maximum(np.float32(cfg[1]), limbs_l[:, 12]) if cfg[2] else np.float32(cfg[1])
    return (limbs_l[:, 8] < lim) & (limbs_l[:, 0] > 0) & (limbs_l[:, 4] > 0) & (limbs_l[:, 3] > 0) & (limbs_l[:, 1] > 0)


def count(case, cond, traces):
    """Occurrences of `cond`: from the per-limb-type records of the traced restatement (`traces`: one list per image), the planted
    limbs and `plan`."""
    limbs, cfg, (sk, n_kp) = build(case), CFGS[case.cfg], skeleton(case)
    L, K = len(sk), case.K
    steps = [r for t in traces for r in t[:-1]]
    finals = [t[-1] for t in traces]
    mmax = launch_mmax(case, traces)
    pl = plan(L, K, n_kp, mmax, len(limbs))
    pairs = [(r, a, b) for r in steps for a, b in r['pairs']]
    if cond == 'no_nan_score':
        return int(all(not np.isnan(f['scores']).any() for f in finals))
    if cond == 'ties_in_contract':
        for img in limbs:
            for l in range(L):
                s = img[l, _valid(img[l], cfg), 10]
                if len(s) > TIE_ROWS and len(np.unique(s)) < len(s):
                    return 0
        return 1
    if cond.startswith('variant_'):
        return int(pl.variant == cond[8:])
    if cond.startswith('body_'):
        return int(pl.body == cond[5:])
    # ---- rank
    if cond in ('tie2', 'tie3', 'tie_same_to', 'later_owner', 'invalid_between'):
        n = 0
        for img in limbs:
            for l in range(L):
                ok = _valid(img[l], cfg)
                s, to = img[l, :, 10], img[l, :, 7].astype(np.int64)
                idx = np.nonzero(ok)[0]
                if cond == 'invalid_between':
                    n += int(len(idx) >= 2 and (~ok[idx[0]:idx[-1]]).any())
                for v in np.unique(s[ok]):
                    same = idx[s[idx] == v]
                    if cond == 'tie2':
                        n += int(len(same) == 2 and len(set(to[same])) == 2)
                    if cond == 'tie3':
                        n += int(len(same) >= 3 and len(set(to[same])) == len(same))
                    if cond == 'tie_same_to':
                        n += int(len(same) >= 2 and len(set(to[same])) < len(same))
                if cond == 'later_owner':
                    n += sum(int(to[i] == to[j] and s[j] > s[i]) for i in idx for j in idx if i < j)
        return n
    if cond == 'kk_eq_K':
        return sum(r['kk'] == K for r in steps)
    if cond == 'empty_between':
        kk = [r['kk'] for r in traces[0][:-1]]
        return sum(kk[l] == 0 and any(kk[:l]) and any(kk[l + 1:]) for l in range(L))
    if cond == 'leading_empty':
        kk = [r['kk'] for r in traces[0][:-1]]
        return int(kk[0] == 0 and kk[1] == 0 and any(kk))
    # ---- validity
    c8, c12, d = limbs[..., 8], limbs[..., 12], np.float32(cfg[1])
    real = limbs[..., 2] >= 1 / 128                        # not a filler
    if cond == 'delta_eq_dist':
        return int((real & (c8 == d) & (c12 <= d)).sum())
    if cond == 'delta_below_dist':
        return int((real & (c8 == np.nextafter(d, np.float32(0))) & (c12 <= d)).sum())
    if cond in ('x1_zero', 'y1_zero', 'x2_zero', 'y2_zero'):
        return int((real & (limbs[..., {'x1_zero': 0, 'y1_zero': 1, 'x2_zero': 3, 'y2_zero': 4}[cond]] == 0)).sum())
    if cond == 'scale_above':                              # admitted only because of the scale; refused on the scale's own limit
        return int(min((real & (c12 > d) & (c8 > d) & (c8 < c12)).sum(), (real & (c12 > d) & (c8 == c12)).sum()))
    if cond == 'scale_equal':
        return int(min((real & (c12 == d) & (c8 == d)).sum(), (real & (c12 == d) & (c8 == np.nextafter(d, np.float32(0)))).sum()))
    if cond == 'scale_below':                              # between scale2 and dist_max: in; on dist_max: out
        return int(min((real & (c12 < d) & (c8 > c12) & (c8 < d)).sum(), (real & (c12 < d) & (c8 == d)).sum()))
    # ---- seams, phases
    if cond == 'm0_gt64_kk_gt64':                          # csh = 7 with a live table
        return sum(r['m0'] > 64 and 64 < r['kk'] <= 128 for r in steps)
    if cond == 'first_new_gt64':
        first = next(r for r in traces[0][:-1] if r['kk'])
        return int(len(first['new_cols']) > 64)
    if cond == 'merge_a_lt64_le_b':
        return sum(a < 64 <= b for _, a, b in pairs)
    if cond == 'merge_64_le_a':
        return sum(64 <= a < b for _, a, b in pairs)
    if cond == 'merge_far':
        return sum(b - a >= 16 for _, a, b in pairs)
    if cond == 'merge':
        return len(pairs)
    if cond == 'two_partners':                             # last one wins, both deleted
        return sum(len({b for a2, b in r['pairs'] if a2 == a}) >= 2 and a not in r['deleted'] for r in steps for a in {a for a, _ in r['pairs']})
    if cond == 'deleted_is_a':
        return sum(a in r['deleted'] for r, a, _ in pairs)
    if cond == 'deleted_both_sides':
        return sum(bool(r['deleted']) and min(r['deleted']) < 64 <= max(r['deleted']) for r in steps)
    if cond == 'multi_b':
        return sum(len(r['multi_b']) for r in steps)
    if cond == 'multi_b_across_64':
        return sum(min(cols) < 64 <= max(cols) for r in steps for _, cols in r['multi_b'])
    if cond == 'new_col_ge64_live':
        return sum(r['m0'] > 0 and c >= 64 for r in steps for c in r['new_cols'])
    if cond in ('phaseA', 'phaseB'):
        return sum(r['any' + cond[-1]] for r in steps)
    if cond == 'cfg_distinct':                             # no other configuration gives these poses
        mine = trace(limbs[0], sk, n_kp, cfg)[0]
        others = [trace(limbs[0], sk, n_kp, CFGS[o])[0] for o in 'dgsl' if o != case.cfg]
        return int(all(o.shape != mine.shape or (o != mine).any() for o in others))
    # ---- overflow
    created, live = [t[-2]['P'] for t in traces], [max(r['M'] for r in t[:-1]) for t in traces]
    if cond == 'mmax_eq_created':
        return int(case.mmax == created[0])
    if cond == 'mmax_eq_created_minus_1':
        return int(case.mmax == created[0] - 1)
    if cond == 'live_le_mmax_lt_created':
        return int(live[0] <= case.mmax < created[0] - 1)
    if cond in ('status0', 'status1'):
        return int((created[0] > case.mmax) == (cond == 'status1'))
    if cond == 'only_middle_overflows':
        return int(len(created) == 3 and created[1] > MMAX and created[0] <= MMAX and created[2] <= MMAX and min(len(f['order']) for f in finals) > 0)
    if cond == 'created_gt_512':
        return int(max(created) > 512)
    if cond == 'final_mmax_odd':
        return int(mmax % 2 == 1 and mmax >= max(created))
    if cond == 'fits_exactly':
        return int(created[0] == MMAX == mmax)
    # ---- delete_sort
    f = finals[0]
    if cond == 'mean_eq_f32_thre':
        return int((f['scores'] == F32_THRE).sum())
    if cond == 'mean_step_above':
        return int((f['scores'] == float(np.nextafter(np.float32(0.04), np.float32(1)))).sum())
    if cond == 'mean_step_below':
        return int((f['scores'] == float(np.nextafter(np.float32(0.04), np.float32(0)))).sum())
    if cond == 'eq_dropped':
        return int(((f['scores'] == F32_THRE) & ~f['kept']).sum())
    if cond == 'eq_kept':
        return int(((f['scores'] == F32_THRE) & f['kept']).sum())
    if cond.startswith('npos_'):
        return int((f['npos'][f['kept']] == int(cond[5:])).sum())
    if cond in ('rows_gt_64', 'rows_gt_256'):
        return int(f['kept'].sum() > int(cond[8:]))
    if cond in ('tie3_span_gt_64', 'tie3_span_gt_256'):
        n, kept = 0, np.nonzero(f['kept'])[0]
        for v in np.unique(f['scores'][kept]):
            same = kept[f['scores'][kept] == v]
            n += int(len(same) >= 3 and same[-1] - same[0] > int(cond[13:]))
        return n
    if cond == 'nkp_lt_17':
        return int(n_kp < 17 and max(max(c) for c in sk) == n_kp - 1)
    raise KeyError(cond)


def counts(case, traces):
    return {c: count(case, c, traces) for c in conditions(case)}


# ---------------------------------------------------------------------------------- the stored reference output
def input_sha(case):
    from helpers import sha
    return sha(build(case))


def load(name):
    """-> case, limbs (N,L,K,13) (rebuilt, sha-guarded), expected: per image the reference's poses, or None where only their count and
    sha256 are stored (`n_poses`, `poses_sha`) -- from tests/golden/grouping_edges.npz (tools/gen_golden_grouping.py)."""
    import os
    from helpers import GOLDEN
    global _FIXTURE
    if _FIXTURE is None:
        _FIXTURE = np.load(os.path.join(GOLDEN, 'grouping_edges.npz'))
    g, case = _FIXTURE, BY_NAME[name]
    limbs = build(case)
    assert input_sha(case) == str(g[f'{name}/in_sha']), "case builder drifted (not a parity failure)"
    n_poses, shas = g[f'{name}/n_poses'], g[f'{name}/poses_sha']
    poses = [g[f'{name}/poses_{i}'] if f'{name}/poses_{i}' in g.files else None for i in range(len(limbs))]
    return case, limbs, dict(n_poses=[int(n) for n in n_poses], poses_sha=[str(s) for s in shas], poses=poses)


def first_difference(ref, got, tr):
    """'row r keypoint j field f: ref x, got y; table row t, first touched at limb type l' for the first differing element"""
    if ref.shape != got.shape:
        return f'{len(got)} poses, expected {len(ref)}'
    bad = np.argwhere(ref != got)
    if not len(bad):
        return ''
    r, j, f = (int(v) for v in bad[0])
    fin = tr[-1]
    t = fin['order'][r]
    return (f'row {r} keypoint {j} field {f}: expected {ref[r, j, f]!r}, got {got[r, j, f]!r}; table row {t}, created at limb type '
            f'{fin["hist"][t][0]}, touched at {fin["hist"][t]}')


_FIXTURE = None
