"""Directed cases for og_oks_match_i32 (csrc/oks.hip), as data: the matcher takes the OKS block as an input, so the blocks here are
written by hand from a small set of exact doubles (VALUES) -- an OKS can sit exactly on a threshold or exactly on another OKS of its
row, and everything the matcher returns is compared for equality with cocoeval_common.match_rows.

A case is {'name', 'pins' (what it is there for), 'images', 'area_ranges' (A, 2), 'thresholds' (T,)}; an image is
(oks (d, g) float64, gt_area (g,), gt_ignore (g,) uint8, gt_crowd (g,) uint8, det_area (d,)).  gt_ignore is the flag before the area
range is applied (iscrowd or num_keypoints == 0).

    cases()         -> {name: case}: the directed cases and the seeded sweep (built once per process)
    pack(case)      -> the flat arrays the entry point takes, laid out as cocoeval.KeypointEval._pack lays them out
    expected(case)  -> (dt_match (A,T,D), dt_ignore (A,T,D), gt_ignore_a (A,G)) from match_rows, image after image (cached)
    routes(case)    -> per image (mask route?, staged in LDS?): the matcher's two choices, restated
    workspace_bytes(G, A, T) -> og_oks_match_workspace_bytes restated
"""
import numpy as np

import cocoeval_common as cc

MASK_GTS, LDS_PAIRS, MAX_DET = 64, 1024, 64          # the kernel's seams, restated: g_i <= 64 bit mask, d_i * g_i <= 1024 LDS

HALF, HALF_LO, HALF_HI = 0.5, 0.5 - 2.0 ** -53, 0.5 + 2.0 ** -52
CLAMP = 1 - 1e-10                                     # what a threshold >= 1 is clamped to
CLAMP_LO = float(np.nextafter(CLAMP, 0.0))
ONE_LO, ONE = 1.0 - 2.0 ** -53, 1.0
THR = [float(t) for t in cc.IOU_THRS]                 # 0.5 ... 0.95 as COCOeval's linspace gives them
VALUES = [0.0, 0.25, HALF_LO, HALF, HALF_HI] + THR[1:] + [CLAMP_LO, CLAMP, ONE_LO, ONE]
assert HALF_LO < HALF < HALF_HI and CLAMP_LO < CLAMP < ONE_LO < ONE and THR[0] == HALF and len(set(VALUES)) == len(VALUES) == 18

ALL = [0.0, 1e10]
# sixteen area ranges: COCO's three first; among the others ranges that hold one of AREAS only, one whose lo and hi are both an area
# of the cases (strict < and >), an empty one and a degenerate one
RANGES16 = [ALL, [32.0 ** 2, 96.0 ** 2], [96.0 ** 2, 1e10], [0.0, 32.0 ** 2], [400.0, 600.0], [1500.0, 2500.0], [4000.0, 6000.0],
            [15000.0, 25000.0], [50000.0, 1e5], [500.0, 500.0], [2000.0, 5000.0], [501.0, 1999.0], [0.0, 0.0], [5000.0, 20000.0],
            [600.0, 1e10], [0.0, 19999.0]]
THR16 = THR + [HALF_LO, HALF_HI, CLAMP, ONE_LO, 1.0, 2.0]
AREAS = [500.0, 2000.0, 5000.0, 20000.0]
LANES = {(1, 1): (RANGES16[:1], THR[:1]), (4, 16): (RANGES16[:4], THR16), (16, 4): (RANGES16, [THR[0], THR[5], THR[9], 1.0]),
         (3, 10): (RANGES16[:3], THR)}

LARGE_SHAPES = [(16, 64), (64, 16), (41, 25), (20, 52), (15, 65), (16, 65), (1, 1025), (64, 80)]


def image(oks, gt_area=None, gt_ignore=None, gt_crowd=None, det_area=None):
    oks = np.array(oks, np.float64)
    assert oks.ndim == 2
    d, g = oks.shape
    fill = lambda v, n, default, dtype: np.full(n, default, dtype) if v is None else np.array(v, dtype).reshape(n)   # noqa: E731
    return (oks, fill(gt_area, g, 5000.0, np.float64), fill(gt_ignore, g, 0, np.uint8), fill(gt_crowd, g, 0, np.uint8),
            fill(det_area, d, 5000.0, np.float64))


def empty(d, g):
    """An image without pairs: detections only, ground truths only, or neither."""
    assert d == 0 or g == 0
    return (np.zeros((d, g)), np.array(AREAS * g)[:g].astype(np.float64), np.zeros(g, np.uint8), np.zeros(g, np.uint8),
            np.array([500.0, 5000.0, 20000.0] * d)[:d].astype(np.float64))


def special_gts(g):
    """The ground-truth indices a large image's decisive matches sit at: both sides of the 32-bit and of the 64-bit seam, the last."""
    return sorted({j for j in (31, 32, 63, 64, g - 1) if j < g})


def large(d, g):
    """A (d, g) image whose matches are decided at special_gts(g) and in its last pairs.  Detection k has its best value (1.0) on the
    target of detection k - 1, which that detection has taken where it counts, and a high value on a target of its own: a matched
    set that forgets or misplaces an entry gives detection k the earlier target a second time.  The targets of the last
    detections are the special indices, so that they sit in the image's last rows (pairs past the 1024th where there are any);
    the last row has a second, lower candidate three columns before the end.  Areas cycle through AREAS, so lanes differ; ground truth
    5 is ignored for its keypoints and 7 is a crowd.

    Worked example, large(15, 65): the targets are 2, 13, 24, 35, 46, 57, 3, 14, 25, 36, 47 (the free walk 11 k + 2 mod 65) and then
    the special 31, 32, 63, 64 for detections 11 ... 14.  Row 1 is {2: 1.0, 13: 0.95, 35: 0.55}: ground truth 2 is detection 0's
    target (row 0 is {2: 0.9, 24: 0.55}), so where 2 counts detection 1 must pass over its 1.0 and take 13.  Row 12 is
    {31: 1.0, 32: 0.9, 64: 0.55}, row 13 {2: 0.55, 32: 1.0, 63: 0.95}: bit 31 and bit 32 of the matched set decide them.  Row 14 is
    {13: 0.55, 62: 0.65, 63: 1.0, 64: 1 - 2^-53}: 63 is taken, 64 wins, and 62 wins in the ranges that leave 64 (area 500) out.
    Rows 7 and 8 also hold 1.0 on the crowd 7, which wins only where no counted ground truth reaches the threshold."""
    oks = np.zeros((d, g))
    area = np.array([AREAS[j % 4] for j in range(g)])
    ign, crowd = np.zeros(g, np.uint8), np.zeros(g, np.uint8)
    if g > 8:
        ign[5] = ign[7] = crowd[7] = 1
    special = special_gts(g)
    if d == 1:                                           # one row: ties between all special columns; the range decides
        area[special] = [500.0, 2000.0, 5000.0, 20000.0, 80000.0][-len(special):]
        oks[0, special] = THR[8]
        oks[0, 7] = ONE                                  # the crowd: better, but ignored
        return image(oks, area, ign, crowd, [2000.0])
    special = special[-d:]
    free = [j for j in ((11 * k + 2) % g for k in range(4 * g)) if j not in special and j not in (5, 7)]
    targets = list(dict.fromkeys(free))[:d - len(special)] + special
    n, first = len(targets), d - len(targets)            # more detections than free ground truths: the first ones see the crowd
    assert len(set(targets)) == n and (first == 0 or g > 8)      # (matched every time) or the ignored one (matched once)
    for k in range(first):
        oks[k, 7 if k % 2 == 0 else 5] = THR[1]
    high = [THR[8], THR[9], ONE_LO, THR[7]]
    for i, j in enumerate(targets):
        k = first + i
        oks[k, j] = high[i % 4]
        if i:
            oks[k, targets[i - 1]] = ONE
        oks[k, targets[(i + 2) % n]] = max(oks[k, targets[(i + 2) % n]], THR[1])
    if g > 3:
        oks[d - 1, g - 3] = THR[3]                       # wins where the last ground truth's area is out of the range
    if g > 8:
        oks[d // 2, 7] = oks[d // 2 + 1, 7] = ONE         # two detections see the crowd at 1.0
    return image(oks, area, ign, crowd, [AREAS[(k + 1) % 4] for k in range(d)])


def small(seed, d, g):
    rs = np.random.RandomState(seed)
    return image(rs.choice(VALUES, (d, g)), rs.choice(AREAS, g), rs.uniform(size=g) < 0.2, np.zeros(g), rs.choice(AREAS, d))


def routes_and_seams(A, T):
    """Every large shape in one launch.  Order: small, the three at or just over a seam from below / above with the bit mask, then
    the four workspace-route images next to each other (their slices start at g0 * lanes) behind the mask-route ones, then small."""
    ranges, thresholds = LANES[(A, T)]
    images = [empty(3, 0), small(1, 3, 4), large(16, 64), large(64, 16), empty(0, 4), small(2, 5, 2), large(41, 25), large(20, 52),
              large(15, 65), large(16, 65), large(1, 1025), large(64, 80), small(3, 2, 2), empty(0, 0), small(4, 7, 3), empty(2, 0)]
    return {'name': f'routes_seams_a{A}_t{T}', 'images': images, 'area_ranges': ranges, 'thresholds': thresholds,
            'pins': 'all four (mask | workspace) x (LDS | global) routes, 64|65 ground truths and 1024|1025 pairs from both sides, '
                    'd_i = 64, matches at ground truths 31, 32, 63, 64 and the last, in pairs past the 1024th, adjacent workspace '
                    f'images behind mask ones, images without pairs at head, middle and tail, A x T = {A} x {T}'}


def threshold_equality():
    """One detection per ground truth, on the diagonal: column j decides on value j alone."""
    diag = [HALF, HALF_LO, HALF_HI, ONE, CLAMP, ONE_LO, THR[9], CLAMP_LO]
    return {'name': 'threshold_equality', 'images': [image(np.diag(diag))], 'area_ranges': [ALL], 'thresholds': [HALF, THR[9], 1.0, 2.0],
            'pins': 'an OKS equal to its threshold matches, two ulp below does not; thresholds 1.0 and 2.0 are clamped to 1 - 1e-10, '
                    'which 1.0, 1 - 1e-10 and 1 - 2^-53 reach and the double below 1 - 1e-10 does not'}


def ties():
    e = THR[5]
    images = [image([[e, e]]),                                                        # 0: two counted: the later wins
              image([[e, e]], gt_ignore=[1, 1]),                                      # 1: two ignored (pass 1): the later wins
              image([[e, e]], gt_ignore=[0, 1]),                                      # 2: counted then ignored: the counted one
              image([[e, e]], gt_ignore=[1, 0]),                                      # 3: ignored then counted: the counted one
              image([[THR[2], THR[8]]], gt_ignore=[0, 1]),                            # 4: a better ignored one does not replace
              image([[0.0, 0.0, THR[8]], [e, e, e], [e, e, e], [e, e, e]])]           # 5: the winner is taken: the next-later free
    return {'name': 'ties', 'images': images, 'area_ranges': [ALL], 'thresholds': [HALF],
            'pins': 'equal OKS: the later index wins among counted and among ignored ground truths, a counted one is kept against '
                    'an ignored one in either order, a taken winner passes the tie to the next-later free one'}


def crowd():
    hi, lo = THR[8], THR[2]
    mask = image([[hi, 0, 0], [hi, 0, 0], [hi, 0, 0], [hi, lo, 0], [hi, lo, 0], [0, 0, THR[6]], [0, 0, THR[6]]],
                 gt_ignore=[1, 0, 1], gt_crowd=[1, 0, 0])
    o = np.zeros((4, 66))
    o[:, 65] = hi
    o[3, 64] = lo
    ign = np.zeros(66, np.uint8)
    ign[65] = 1
    ws = image(o, gt_ignore=ign, gt_crowd=ign)
    all_ignored = image([[hi, lo], [hi, lo], [hi, lo]], gt_ignore=[1, 1], gt_crowd=[0, 1])
    return {'name': 'crowd', 'images': [mask, ws, all_ignored], 'area_ranges': [ALL], 'thresholds': [HALF],
            'pins': 'a crowd is matched by three detections and again after a counted match is taken, in the bit mask and at index 65 '
                    'through the workspace; an ignored ground truth that is no crowd is matched once; an image whose every ground '
                    'truth is ignored'}


def area_bounds():
    v = THR[8]
    bounds = image(np.concatenate([np.diag([v] * 5), np.zeros((4, 5))]), gt_area=[2000.0, 5000.0, 1999.0, 5001.0, 20000.0],
                   det_area=[2000.0, 5000.0, 1999.0, 5001.0, 20000.0, 2000.0, 5000.0, 1999.0, 5001.0])
    decides = image([[v, THR[2]]], gt_area=[20000.0, 5000.0])
    return {'name': 'area_bounds', 'images': [bounds, decides], 'area_ranges': RANGES16[:3] + [[2000.0, 5000.0]], 'thresholds': [HALF],
            'pins': 'a ground truth and an unmatched detection exactly on lo and exactly on hi of a range are inside it (< and > are '
                    'strict), one unit outside they are not; a ground truth ignored by its area in some ranges only, so that one '
                    'detection matches another ground truth from lane to lane'}


def sweep(seed=7, n=60, n_large=5):
    """Seeded: d in 0..24, g in 0..40, values from VALUES (half of them 0 or 0.25, so that rows keep free ground truths), flags at
    random, areas and detection areas from AREAS and the bounds of COCO's ranges; n_large images take a large shape."""
    rs = np.random.RandomState(seed)
    areas = AREAS + [32.0 ** 2, 96.0 ** 2]
    at = set(rs.choice(n, n_large, replace=False))
    shapes = [LARGE_SHAPES[j] for j in rs.choice(len(LARGE_SHAPES), n_large, replace=False)]
    images = []
    for i in range(n):
        d, g = shapes.pop() if i in at else (int(rs.randint(0, 25)), int(rs.randint(0, 41)))
        low = rs.uniform(size=(d, g)) < 0.5
        oks = np.where(low, rs.choice(VALUES[:2], (d, g)), rs.choice(VALUES[2:], (d, g)))
        ign = rs.uniform(size=g) < 0.2
        images.append(image(oks, rs.choice(areas, g), ign, ign & (rs.uniform(size=g) < 0.5), rs.choice(areas, d)))
    ranges, thresholds = LANES[(4, 16)]
    return {'name': 'sweep', 'images': images, 'area_ranges': ranges, 'thresholds': thresholds,
            'pins': 'dense ties and threshold equalities on random flags, a full wave of lanes'}


_cases = {}


def cases():
    if not _cases:
        for case in [threshold_equality(), ties(), crowd(), area_bounds()] + [routes_and_seams(A, T) for A, T in LANES] + [sweep()]:
            _cases[case['name']] = case
    return _cases


def pack(case):
    """-> dict of the flat arrays: oks (n_pairs,), det_off, gt_off (int32, I + 1), pair_off (int64, I + 1), gt_area, gt_ignore,
    gt_crowd, det_area, area_ranges (A, 2), thresholds (T,), and I, D, G, n_pairs, A, T."""
    ims = case['images']
    d, g = [im[0].shape[0] for im in ims], [im[0].shape[1] for im in ims]
    det_off, gt_off = np.cumsum([0] + d).astype(np.int32), np.cumsum([0] + g).astype(np.int32)
    pair_off = np.concatenate(([0], np.cumsum(np.diff(det_off).astype(np.int64) * np.diff(gt_off)))).astype(np.int64)
    cat = lambda k, dtype: np.concatenate([np.asarray(im[k], dtype).reshape(-1) for im in ims])      # noqa: E731
    ranges, thrs = np.array(case['area_ranges'], np.float64).reshape(-1, 2), np.array(case['thresholds'], np.float64)
    return {'oks': cat(0, np.float64), 'det_off': det_off, 'gt_off': gt_off, 'pair_off': pair_off, 'gt_area': cat(1, np.float64),
            'gt_ignore': cat(2, np.uint8), 'gt_crowd': cat(3, np.uint8), 'det_area': cat(4, np.float64), 'area_ranges': ranges,
            'thresholds': thrs, 'I': len(ims), 'D': int(det_off[-1]), 'G': int(gt_off[-1]), 'n_pairs': int(pair_off[-1]),
            'A': len(ranges), 'T': len(thrs)}


_expected = {}


def expected(case):
    if case['name'] not in _expected:
        parts = [cc.match_rows(*im, case['area_ranges'], case['thresholds']) for im in case['images']]
        _expected[case['name']] = tuple(np.concatenate([p[k] for p in parts], axis=-1) for k in range(3))
    return _expected[case['name']]


def routes(case):
    return [(im[0].shape[1] <= MASK_GTS, im[0].size <= LDS_PAIRS) for im in case['images']]


def workspace_bytes(G, A, T):
    if G < 0 or not 1 <= A <= 16 or not 1 <= T <= 16 or A * T > 64:
        return 0
    return -(-(G * A * T) // 16) * 16 + 16
