"""COCOeval's keypoint protocol (pycocotools/cocoeval.py with iouType='keypoints': computeOks, evaluateImg, accumulate,
_summarizeKps) restated with straight Python loops on Python floats (IEEE double), and the directed case the scorer is held to.
Shares no code with offsetguided_amd/cocoeval.py: the constants are written out again here.

build_case() -> (ground_truth, results, image_ids, notes); restate(ground_truth, results, image_ids) -> dict of numpy arrays.
match_rows(...) is the matching rule of one image on its own (restate calls it; tests/oks_match_cases.py feeds it hand-written OKS
blocks).  build_oks_table() / oks_table_reference() are the directed table for og_oks_matrix_f64, build_perfect_case() a set of
detections that coincide with their ground truths.
"""
import math

import numpy as np

K = 17
SIGMAS = [.026, .025, .025, .035, .035, .079, .079, .072, .072, .062, .062, .107, .107, .087, .087, .089, .089]
IOU_THRS = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1)
REC_THRS = np.linspace(0, 1, int(np.round((1 - 0) / 0.01)) + 1)
MAX_DETS = 20
AREA_RANGES = [[0, 1e10], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
EPS = float(np.spacing(1))
GAP = 1e-9


def oks_pair(det, gt, area, bbox, sigmas=SIGMAS):
    """det, gt: 17 rows [x, y, v]; bbox [x, y, w, h]."""
    k1 = 0
    for k in range(K):
        if gt[k][2] > 0:
            k1 += 1
    total, n = 0.0, 0
    for k in range(K):
        xd, yd, xg, yg = float(det[k][0]), float(det[k][1]), float(gt[k][0]), float(gt[k][1])
        if k1 > 0:
            if not gt[k][2] > 0:
                continue
            dx, dy = xd - xg, yd - yg
        else:
            bx, by, bw, bh = (float(v) for v in bbox)
            x0, x1, y0, y1 = bx - bw, bx + bw * 2, by - bh, by + bh * 2
            dx = max(0.0, x0 - xd) + max(0.0, xd - x1)
            dy = max(0.0, y0 - yd) + max(0.0, yd - y1)
        var = (sigmas[k] * 2) * (sigmas[k] * 2)
        e = (dx * dx + dy * dy) / var / (float(area) + EPS) / 2
        total += math.exp(-e)
        n += 1
    return total / n


def match_rows(oks_rows, gt_area, gt_ignore, gt_crowd, det_area, area_ranges, thresholds):
    """evaluateImg's matching of one image for every (area range, threshold).  oks_rows: d rows of g values (detections in score
    order); gt_ignore: iscrowd or num_keypoints == 0, before the area range is applied.
    -> (dt_match (A,T,d) int32: 1 + the matched ground truth's index or 0, dt_ignore (A,T,d) uint8, gt_ignore_a (A,g) uint8)."""
    n_d, n_g = len(det_area), len(gt_area)
    rows = [[float(v) for v in row] for row in oks_rows]
    assert len(rows) == n_d and all(len(row) == n_g for row in rows) and len(gt_ignore) == len(gt_crowd) == n_g
    area, d_area = [float(v) for v in gt_area], [float(v) for v in det_area]
    ignore, crowd = [bool(v) for v in gt_ignore], [bool(v) for v in gt_crowd]
    A, T = len(area_ranges), len(thresholds)
    dt_match, dt_ignore = np.zeros((A, T, n_d), np.int32), np.zeros((A, T, n_d), np.uint8)
    gt_ignore_a = np.zeros((A, n_g), np.uint8)
    for a, (lo, hi) in enumerate(area_ranges):
        lo, hi = float(lo), float(hi)
        for t, thr in enumerate(thresholds):
            gig = [ignore[j] or area[j] < lo or area[j] > hi for j in range(n_g)]
            visit = [j for j in range(n_g) if not gig[j]] + [j for j in range(n_g) if gig[j]]
            taken = [False] * n_g
            for d in range(n_d):
                best, m = min(float(thr), 1 - 1e-10), -1
                for j in visit:
                    if taken[j] and not crowd[j]:
                        continue
                    if m > -1 and not gig[m] and gig[j]:
                        break
                    if rows[d][j] < best:
                        continue
                    best, m = rows[d][j], j
                if m > -1:
                    dt_match[a, t, d], dt_ignore[a, t, d] = m + 1, gig[m]
                    taken[m] = True
                elif d_area[d] < lo or d_area[d] > hi:
                    dt_ignore[a, t, d] = 1
            for j in range(n_g):
                gt_ignore_a[a, j] = gig[j]
    return dt_match, dt_ignore, gt_ignore_a


def restate(ground_truth, results, image_ids, sigmas=SIGMAS):
    """-> {'oks' (packed, image after image, row-major d_i x g_i), 'det_off', 'gt_off', 'dt_match' (A,T,D), 'dt_ignore' (A,T,D),
    'gt_ignore_a' (A,G), 'precision' (T,R,A), 'recall' (T,A), 'stats' (10)}.  image_ids must not repeat."""
    A, T, R = len(AREA_RANGES), len(IOU_THRS), len(REC_THRS)
    assert len(set(image_ids)) == len(image_ids)
    images = []
    for image_id in image_ids:
        dets = [r for r in results if r['image_id'] == image_id]
        order = sorted(range(len(dets)), key=lambda j: -dets[j]['score'])[:MAX_DETS]      # sorted() is stable
        d_kp, d_score, d_area = [], [], []
        for j in order:
            kp = [dets[j]['keypoints'][3 * k:3 * k + 3] for k in range(K)]
            xs, ys = [float(p[0]) for p in kp], [float(p[1]) for p in kp]
            d_kp.append(kp)
            d_score.append(float(dets[j]['score']))
            d_area.append((max(xs) - min(xs)) * (max(ys) - min(ys)))
        gt = ground_truth.get(image_id)
        g_n = 0 if gt is None else len(gt['area'])
        g = {'kp': [], 'area': [], 'bbox': [], 'crowd': [], 'ignore': []}
        for j in range(g_n):
            g['kp'].append([[float(v) for v in row] for row in np.asarray(gt['keypoints'][j]).reshape(K, 3)])
            g['area'].append(float(gt['area'][j]))
            g['bbox'].append([float(v) for v in gt['bbox'][j]])
            g['crowd'].append(bool(gt['iscrowd'][j]))
            g['ignore'].append(bool(gt['iscrowd'][j]) or int(gt['num_keypoints'][j]) == 0)
        oks = [[oks_pair(d_kp[d], g['kp'][j], g['area'][j], g['bbox'][j], sigmas) for j in range(g_n)] for d in range(len(d_kp))]
        images.append({'kp': d_kp, 'score': d_score, 'area': d_area, 'gt': g, 'oks': oks})
    D, G = sum(len(im['score']) for im in images), sum(len(im['gt']['area']) for im in images)
    dt_match, dt_ignore = np.zeros((A, T, D), np.int32), np.zeros((A, T, D), np.uint8)
    gt_ignore_a = np.zeros((A, G), np.uint8)
    d0 = g0 = 0
    for im in images:
        g, n_d, n_g = im['gt'], len(im['score']), len(im['gt']['area'])
        dt_match[:, :, d0:d0 + n_d], dt_ignore[:, :, d0:d0 + n_d], gt_ignore_a[:, g0:g0 + n_g] = match_rows(
            im['oks'], g['area'], g['ignore'], g['crowd'], im['area'], AREA_RANGES, IOU_THRS)
        d0, g0 = d0 + n_d, g0 + n_g
    scores = [s for im in images for s in im['score']]
    order = sorted(range(D), key=lambda j: -scores[j])
    precision, recall = -np.ones((T, R, A)), -np.ones((T, A))
    for a in range(A):
        npig = sum(1 for j in range(G) if gt_ignore_a[a, j] == 0)
        if npig == 0:
            continue
        for t in range(T):
            tp = fp = 0
            rc, pr = [], []
            for j in order:
                if not dt_ignore[a, t, j]:
                    if dt_match[a, t, j] != 0:
                        tp += 1
                    else:
                        fp += 1
                rc.append(float(tp) / npig)
                pr.append(float(tp) / (float(fp) + float(tp) + EPS))
            recall[t, a] = rc[-1] if D else 0
            for i in range(D - 1, 0, -1):
                if pr[i] > pr[i - 1]:
                    pr[i - 1] = pr[i]
            for r, rec in enumerate(REC_THRS):
                i = 0
                while i < D and rc[i] < rec:          # searchsorted(rc, rec, side='left')
                    i += 1
                precision[t, r, a] = pr[i] if i < D else 0.0

    def figure(ap, iou_thr, a):
        ts = range(T) if iou_thr is None else [t for t in range(T) if IOU_THRS[t] == iou_thr]
        vals = ([precision[t, r, a] for t in ts for r in range(R)] if ap else [recall[t, a] for t in ts])
        vals = np.array([v for v in vals if v > -1], np.float64)
        return float(np.mean(vals)) if len(vals) else -1.0        # np.mean like COCOeval: pairwise summation

    stats = np.array([figure(True, None, 0), figure(True, .5, 0), figure(True, .75, 0), figure(True, None, 1), figure(True, None, 2),
                      figure(False, None, 0), figure(False, .5, 0), figure(False, .75, 0), figure(False, None, 1),
                      figure(False, None, 2)])
    det_off = np.cumsum([0] + [len(im['score']) for im in images])
    gt_off = np.cumsum([0] + [len(im['gt']['area']) for im in images])
    return {'oks': np.array([v for im in images for row in im['oks'] for v in row], np.float64), 'rows': [row for im in images
                                                                                                          for row in im['oks']],
            'det_off': det_off, 'gt_off': gt_off, 'dt_match': dt_match, 'dt_ignore': dt_ignore, 'gt_ignore_a': gt_ignore_a,
            'precision': precision, 'recall': recall, 'stats': stats}


# ---- the directed case ----
# unit-height figure (y down), origin at the hips
_FIGURE = np.array([[0.00, -0.52], [0.03, -0.55], [-0.03, -0.55], [0.06, -0.53], [-0.06, -0.53], [0.12, -0.40], [-0.12, -0.40],
                    [0.16, -0.22], [-0.16, -0.22], [0.18, -0.05], [-0.18, -0.05], [0.08, 0.00], [-0.08, 0.00], [0.09, 0.22],
                    [-0.09, 0.22], [0.10, 0.45], [-0.10, 0.45]])
SEED = 20


def _person(rs, centre, spread, size=80.0):
    """(17, 3) float64 [x, y, 2]: the figure at centre + U(-spread, spread), every joint jittered by N(0, 2) pixels."""
    xy = _FIGURE * size * rs.uniform(0.8, 1.2) + np.asarray(centre, float) + rs.uniform(-spread, spread, 2) + rs.normal(0, 2.0, (K, 2))
    return np.concatenate([xy, np.full((K, 1), 2.0)], 1)


def _hide(rs, kp, keep=0.85):
    """COCO style: an unannotated joint is [0, 0, 0]; at least one joint stays."""
    kp = kp.copy()
    gone = rs.uniform(size=K) > keep
    gone[rs.randint(K)] = False
    kp[gone] = 0.0
    return kp


def _near(rs, kp, noise):
    out = kp.copy()
    out[:, :2] += rs.normal(0, noise, (K, 2))
    out[:, 2] = 2.0
    return out


def _gt(rows):
    """rows: [(keypoints (17,3), area, iscrowd)] -> load_ground_truth's per-image dict (bbox = the extent of the annotated joints)."""
    kps, boxes = [], []
    for kp, _, _ in rows:
        seen = kp[kp[:, 2] > 0]
        x0, y0 = (seen[:, 0].min(), seen[:, 1].min()) if len(seen) else (0.0, 0.0)
        x1, y1 = (seen[:, 0].max(), seen[:, 1].max()) if len(seen) else (0.0, 0.0)
        kps.append(kp)
        boxes.append([x0, y0, x1 - x0, y1 - y0])
    return {'keypoints': np.array(kps, np.float64).reshape(len(rows), K, 3), 'area': np.array([r[1] for r in rows], np.float64),
            'bbox': np.array(boxes, np.float64).reshape(len(rows), 4), 'iscrowd': np.array([r[2] for r in rows], np.uint8),
            'num_keypoints': np.array([int((kp[:, 2] > 0).sum()) for kp, _, _ in rows], np.int64)}


def _results(image_id, dets):
    """dets: [(keypoints (17,3), score)] -> result dicts as evaluate.poses_to_results writes them."""
    return [{'image_id': image_id, 'category_id': 1, 'keypoints': [float(v) for v in np.asarray(kp).reshape(-1)], 'score': float(s)}
            for kp, s in dets]


def build_case(seed=SEED):
    """I = 8 images; `notes` names the rows the directed situations sit in (packed indices after the sort and the truncation are
    found by the tests through the restatement)."""
    rs = np.random.RandomState(seed)
    c = (150.0, 150.0)
    gt, res, notes = {}, [], {}
    image_ids = [7, 3, 11, 5, 2, 13, 17, 19]

    # 7: detections, no ground truth (one of them the all-zero placeholder of an image without poses)
    res += _results(7, [(_person(rs, c, 30), 0.61), (np.zeros((K, 3)), 0.01)])
    # 3: ground truth, no detections (an entry with small and medium area)
    gt[3] = _gt([(_hide(rs, _person(rs, c, 30)), 500.0, 0), (_hide(rs, _person(rs, c, 30)), 4000.0, 0)])
    # 11: neither (and no entry in the ground truth at all)
    # 5: 25 detections against a small, a medium and a large ground truth; the scores at sorted positions 20 and 21 are equal
    g5 = [(_hide(rs, _person(rs, c, 8)), 1000.0, 0), (_hide(rs, _person(rs, c, 8)), 5000.0, 0), (_hide(rs, _person(rs, c, 8)), 20000.0, 0)]
    gt[5] = _gt(g5)
    ranked = [0.95 - 0.03 * j for j in range(25)]
    ranked[20] = ranked[19]
    ranks = list(rs.permutation(25))
    d5 = [(_near(rs, g5[j][0], 0.5) if j < 3 else _person(rs, c, 10), ranked[ranks[j]]) for j in range(25)]
    res += _results(5, d5)
    notes['equal_scores'] = sorted(j for j in range(25) if ranks[j] in (19, 20))     # detection rows of image 5 with the equal scores
    # 2: a crowd two detections both match, a num_keypoints == 0 annotation that is not crowd (the bbox branch), an ordinary one
    crowd, plain = _person(rs, (115.0, 150.0), 5), _hide(rs, _person(rs, (185.0, 150.0), 5))
    gt[2] = _gt([(crowd, 12000.0, 1), (np.zeros((K, 3)), 4000.0, 0), (plain, 8000.0, 0)])
    gt[2]['bbox'][1] = [120.0, 90.0, 30.0, 40.0]
    res += _results(2, [(_near(rs, crowd, 0.8), 0.9), (_near(rs, crowd, 1.2), 0.8), (_near(rs, plain, 1.0), 0.7),
                        (_person(rs, (150.0, 150.0), 10), 0.6)])
    # 13: the stop rule (ground truth 0 counts, 1 is a crowd six pixels away that detection 0 sits on), the tie rule (2 and 3 are
    # identical), two detections on ground truth 4 (the second a false positive)
    a_kp = _person(rs, (105.0, 120.0), 3)
    b_kp = a_kp.copy()
    b_kp[:, :2] += [6.0, 4.0]
    c_kp, e_kp = _person(rs, (150.0, 120.0), 3), _person(rs, (195.0, 120.0), 3)
    gt[13] = _gt([(a_kp, 9000.0, 0), (b_kp, 9000.0, 1), (c_kp, 15000.0, 0), (c_kp.copy(), 15000.0, 0), (e_kp, 12000.0, 0)])
    res += _results(13, [(_near(rs, b_kp, 0.3), 0.95), (_near(rs, c_kp, 1.0), 0.9), (_near(rs, c_kp, 1.5), 0.85),
                         (_near(rs, e_kp, 1.0), 0.8), (_near(rs, e_kp, 2.0), 0.75)])
    # 17: 70 ground truths (areas on both sides of 96^2, every ninth a crowd) and 16 detections: more than 64 ground truths and
    # more than 1024 pairs
    g17 = [(_hide(rs, _person(rs, c, 25)), float(rs.uniform(5000.0, 30000.0)), int(j % 9 == 4)) for j in range(70)]
    gt[17] = _gt(g17)
    res += _results(17, [(_near(rs, g17[5 * j][0], 1.0) if j < 10 else _person(rs, c, 25), float(rs.uniform(0.05, 0.99)))
                         for j in range(16)])
    # 19: an ordinary image
    g19 = [(_hide(rs, _person(rs, c, 25)), area, 0) for area in (3000.0, 7000.0, 11000.0, 25000.0)]
    gt[19] = _gt(g19)
    res += _results(19, [(_near(rs, g19[j][0], 2.0) if j < 3 else _person(rs, c, 25), float(rs.uniform(0.1, 0.9))) for j in range(5)])
    # a result of an image that is not scored, and ground truth of one that is not scored
    res += _results(23, [(_person(rs, c, 30), 0.99)])
    gt[29] = _gt([(_person(rs, c, 30), 6000.0, 0)])
    notes['identical_gts'] = {13: (2, 3)}
    return gt, res, image_ids, notes


def check_gaps(ref, image_ids, notes):
    """The condition the case is built to: no OKS within GAP of a matching threshold, and within one detection's row no two values
    within GAP of each other unless they are equal by construction (identical ground truths)."""
    thrs = [min(float(t), 1 - 1e-10) for t in IOU_THRS]
    for v in ref['oks']:
        for t in thrs:
            assert abs(float(v) - t) >= GAP, (v, t)
    det_off, gt_off = ref['det_off'], ref['gt_off']
    same = {image_ids.index(im): pair for im, pair in notes['identical_gts'].items()}
    row = 0
    for i in range(len(image_ids)):
        for _ in range(det_off[i + 1] - det_off[i]):
            vals = ref['rows'][row]
            row += 1
            for j in range(len(vals)):
                for k in range(j + 1, len(vals)):
                    if (j, k) == same.get(i):
                        assert vals[j] == vals[k]          # equal by construction: the tie rule decides
                    else:
                        assert abs(vals[j] - vals[k]) >= GAP, (image_ids[i], j, k, vals[j], vals[k])
    assert row == len(ref['rows'])


# ---- the directed table for og_oks_matrix_f64 ----
SIGMA_SETS = {'coco': SIGMAS, 'flat': [0.05] * K, 'one_tiny': SIGMAS[:3] + [1e-3] + SIGMAS[4:]}
BBOX = [100.0, 100.0, 40.0, 60.0]            # the doubled box of the bbox branch: x in [60, 180], y in [40, 220]


def build_oks_table(extra=False, seed=5):
    """Images for one og_oks_matrix_f64 launch: [(dets (d,17,3), gts (g,17,3), area (g,), bbox (g,4))] and notes {name: image index}.
    256 pairs -- one full block -- or 257 with `extra` (one more 1 x 1 image); images without pairs stand first (detections only), in
    the middle (ground truths only) and last (detections only).
      ordinary   6 x 5: ground truth 2 is ground truth 1 with every v = 2 written as v = 1
      exact      3 x 3: ground truths P (area 5000), P (area 0), P with joints hidden (area 0); detections P, P + 1 px, P + 10^4 px
      bbox       6 x 2: ground truth 0 has no annotated joint and BBOX; detections: all joints inside the doubled box, all on its edges,
                 then 4 / 8 / 12 / 17 joints 3 px beyond its left / right / top / bottom side
      underflow  1 x 1: one annotated joint, 62.4 px off at area 1000: e = 720 under COCO's sigma, exp(-e) is subnormal
      filler     3 x 68 ordinary pairs"""
    rs = np.random.RandomState(seed)
    c = (150.0, 150.0)

    def img(dets, rows):
        g = _gt(rows)
        return (np.array(dets, np.float64).reshape(-1, K, 3), g['keypoints'], g['area'], g['bbox'])

    none = np.zeros((0, K, 3))
    p = [_hide(rs, _person(rs, c, 20)) for _ in range(4)]
    twin = p[1].copy()
    twin[twin[:, 2] > 0, 2] = 1.0
    ordinary = img([_near(rs, p[j % 4], 1.0 + j) for j in range(6)],
                   [(p[0], 3000.0, 0), (p[1], 6000.0, 0), (twin, 6000.0, 0), (p[2], 12000.0, 0), (p[3], 25000.0, 0)])
    P = _person(rs, c, 5)
    off1, far = P.copy(), P.copy()
    off1[:, 0] += 1.0
    far[:, :2] += 1e4
    exact = img([P.copy(), off1, far], [(P, 5000.0, 0), (P.copy(), 0.0, 0), (_hide(rs, P), 0.0, 0)])
    x0, x1, y0, y1 = 60.0, 180.0, 40.0, 220.0
    inside = np.stack([rs.uniform(x0 + 1, x1 - 1, K), rs.uniform(y0 + 1, y1 - 1, K), np.full(K, 2.0)], 1)
    edges = inside.copy()
    for k in range(K):
        edges[k, k % 2] = (x0, y0, x1, y1)[k % 4]                      # x = 60, y = 40, x = 180, y = 220 in turn
    edges[16, :2] = [x0, y1]                                            # and a corner
    beyond = []
    for n, col, value in ((4, 0, x0 - 3.0), (8, 0, x1 + 3.0), (12, 1, y0 - 3.0), (17, 1, y1 + 3.0)):
        kp = inside.copy()
        kp[:n, col] = value
        beyond.append(kp)
    bbox = img([inside, edges] + beyond, [(np.zeros((K, 3)), 4000.0, 0), (_hide(rs, _person(rs, c, 20)), 8000.0, 0)])
    bbox[3][0] = BBOX
    one = np.zeros((K, 3))
    one[0] = [100.0, 100.0, 2.0]
    off = one.copy()
    off[0, 0] += 62.4
    underflow = img([off], [(one, 1000.0, 0)])
    f = [_hide(rs, _person(rs, c, 25)) for _ in range(68)]
    filler = img([_near(rs, f[j], 3.0) for j in range(3)], [(kp, float(rs.uniform(2000.0, 30000.0)), 0) for kp in f])
    q = _hide(rs, _person(rs, c, 10))
    images = [(np.array([_person(rs, c, 10), _person(rs, c, 10)]), none, np.zeros(0), np.zeros((0, 4))), ordinary, exact,
              (none, ) + img([], [(kp, 5000.0, 0) for kp in f[:3]])[1:], bbox, underflow, filler]
    notes = {'ordinary': 1, 'exact': 2, 'bbox': 4, 'underflow': 5, 'filler': 6}
    if extra:
        images.append(img([_near(rs, q, 2.0)], [(q, 7000.0, 0)]))
        notes['extra'] = 7
    images.append((np.array([_person(rs, c, 10)]), none, np.zeros(0), np.zeros((0, 4))))
    return images, notes


def oks_table_reference(images, sigmas=SIGMAS):
    """-> the packed values (image after image, row-major d_i x g_i) from oks_pair."""
    return np.array([oks_pair(d, gts[j], area[j], bbox[j], sigmas) for dets, gts, area, bbox in images for d in dets
                     for j in range(len(gts))], np.float64)


def build_perfect_case(seed=6):
    """Two images, three ground truths each (one of area 0), far apart; one detection per ground truth with its very coordinates: every
    matching OKS is exactly 1.0.  -> (ground_truth, results, image_ids)."""
    rs = np.random.RandomState(seed)
    gt, res = {}, []
    for image_id, areas in ((31, (5000.0, 0.0, 20000.0)), (37, (900.0, 7000.0, 0.0))):
        people = [_hide(rs, _person(rs, (150.0 + 300.0 * j, 150.0), 5)) for j in range(3)]
        gt[image_id] = _gt([(kp, a, 0) for kp, a in zip(people, areas)])
        res += _results(image_id, [(kp, float(rs.uniform(0.1, 0.9))) for kp in people])
    return gt, res, [31, 37]
