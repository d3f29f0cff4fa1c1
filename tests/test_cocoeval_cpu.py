"""CPU-only: the numpy restatement of COCOeval's keypoint protocol (tests/cocoeval_common.py) at the hand-derived ends of the scale, the
directed case's gap condition, cocoeval.load_ground_truth, the C ABI's argument checks, and: no device, no score (no CPU path)."""
import argparse
import ctypes
import json

import numpy as np
import pytest
import torch

import cocoeval_common as cc
import oks_match_cases as mc
from offsetguided_amd import _lib, build as og_build, cocoeval, evaluate


@pytest.fixture(scope='module')
def case():
    gt, results, image_ids, notes = cc.build_case()
    return gt, results, image_ids, notes, cc.restate(gt, results, image_ids)


def _two_images():
    rs = np.random.RandomState(1)
    people = [cc._person(rs, (150.0, 150.0), 30) for _ in range(4)]
    gt = {1: cc._gt([(people[0], 5000.0, 0), (people[1], 20000.0, 0)]), 2: cc._gt([(people[2], 6000.0, 0), (people[3], 30000.0, 0)])}
    return people, gt


def test_constants_are_the_packages():
    from offsetguided_amd.config.coco_data import COCO_PERSON_SIGMAS
    assert list(COCO_PERSON_SIGMAS) == cc.SIGMAS
    assert np.array_equal(cocoeval.IOU_THRS, cc.IOU_THRS) and len(cc.IOU_THRS) == 10
    assert np.array_equal(cocoeval.REC_THRS, cc.REC_THRS) and len(cc.REC_THRS) == 101
    assert np.array_equal(cocoeval.AREA_RANGES, np.array(cc.AREA_RANGES, float)) and cocoeval.MAX_DETS == cc.MAX_DETS == 20


def test_case_keeps_its_gaps(case):
    gt, results, image_ids, notes, ref = case
    cc.check_gaps(ref, image_ids, notes)


def test_case_holds_every_directed_situation(case):
    gt, results, image_ids, notes, ref = case
    d, g = np.diff(ref['det_off']), np.diff(ref['gt_off'])
    at = {im: i for i, im in enumerate(image_ids)}
    assert len(image_ids) == 8
    assert d[at[7]] > 0 and g[at[7]] == 0 and d[at[3]] == 0 and g[at[3]] > 0 and d[at[11]] == 0 and g[at[11]] == 0
    assert sum(r['image_id'] == 5 for r in results) == 25 and d[at[5]] == 20                     # truncation
    s5 = sorted((r['score'] for r in results if r['image_id'] == 5), reverse=True)
    assert s5[19] == s5[20] and s5[18] > s5[19] > s5[21]                                          # equal scores at positions 20 and 21
    assert g[at[17]] == 70 and g[at[17]] > 64 and d[at[17]] * g[at[17]] > 1024                     # workspace + global-memory routes
    assert all(d[i] * g[i] <= 1024 and g[i] <= 64 for i in range(8) if i != at[17])                # the others: LDS + bit mask
    areas = np.concatenate([gt[im]['area'] for im in image_ids if im in gt])
    assert (areas < 32 ** 2).any() and ((areas >= 32 ** 2) & (areas <= 96 ** 2)).any() and (areas > 96 ** 2).any()
    assert gt[2]['num_keypoints'][1] == 0 and gt[2]['iscrowd'][1] == 0                            # the bbox branch
    m2 = ref['dt_match'][0, 0, ref['det_off'][at[2]]:ref['det_off'][at[2] + 1]]
    assert gt[2]['iscrowd'][0] == 1 and list(m2[:2]) == [1, 1]                                    # two detections on one crowd
    o13, p13 = ref['det_off'][at[13]], sum(int(d[i]) * int(g[i]) for i in range(at[13]))
    oks13 = ref['oks'][p13:p13 + 25].reshape(5, 5)
    m13 = ref['dt_match'][0, 0, o13:o13 + 5]
    assert oks13[0, 1] > oks13[0, 0] >= 0.5 and gt[13]['iscrowd'][1] == 1 and m13[0] == 1            # the stop rule
    assert oks13[1, 2] == oks13[1, 3] and m13[1] == 4 and m13[2] == 3                              # the tie rule: the later one wins
    assert m13[3] == 5 and m13[4] == 0 and oks13[4, 4] >= 0.5                                      # second detection: false positive


def test_perfect_detections_score_one():
    people, gt = _two_images()
    results = cc._results(1, [(people[0], 0.9), (people[1], 0.8)]) + cc._results(2, [(people[2], 0.7), (people[3], 0.6)])
    stats = cc.restate(gt, results, [1, 2])['stats']
    assert (stats > -1).all() and (stats >= 1 - 1e-12).all()


def test_no_detections_score_zero():
    _, gt = _two_images()
    ref = cc.restate(gt, [], [1, 2])
    assert (ref['stats'] == 0).all() and (ref['precision'] == 0).all() and (ref['recall'] == 0).all()


def test_only_ignored_ground_truth_scores_nothing():
    people, gt = _two_images()
    for entry in gt.values():
        entry['iscrowd'][:] = 1
    results = cc._results(1, [(people[0], 0.9)])
    assert (cc.restate(gt, results, [1, 2])['stats'] == -1).all()


def test_false_positive_ahead_of_the_match_halves_ap50():
    """One ground truth; a far detection scores higher than the perfect one: tp = [0, 1], fp = [1, 1], precision [0, 1/2] becomes
    [1/2, 1/2] under the envelope, recall [0, 1]: 1/2 at every recall threshold."""
    rs = np.random.RandomState(2)
    person = cc._person(rs, (150.0, 150.0), 5)
    far = person.copy()
    far[:, :2] += 400.0
    gt = {1: cc._gt([(person, 20000.0, 0)])}
    stats = cc.restate(gt, cc._results(1, [(far, 0.9), (person, 0.5)]), [1])['stats']
    assert abs(stats[1] - 0.5) <= 1e-12 and abs(stats[0] - 0.5) <= 1e-12 and stats[5] == 1.0


def test_load_ground_truth(tmp_path):
    kp = [float(v) for v in range(51)]
    data = {'images': [{'id': 4}, {'id': 9}, {'id': 6}],
            'annotations': [
                {'image_id': 9, 'category_id': 1, 'keypoints': kp, 'area': 100.5, 'bbox': [1, 2, 3, 4], 'iscrowd': 0, 'num_keypoints': 16},
                {'image_id': 9, 'category_id': 2, 'keypoints': kp, 'area': 1.0, 'bbox': [0, 0, 1, 1], 'iscrowd': 0, 'num_keypoints': 16},
                {'image_id': 4, 'category_id': 1, 'keypoints': [0] * 51, 'area': 7.0, 'bbox': [5, 6, 7, 8], 'iscrowd': 1, 'num_keypoints': 0},
                {'image_id': 9, 'category_id': 1, 'keypoints': kp[::-1], 'area': 3.0, 'bbox': [9, 8, 7, 6], 'iscrowd': 0, 'num_keypoints': 17}]}
    path = tmp_path / 'person_keypoints.json'
    path.write_text(json.dumps(data))
    gt = cocoeval.load_ground_truth(str(path))
    assert sorted(gt) == [4, 6, 9]
    assert gt[9]['keypoints'].shape == (2, 17, 3) and gt[9]['keypoints'].dtype == np.float64
    assert np.array_equal(gt[9]['keypoints'][0].reshape(-1), kp) and np.array_equal(gt[9]['keypoints'][1].reshape(-1), kp[::-1])   # file order
    assert np.array_equal(gt[9]['area'], [100.5, 3.0]) and np.array_equal(gt[9]['bbox'], [[1, 2, 3, 4], [9, 8, 7, 6]])
    assert np.array_equal(gt[9]['iscrowd'], [0, 0]) and np.array_equal(gt[9]['num_keypoints'], [16, 17])
    assert np.array_equal(gt[4]['iscrowd'], [1]) and np.array_equal(gt[4]['num_keypoints'], [0])
    assert gt[6]['keypoints'].shape == (0, 17, 3) and gt[6]['area'].shape == (0,) and gt[6]['bbox'].shape == (0, 4)


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_no_cpu_scoring(case, tmp_path):
    gt, results, image_ids, _, _ = case
    with pytest.raises(_lib.OgError):
        cocoeval.KeypointEval(gt).evaluate(results, image_ids)
    with pytest.raises(_lib.OgError):
        cocoeval.oks_matrix(np.zeros((1, 17, 3)), np.zeros((1, 17, 3)), [1.0], [[0, 0, 1, 1]])
    with pytest.raises(_lib.OgError):
        evaluate.validation(argparse.Namespace(annotation_file=str(tmp_path / 'none.json'), dataset='val', dump_name='x'), scorer='native')


def test_validation_scorer_names():
    with pytest.raises(ValueError):
        evaluate.validation(argparse.Namespace(), scorer='cocoapi')
    assert evaluate.evaluate_cli(['--no-pretrain']).score is False
    a = evaluate.evaluate_cli(['--no-pretrain', '--score', '--annotation-file', 'some.json'])
    assert a.score is True and a.annotation_file == 'some.json'
    assert evaluate.evaluate_cli(['--no-pretrain']).annotation_file == evaluate.ANNOTATIONS_VAL


def test_abi_entries_and_argument_checks():
    og_build.build()
    lib = _lib.load()
    for name in ('og_oks_matrix_f64', 'og_oks_match_i32', 'og_oks_match_workspace_bytes'):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == 4 and lib.og_abi_version() == 4            # the ABI only grew
    p = ctypes.c_void_p(16)
    sig = (ctypes.c_double * 17)(*cc.SIGMAS)
    rc = lib.og_oks_matrix_f64(None, p, p, p, p, p, p, sig, 1, 1, 1, 1, p, None)
    assert rc == _lib.OG_EINVAL and b'null pointer' in lib.og_last_error()
    rc = lib.og_oks_matrix_f64(p, p, p, p, p, p, p, sig, 0, 1, 1, 1, p, None)
    assert rc == _lib.OG_EINVAL and b'I must be positive' in lib.og_last_error()
    ranges, thrs = (ctypes.c_double * 32)(), (ctypes.c_double * 16)()
    match = lambda *a: lib.og_oks_match_i32(*a)   # noqa: E731
    rc = match(p, p, p, p, p, p, p, p, ranges, 3, thrs, 10, 1, 1, 1, 1, p, None, p, p, 1 << 20, None)
    assert rc == _lib.OG_EINVAL and b'null pointer' in lib.og_last_error()
    for A, T in ((9, 8), (16, 5), (17, 1), (1, 17), (0, 4), (4, 0)):
        rc = match(p, p, p, p, p, p, p, p, ranges, A, thrs, T, 1, 1, 1, 1, p, p, p, p, 1 << 20, None)
        assert rc == _lib.OG_EINVAL and b'A * T <= 64' in lib.og_last_error(), (A, T)
    rc = match(p, p, p, p, p, p, p, p, ranges, 3, thrs, 10, 0, 1, 1, 1, p, p, p, p, 1 << 20, None)
    assert rc == _lib.OG_EINVAL and b'I must be positive' in lib.og_last_error()
    rc = match(p, p, p, p, p, p, p, p, ranges, 3, thrs, 10, 1, 1, 70, 1, p, p, p, p, 8, None)
    assert rc == _lib.OG_ENOSPC
    assert lib.og_oks_match_workspace_bytes(70, 3, 10) >= 70 * 30                 # pure host arithmetic
    assert lib.og_oks_match_workspace_bytes(70, 9, 8) == 0


# ---- the matcher's rule (cocoeval_common.match_rows) on the directed OKS blocks of tests/oks_match_cases.py ----
# The expected values below are written out by hand from COCOeval.evaluateImg, not taken from match_rows: the restatement the device
# is compared with is held to them first.

def _per_image(case):
    """[(image, dt_match (A,T,d_i), dt_ignore (A,T,d_i), gt_ignore_a (A,g_i))] from the case's expected arrays."""
    dtm, dtig, gig = mc.expected(case)
    p = mc.pack(case)
    return [(im, dtm[:, :, p['det_off'][i]:p['det_off'][i + 1]], dtig[:, :, p['det_off'][i]:p['det_off'][i + 1]],
             gig[:, p['gt_off'][i]:p['gt_off'][i + 1]]) for i, im in enumerate(case['images'])]


def test_match_rows_exact_value_set():
    assert mc.HALF_LO == 0.5 - 2.0 ** -53 < 0.5 < mc.HALF_HI == 0.5 + 2.0 ** -52
    assert mc.CLAMP == 1 - 1e-10 and np.nextafter(mc.CLAMP_LO, 1.0) == mc.CLAMP and np.nextafter(mc.ONE_LO, 2.0) == 1.0
    assert mc.THR == [float(t) for t in cocoeval.IOU_THRS] and set(mc.THR16) <= set(mc.VALUES) | {2.0}
    for case in mc.cases().values():
        assert case['pins'] and all(set(im[0].reshape(-1)) <= set(mc.VALUES) for im in case['images']), case['name']


def test_match_rows_threshold_equality():
    case = mc.cases()['threshold_equality']
    assert case['thresholds'] == [0.5, mc.THR[9], 1.0, 2.0] and mc.THR[9] < mc.CLAMP_LO
    assert list(np.diag(case['images'][0][0])) == [0.5, mc.HALF_LO, mc.HALF_HI, 1.0, mc.CLAMP, mc.ONE_LO, mc.THR[9], mc.CLAMP_LO]
    dtm, dtig, gig = mc.expected(case)
    assert dtm.tolist() == [[[1, 0, 3, 4, 5, 6, 7, 8],         # t = 0.5: 0.5 itself matches, 0.5 - 2^-53 does not
                             [0, 0, 0, 4, 5, 6, 7, 8],         # t = 0.95 (linspace's): 0.95 itself and 1 - 2^-53 match
                             [0, 0, 0, 4, 5, 6, 0, 0],         # t = 1.0 -> 1 - 1e-10: 1.0, 1 - 1e-10 and 1 - 2^-53 match, the double below not
                             [0, 0, 0, 4, 5, 6, 0, 0]]]        # t = 2.0: clamped the same way
    assert not dtig.any() and not gig.any()


def test_match_rows_ties():
    case = mc.cases()['ties']
    dtm, dtig, gig = mc.expected(case)
    #                               two counted | two ignored | counted, ignored | ignored, counted | better ignored | winner taken
    assert dtm.tolist() == [[[2, 2, 1, 2, 1, 3, 2, 1, 0]]]
    assert dtig.tolist() == [[[0, 1, 0, 0, 0, 0, 0, 0, 0]]]
    assert gig.tolist() == [[0, 0, 1, 1, 0, 1, 1, 0, 0, 1, 0, 0, 0]]
    for im in case['images'][:4]:
        assert im[0][0, 0] == im[0][0, 1] >= 0.5                    # the condition: equal doubles above the threshold
    last = case['images'][5][0]
    assert (last[1:] == last[1, 0]).all() and last[0, 2] > last[1, 0]   # three equal values, the last column taken by detection 0


def test_match_rows_crowd_and_ignore():
    case = mc.cases()['crowd']
    (mask, m0, i0, g0), (ws, m1, i1, g1), (ign, m2, i2, g2) = _per_image(case)
    # bit-mask route: the crowd (0) three times, the counted one (1) once, then the crowd again; the ignored non-crowd (2) once only
    assert m0.tolist() == [[[1, 1, 1, 2, 1, 3, 0]]] and i0.tolist() == [[[1, 1, 1, 0, 1, 1, 0]]] and g0.tolist() == [[1, 0, 1]]
    # workspace route: the crowd at index 65 three times, then ground truth 64 which counts
    assert ws[0].shape == (4, 66) and ws[3][65] == 1 and m1.tolist() == [[[66, 66, 66, 65]]] and i1.tolist() == [[[1, 1, 1, 0]]]
    assert g1.tolist() == [[0] * 65 + [1]]
    # every ground truth ignored: the non-crowd one once, the crowd for the rest
    assert ign[2].all() and m2.tolist() == [[[1, 2, 2]]] and i2.tolist() == [[[1, 1, 1]]] and g2.tolist() == [[1, 1]]


def test_match_rows_area_bounds():
    case = mc.cases()['area_bounds']
    assert case['area_ranges'] == [[0.0, 1e10], [1024.0, 9216.0], [9216.0, 1e10], [2000.0, 5000.0]]
    (b, m0, i0, g0), (dec, m1, i1, g1) = _per_image(case)
    assert list(b[1]) == [2000.0, 5000.0, 1999.0, 5001.0, 20000.0] and list(b[4][5:]) == [2000.0, 5000.0, 1999.0, 5001.0]
    assert m0.tolist() == [[[1, 2, 3, 4, 5, 0, 0, 0, 0]]] * 4               # an ignored ground truth is still matched (pass 1)
    assert g0.tolist() == [[0, 0, 0, 0, 0], [0, 0, 0, 0, 1], [1, 1, 1, 1, 0], [0, 0, 1, 1, 1]]     # 2000 and 5000 are inside [2000, 5000]
    assert i0.tolist() == [[[0, 0, 0, 0, 0, 0, 0, 0, 0]], [[0, 0, 0, 0, 1, 0, 0, 0, 0]], [[1, 1, 1, 1, 0, 1, 1, 1, 1]],
                           [[0, 0, 1, 1, 1, 0, 0, 1, 1]]]                   # unmatched detections: the same strict bounds
    assert m1.tolist() == [[[1]], [[2]], [[1]], [[2]]] and not i1.any()     # lanes differ: the ground truth of the range that counts
    assert g1.tolist() == [[0, 0], [1, 0], [0, 1], [1, 0]]


@pytest.mark.parametrize('lanes', list(mc.LANES))
def test_routes_and_seams_case_holds_its_conditions(lanes):
    A, T = lanes
    case = mc.cases()[f'routes_seams_a{A}_t{T}']
    p, per = mc.pack(case), _per_image(case)
    assert (p['A'], p['T']) == lanes and p['A'] * p['T'] in (1, 64, 30)
    shapes = [im[0].shape for im in case['images']]
    at = {s: shapes.index(s) for s in mc.LARGE_SHAPES}
    route = mc.routes(case)
    assert [route[at[s]] for s in mc.LARGE_SHAPES] == [(True, True), (True, True), (True, False), (True, False), (False, True),
                                                       (False, False), (False, False), (False, False)]
    assert 16 * 64 == 64 * 16 == 1024 and 41 * 25 == 1025 and max(d for d, _ in shapes) == mc.MAX_DET
    ws = [i for i, r in enumerate(route) if not r[0]]
    assert ws == list(range(ws[0], ws[0] + 4)) and all(route[i][0] for i in range(ws[0])) and p['gt_off'][ws[0]] > 0
    assert route[ws[0]][1] and not route[ws[1]][1]                       # the staged workspace image is followed by a global one
    none = [i for i in range(p['I']) if p['pair_off'][i] == p['pair_off'][i + 1]]
    assert 0 in none and p['I'] - 1 in none and any(0 < i < p['I'] - 1 for i in none)
    assert any(shapes[i][0] > 0 for i in none) and any(shapes[i][1] > 0 for i in none)
    for s in mc.LARGE_SHAPES:
        im, dtm, dtig, gig = per[at[s]]
        d, g = s
        matched = set(np.unique(dtm)) - {0}
        assert g in matched, s                                            # the last ground truth, in every lane set
        if g > 64:
            assert max(matched) > 64, s                                   # through the workspace, past the mask's width
        if s in ((20, 52), (16, 65), (1, 1025), (64, 80), (41, 25)):
            pair = np.array([[(k * g + m - 1) for k, m in enumerate(row) if m > 0] for row in dtm.reshape(-1, d)], dtype=object)
            assert max(max(r) for r in pair if len(r)) >= 1024, s         # a decisive match in a pair past the 1024th
        if A * T > 1:
            assert len({dtm[a, t].tobytes() for a in range(A) for t in range(T)}) > 1, s      # lanes differ
        if d > 1:                                                         # a detection whose best column was taken: the matched set decides
            best_taken = [(k, m) for row in dtm.reshape(-1, d) for k, m in enumerate(row) if m > 0 and im[0][k, m - 1] < im[0][k].max()]
            assert best_taken, s
            assert {m - 1 for _, m in best_taken} & set(range(32, g)) or g <= 32, s


def test_routes_and_seams_special_indices_decide():
    """Over the four lane sets, every large image is matched at each of ground truths 31, 32, 63, 64 and the last it has; with all
    sixteen area ranges the one-row image is matched at all five."""
    seen = {s: set() for s in mc.LARGE_SHAPES}
    for A, T in mc.LANES:
        case = mc.cases()[f'routes_seams_a{A}_t{T}']
        for im, dtm, _, _ in _per_image(case):
            if im[0].shape in seen:
                seen[im[0].shape] |= set(int(m) - 1 for m in np.unique(dtm) if m > 0)
                if (A, T) == (16, 4) and im[0].shape == (1, 1025):
                    assert set(int(m) - 1 for m in np.unique(dtm) if m > 0) >= {31, 32, 63, 64, 1024}
    for s, got in seen.items():
        assert got >= set(mc.special_gts(s[1])), (s, sorted(got))


def test_sweep_case_holds_its_conditions():
    case = mc.cases()['sweep']
    p = mc.pack(case)
    dtm, dtig, gig = mc.expected(case)
    shapes = [im[0].shape for im in case['images']]
    assert p['I'] == 60 and sum(s in mc.LARGE_SHAPES for s in shapes) >= 5 and p['A'] * p['T'] == 64
    assert p['A'] * p['T'] * p['n_pairs'] < 3_000_000
    assert all(d <= 24 and g <= 40 for d, g in shapes if (d, g) not in mc.LARGE_SHAPES)
    assert any(d == 0 and g > 0 for d, g in shapes) and any(g == 0 and d > 0 for d, g in shapes)      # both kinds of image without pairs
    thr = [min(t, mc.CLAMP) for t in case['thresholds']]
    on_threshold = ties = 0
    for i, im in enumerate(case['images']):
        d0 = p['det_off'][i]
        for k, row in enumerate(im[0]):
            ties += len(row) > 1 and np.sort(row)[-1] == np.sort(row)[-2] >= 0.5
            for t in range(p['T']):
                m = dtm[0, t, d0 + k]
                on_threshold += m > 0 and row[m - 1] == thr[t]
    assert ties >= 100 and on_threshold >= 100, (ties, on_threshold)
    assert (dtm > 0).mean() > 0.1 and (dtm == 0).mean() > 0.1 and dtig.any() and gig.any() and not gig.all()
    assert len({dtm[a, t].tobytes() for a in range(p['A']) for t in range(p['T'])}) >= 32


def test_workspace_bytes_is_the_restated_formula():
    og_build.build()
    lib = _lib.load()
    for case in mc.cases().values():
        p = mc.pack(case)
        assert lib.og_oks_match_workspace_bytes(p['G'], p['A'], p['T']) == mc.workspace_bytes(p['G'], p['A'], p['T']) >= p['G'] * p['A'] * p['T']
    for G, A, T in ((0, 1, 1), (1, 1, 1), (16, 1, 1), (17, 1, 1), (1407, 16, 4), (1, 16, 4)):
        assert lib.og_oks_match_workspace_bytes(G, A, T) == mc.workspace_bytes(G, A, T) == -(-G * A * T // 16) * 16 + 16
    assert 13 * 5 == 65 and lib.og_oks_match_workspace_bytes(70, 13, 5) == mc.workspace_bytes(70, 13, 5) == 0
    assert lib.og_oks_match_workspace_bytes(70, 16, 4) > 0 and lib.og_oks_match_workspace_bytes(-1, 1, 1) == 0


# ---- the directed table for og_oks_matrix_f64 (cocoeval_common.build_oks_table) ----

def _blocks(images, values):
    off = np.cumsum([0] + [len(d) * len(g) for d, g, _, _ in images])
    return [values[off[i]:off[i + 1]].reshape(len(im[0]), len(im[1])) for i, im in enumerate(images)]


@pytest.mark.parametrize('extra', [False, True])
def test_oks_table_holds_its_cells(extra):
    images, notes = cc.build_oks_table(extra)
    shapes = [(len(d), len(g)) for d, g, _, _ in images]
    assert sum(d * g for d, g in shapes) == (257 if extra else 256)               # one full block of the kernel | one pair more
    assert shapes[0] == (2, 0) and shapes[3] == (0, 3) and shapes[-1] == (1, 0) and 0 < 3 < len(shapes) - 1
    assert all(d * g > 0 for d, g in shapes[1:3] + shapes[4:-1])
    for name, sigmas in cc.SIGMA_SETS.items():
        b = _blocks(images, cc.oks_table_reference(images, sigmas))
        o, e, x = b[notes['ordinary']], b[notes['exact']], b[notes['bbox']]
        g = images[notes['ordinary']][1]
        assert {2.0} <= set(g[1][:, 2]) <= {0.0, 2.0} and {1.0} <= set(g[2][:, 2]) <= {0.0, 1.0} and np.array_equal(g[1][:, :2], g[2][:, :2])
        assert np.array_equal(o[:, 1], o[:, 2]) and (o > 0).all() and (o < 1).all()          # v = 1 against v = 2
        assert list(images[notes['exact']][2]) == [5000.0, 0.0, 0.0]
        assert e[0].tolist() == [1.0, 1.0, 1.0] and e[1, 1:].tolist() == [0.0, 0.0] and e[2].tolist() == [0.0, 0.0, 0.0], name
        assert 0.9 < e[1, 0] < 1.0
        assert 2 * 1e4 ** 2 / max((2 * s) ** 2 for s in sigmas) / 5000.0 / 2 > 800             # the far detection: every e > 800
        assert not images[notes['bbox']][1][0].any() and list(images[notes['bbox']][3][0]) == cc.BBOX
        assert x[0, 0] == 1.0 and x[1, 0] == 1.0 and len(set(x[2:, 0])) == 4 and (x[2:, 0] > 0.5).all() and (x[2:, 0] < 1).all(), name
    kp = images[notes['bbox']][0][1]                                              # the detection on the doubled box's edges
    assert all(kp[k, 0] in (60.0, 180.0) or kp[k, 1] in (40.0, 220.0) for k in range(17))
    assert {60.0, 180.0} <= set(kp[:, 0]) and {40.0, 220.0} <= set(kp[:, 1])
    assert 700 < 62.4 ** 2 / (2 * cc.SIGMAS[0]) ** 2 / (1000.0 + cc.EPS) / 2 < 745
    u = _blocks(images, cc.oks_table_reference(images))[notes['underflow']]
    assert 0 < u[0, 0] < 2.3e-308                                                 # subnormal


def test_perfect_case_scores_exactly_one():
    gt, results, image_ids = cc.build_perfect_case()
    ref = cc.restate(gt, results, image_ids)
    assert sorted(np.concatenate([g['area'] for g in gt.values()]))[:2] == [0.0, 0.0]
    assert (np.sort(ref['oks'].reshape(2, 3, 3), axis=2)[:, :, 2] == 1.0).all() and (np.sort(ref['oks'].reshape(2, 3, 3), axis=2)[:, :, 1] < 0.5).all()
    assert ref['stats'][0] == 1.0 and (ref['dt_match'][0] > 0).all()
