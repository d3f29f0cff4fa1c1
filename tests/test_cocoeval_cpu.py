"""CPU-only: the numpy restatement of COCOeval's keypoint protocol (tests/cocoeval_common.py) at the hand-derived ends of the scale, the
directed case's gap condition, cocoeval.load_ground_truth, the C ABI's argument checks, and: no device, no score (no CPU path)."""
import argparse
import ctypes
import json

import numpy as np
import pytest
import torch

import cocoeval_common as cc
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
