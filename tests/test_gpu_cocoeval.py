"""csrc/oks.hip behind cocoeval.KeypointEval against the numpy restatement of COCOeval's keypoint protocol (tests/cocoeval_common.py)
on the directed case: eight images that hold every branch of the matching, one of them with 70 ground truths (the workspace route of
the matched set and the global-memory route of the OKS block).

The OKS values are held to 1e-12 absolute.  Derived, not measured: an OKS is at most 1 and is the mean of at most 17 double exp
values, each a few ulp (2.2e-16) from libm's; 1e-12 is four orders above that and three orders below the 1e-9 gap the case keeps
between any OKS and a matching threshold and between the values of one detection's row -- so every comparison of the matching is
decided the same way on both sides and everything behind the OKS values is compared for equality."""
import argparse

import numpy as np
import pytest
import torch

import cocoeval_common as cc
from offsetguided_amd import cocoeval, decoder, evaluate, synth

pytestmark = pytest.mark.gpu
OKS_TOL = 1e-12


@pytest.fixture(scope='module')
def scored():
    gt, results, image_ids, notes = cc.build_case()
    ref = cc.restate(gt, results, image_ids)
    cc.check_gaps(ref, image_ids, notes)
    ev = cocoeval.KeypointEval(gt).evaluate(results, image_ids)
    return gt, results, image_ids, ref, ev


def test_oks_values(scored):
    *_, ref, ev = scored
    assert np.array_equal(ev.det_off, ref['det_off']) and np.array_equal(ev.gt_off, ref['gt_off'])
    assert ev.oks.dtype == np.float64 and ev.oks.shape == ref['oks'].shape == (int(ev.pair_off[-1]),)
    err = np.abs(ev.oks - ref['oks']).max()
    print(f'max |OKS - restatement| = {err:.3e} over {ev.oks.size} pairs')
    assert err <= OKS_TOL


def test_matching_is_equal(scored):
    *_, ref, ev = scored
    assert ev.dt_match.dtype == np.int32 and np.array_equal(ev.dt_match, ref['dt_match'])
    assert np.array_equal(ev.dt_ignore, ref['dt_ignore'])
    assert np.array_equal(ev.gt_ignore_a, ref['gt_ignore_a'])


def test_precision_recall_stats_are_equal(scored, capsys):
    *_, ref, ev = scored
    assert ev.precision.shape == (10, 101, 3) and ev.recall.shape == (10, 3) and ev.stats.shape == (10,)
    assert np.array_equal(ev.precision, ref['precision'])
    assert np.array_equal(ev.recall, ref['recall'])
    assert np.array_equal(ev.stats, ref['stats'])
    assert ev.summarize() is ev.stats
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 10
    assert lines[0] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets= 20 ] = %0.3f' % ref['stats'][0]
    assert lines[8] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=medium | maxDets= 20 ] = %0.3f' % ref['stats'][8]


def test_evaluating_twice_is_identical(scored):
    gt, results, image_ids, _, ev = scored
    again = cocoeval.KeypointEval(gt).evaluate(results, image_ids)
    for name in ('oks', 'dt_match', 'dt_ignore', 'gt_ignore_a', 'precision', 'recall', 'stats'):
        assert np.array_equal(getattr(again, name), getattr(ev, name)), name


def test_oks_matrix_single_image(scored):
    """Image 2 of the case: ground truth 0 and 2 take the k1 > 0 branch, ground truth 1 (num_keypoints == 0) the bbox branch."""
    gt, results, *_ = scored
    dets = np.array([r['keypoints'] for r in results if r['image_id'] == 2]).reshape(-1, 17, 3)
    g = gt[2]
    assert (g['keypoints'][1][:, 2] == 0).all() and (g['keypoints'][0][:, 2] > 0).any()
    got = cocoeval.oks_matrix(dets, g['keypoints'], g['area'], g['bbox'])
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (len(dets), 3)
    want = np.array([[cc.oks_pair(d, g['keypoints'][j], g['area'][j], g['bbox'][j]) for j in range(3)] for d in dets])
    assert 0 < want[:, 1].min() and want[:, 1].max() < 1          # the bbox branch is not at either end of its range
    assert np.abs(got.cpu().numpy() - want).max() <= OKS_TOL
    assert tuple(cocoeval.oks_matrix(dets, np.zeros((0, 17, 3)), [], np.zeros((0, 4))).shape) == (len(dets), 0)


def test_decoded_synthetic_scenes_end_to_end():
    """Noise-free synthetic head outputs -> decoder -> result dicts -> score against the scenes they were rendered from: the native
    stats equal the restatement's on the same dicts.  No AP value is asserted: nobody has measured one."""
    seed, n, size = 3, 2, 128
    p = argparse.ArgumentParser()
    decoder.decoder_cli(p)
    a = p.parse_args('--topk 32 --thre-hmp 0.04 --person-thre 0.04 --dist-max 40'.split())
    a.headnets, a.strides, a.batch_size = ['hmp', 'omp'], [4, 4], n
    a.include_scale = a.include_jitter_offset = False
    proc = decoder.decoder_factory(a)
    hm, off = synth.synth_batch(seed, n, size, size, hm_noise=0, off_noise=0)
    dev = torch.device('cuda:0')
    thm, toff = torch.from_numpy(hm).to(dev), torch.from_numpy(off).to(dev)
    poses = proc.generate_poses([([thm, thm], [[], []], [[], []]), ([toff, toff], [[], []], [[], []])])
    results, ids, gt = [], [], {}
    for i in range(n):
        meta = {'image_id': 100 + i, 'offset': np.array([0.0, 0.0]), 'scale': np.array([1.0, 1.0]), 'hflip': False}
        evaluate.poses_to_results(poses[i], meta, results, ids)
        xy, vis, _ = synth.make_scene(synth.HashRng(seed * 1000003 + i), size, size)
        kp = np.concatenate([xy * vis[..., None], 2.0 * vis[..., None]], 2)
        w, h = xy[..., 0].max(1) - xy[..., 0].min(1), xy[..., 1].max(1) - xy[..., 1].min(1)
        gt[100 + i] = {'keypoints': kp, 'area': w * h, 'bbox': np.stack([xy[..., 0].min(1), xy[..., 1].min(1), w, h], 1),
                       'iscrowd': np.zeros(len(xy), np.uint8), 'num_keypoints': vis.sum(1)}
    assert ids == [100, 101] and len(results) >= n
    ev = cocoeval.KeypointEval(gt).evaluate(results, ids)
    ref = cc.restate(gt, results, ids)
    assert np.abs(ev.oks - ref['oks']).max(initial=0) <= OKS_TOL
    print('end to end: stats', ev.stats)
    assert np.array_equal(ev.stats, ref['stats'])
    assert 0.0 <= ev.stats[0] <= 1.0
