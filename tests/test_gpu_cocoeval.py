"""csrc/oks.hip behind cocoeval.KeypointEval against the numpy restatement of COCOeval's keypoint protocol (tests/cocoeval_common.py)
on the directed case: eight images that hold every branch of the matching, one of them with 70 ground truths (the workspace route of
the matched set and the global-memory route of the OKS block).

The OKS values are held to 1e-12 absolute.  Derived, not measured: an OKS is at most 1 and is the mean of at most 17 double exp
values, each a few ulp (2.2e-16) from libm's; 1e-12 is four orders above that and three orders below the 1e-9 gap the case keeps
between any OKS and a matching threshold and between the values of one detection's row -- so every comparison of the matching is
decided the same way on both sides and everything behind the OKS values is compared for equality.

Below that: og_oks_match_i32 called directly on hand-written OKS blocks of exact doubles (tests/oks_match_cases.py), where an OKS sits
exactly on a threshold or on another OKS of its row and no gap is needed, and og_oks_matrix_f64 on a directed table
(cocoeval_common.build_oks_table).  The conditions those cases are built to are asserted in tests/test_cocoeval_cpu.py."""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch

import cocoeval_common as cc
import oks_match_cases as mc
from offsetguided_amd import _lib, cocoeval, decoder, evaluate, synth

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


# ---- og_oks_match_i32 itself on the hand-written OKS blocks of tests/oks_match_cases.py: everything is compared for equality ----
GUARD = 256


def _ptrs(pack, pinned, dev):
    """The sections of a cocoeval._Pack as pointers: into the pinned host buffer itself, or into its device copy (as evaluate does)."""
    if not pinned:
        return pack.to(dev)
    return [C.c_void_p(pack.host.data_ptr() + off) for off in pack.offsets]


def _guarded(sizes, dev):
    """One device buffer of 0xAA bytes: a GUARD-byte band, then each section followed by a band.  -> (buffer, section offsets)."""
    at, total = [], GUARD
    for n in sizes:
        at.append(total)
        total += -(-n // GUARD) * GUARD + GUARD
    return torch.full((total,), 0xAA, dtype=torch.uint8, device=dev), at


def _match_call(lib, p, tables, data, out_ptrs, ws_ptr, ws_bytes, dev, A=None, T=None):
    A, T = A or p['A'], T or p['T']
    return lib.og_oks_match_i32(data[0], tables[0], tables[1], tables[2], data[1], data[2], data[3], data[4],
                                p['area_ranges'].ctypes.data_as(C.c_void_p), A, p['thresholds'].ctypes.data_as(C.c_void_p), T, p['I'],
                                p['D'], p['G'], p['n_pairs'], out_ptrs[0], out_ptrs[1], out_ptrs[2], ws_ptr, ws_bytes,
                                _lib.stream_ptr(dev))


def _run_match(case, pinned):
    """Twice on one workspace that starts as 0xff bytes, the outputs refilled with the sentinel in between.  Asserts per call: the
    bands around the outputs and the workspace are untouched (nothing outside [0, A T D) is written), every output element is written,
    and the outputs equal match_rows'."""
    dev = torch.device('cuda:0')
    lib = _lib.load()
    p = mc.pack(case)
    want = mc.expected(case)
    A, T, D, G = p['A'], p['T'], p['D'], p['G']
    data_pack = cocoeval._Pack([p['oks'], p['gt_area'], p['gt_ignore'], p['gt_crowd'], p['det_area']])
    table_pack = cocoeval._Pack([p['det_off'], p['gt_off'], p['pair_off']])
    data, tables = data_pack.to(dev), _ptrs(table_pack, pinned, dev)
    sizes = [4 * A * T * D, A * T * D, A * G]
    ws_bytes = lib.og_oks_match_workspace_bytes(G, A, T)
    assert ws_bytes == mc.workspace_bytes(G, A, T) > 0
    ws, (ws_at,) = _guarded([ws_bytes], dev)
    ws[ws_at:ws_at + ws_bytes] = 0xff
    calls = []
    for _ in range(2):
        out, at = _guarded(sizes, dev)
        out[at[0]:at[0] + sizes[0]].view(torch.int32).fill_(-7)
        rc = _match_call(lib, p, tables, data, [C.c_void_p(out.data_ptr() + o) for o in at], C.c_void_p(ws.data_ptr() + ws_at), ws_bytes, dev)
        _lib.check(rc, lib)
        host, ws_host = out.cpu().numpy(), ws.cpu().numpy()
        inside = np.zeros(host.size, bool)
        for o, n in zip(at, sizes):
            inside[o:o + n] = True
        assert (host[~inside] == 0xAA).all(), 'a byte outside the outputs was written'
        assert (ws_host[:ws_at] == 0xAA).all() and (ws_host[ws_at + ws_bytes:] == 0xAA).all(), 'a byte outside the workspace was written'
        dtm = host[at[0]:at[0] + sizes[0]].view(np.int32).reshape(A, T, D)
        dtig = host[at[1]:at[1] + sizes[1]].reshape(A, T, D)
        gig = host[at[2]:at[2] + sizes[2]].reshape(A, G)
        assert (dtm != -7).all() and (dtig != 0xAA).all() and (gig != 0xAA).all(), 'an output element was left unwritten'
        assert np.array_equal(dtm, want[0]), np.argwhere(dtm != want[0])[:8]
        assert np.array_equal(dtig, want[1]), np.argwhere(dtig != want[1])[:8]
        assert np.array_equal(gig, want[2]), np.argwhere(gig != want[2])[:8]
        calls.append((dtm.copy(), dtig.copy(), gig.copy()))
    assert all(np.array_equal(x, y) for x, y in zip(*calls))
    del data_pack, table_pack


@pytest.mark.parametrize('pinned', [True, False], ids=['pinned_tables', 'device_tables'])
@pytest.mark.parametrize('name', list(mc.cases()))
def test_match_entry_point_equals_match_rows(name, pinned):
    _run_match(mc.cases()[name], pinned)


def _refusal_setup(case_name):
    dev = torch.device('cuda:0')
    p = mc.pack(mc.cases()[case_name])
    data = cocoeval._Pack([p['oks'], p['gt_area'], p['gt_ignore'], p['gt_crowd'], p['det_area']])
    out, at = _guarded([4 * 64 * max(p['D'], 65), 64 * max(p['D'], 65), 16 * p['G']], dev)
    ws, (ws_at,) = _guarded([1 << 16], dev)
    return dev, p, data, data.to(dev), out, [C.c_void_p(out.data_ptr() + o) for o in at], ws, C.c_void_p(ws.data_ptr() + ws_at)


def test_match_entry_point_refusals():
    """Pinned tables: the host check reads them and decides, nothing is launched -- the outputs and the workspace keep their fill."""
    lib = _lib.load()
    dev, p, keep, data, out, out_ptrs, ws, ws_ptr = _refusal_setup('crowd')
    good = [p['det_off'], p['gt_off'], p['pair_off']]

    def refused(tables, code, text, q=p, ws_bytes=1 << 16, **lanes):
        pack = cocoeval._Pack(tables)
        rc = _match_call(lib, q, _ptrs(pack, True, dev), data, out_ptrs, ws_ptr, ws_bytes, dev, **lanes)
        assert rc == code and text in lib.og_last_error(), (rc, lib.og_last_error())

    # 65 detections in one image (tables consistent with each other and with the totals)
    q65 = dict(p, I=1, D=65, G=1, n_pairs=65)
    refused([np.array([0, 65], np.int32), np.array([0, 1], np.int32), np.array([0, 65], np.int64)], _lib.OG_EINVAL, b'at most 64', q=q65)
    # A * T = 65
    q13 = dict(p, area_ranges=np.array(mc.RANGES16[:13]), thresholds=np.array(mc.THR[:5]))
    refused(good, _lib.OG_EINVAL, b'A * T <= 64', q=q13, A=13, T=5)
    # a workspace one byte short
    need = lib.og_oks_match_workspace_bytes(p['G'], p['A'], p['T'])
    refused(good, _lib.OG_ENOSPC, b'workspace', ws_bytes=need - 1)
    # pair_off that is not d_i * g_i (still monotonic, still ending at n_pairs)
    bad = p['pair_off'].copy()
    bad[1] += 1
    refused([p['det_off'], p['gt_off'], bad], _lib.OG_EINVAL, b'is not d_i * g_i')
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xAA).all() and (ws.cpu().numpy() == 0xAA).all()
    del keep


# ---- og_oks_matrix_f64 on the directed table (cocoeval_common.build_oks_table) ----

def _oks_launch(images, sigmas):
    dev = torch.device('cuda:0')
    d, g = [len(im[0]) for im in images], [len(im[1]) for im in images]
    det_off, gt_off = np.cumsum([0] + d).astype(np.int32), np.cumsum([0] + g).astype(np.int32)
    pair_off = np.cumsum([0] + [a * b for a, b in zip(d, g)]).astype(np.int64)
    cat = lambda k, shape: np.concatenate([np.asarray(im[k], np.float64).reshape((-1,) + shape) for im in images])     # noqa: E731
    pack = cocoeval._Pack([cat(0, (17, 3)), cat(1, (17, 3)), cat(2, ()), cat(3, (4,)), det_off, gt_off, pair_off])
    n = int(pair_off[-1])
    oks = cocoeval._launch_oks(_lib.load(), dev, pack.to(dev), np.ascontiguousarray(sigmas, np.float64), len(images), int(det_off[-1]),
                               int(gt_off[-1]), n)
    got = oks[:n].cpu().numpy()
    off = pair_off
    return got, [got[off[i]:off[i + 1]].reshape(d[i], g[i]) for i in range(len(images))]


@pytest.mark.parametrize('sigma_set', list(cc.SIGMA_SETS))
@pytest.mark.parametrize('extra', [False, True], ids=['256_pairs', '257_pairs'])
def test_oks_matrix_directed_table(extra, sigma_set):
    """One launch over images with and without pairs.  Held to OKS_TOL against oks_pair: ordinary pairs, v = 1 against v = 2, the
    bbox branch beyond each side, the subnormal pair.  Held to equality: coincident joints give 1.0 (area 0 included), 1 px off at area
    0 and a far detection give 0.0, the bbox branch inside and on the edges of the doubled box gives 1.0."""
    images, notes = cc.build_oks_table(extra)
    sigmas = cc.SIGMA_SETS[sigma_set]
    want = cc.oks_table_reference(images, sigmas)
    got, b = _oks_launch(images, sigmas)
    assert got.shape == want.shape == (257 if extra else 256,)
    assert not np.isnan(got).any() and (got >= 0).all() and (got <= 1).all()
    err = np.abs(got - want).max()
    print(f'{sigma_set}: max |OKS - oks_pair| = {err:.3e} over {got.size} pairs')
    assert err <= OKS_TOL
    o, e, x = b[notes['ordinary']], b[notes['exact']], b[notes['bbox']]
    assert np.array_equal(o[:, 1], o[:, 2])                                       # v = 1 and v = 2 give the same value
    assert e[0].tolist() == [1.0, 1.0, 1.0] and e[1, 1:].tolist() == [0.0, 0.0] and e[2].tolist() == [0.0, 0.0, 0.0]
    assert x[0, 0] == 1.0 and x[1, 0] == 1.0
    # beyond the left / right / top / bottom side: which side is pinned by the comparison with oks_pair above (the four detections move
    # 4 / 8 / 12 / 17 joints, so their values differ by the count too); here only that none of them fell back to the inside value
    assert len(set(x[2:, 0])) == 4 and (x[2:, 0] < 1.0).all()
    u = b[notes['underflow']][0, 0]
    assert u >= 0 and not np.isnan(u) and abs(u - want[int(sum(v.size for v in b[:notes['underflow']]))]) <= OKS_TOL
    if extra:
        assert abs(b[notes['extra']][0, 0] - want[-1]) <= OKS_TOL and 0 < want[-1] < 1     # the pair of the second block


def test_coincident_detections_score_exactly_one():
    """One detection on each ground truth's very coordinates (two ground truths of area 0): the device's OKS is exactly 1.0 and so is
    the AP, through the kernels and not only through the restatement."""
    gt, results, image_ids = cc.build_perfect_case()
    ref = cc.restate(gt, results, image_ids)
    ev = cocoeval.KeypointEval(gt).evaluate(results, image_ids)
    assert np.array_equal(ev.oks == 1.0, ref['oks'] == 1.0) and (ev.oks == 1.0).sum() == 6
    assert np.array_equal(ev.dt_match, ref['dt_match']) and (ev.dt_match[0] > 0).all()
    assert ev.stats[0] == 1.0 and ref['stats'][0] == 1.0 and np.array_equal(ev.stats, ref['stats'])
