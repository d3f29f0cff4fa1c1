"""COCO keypoint scoring (cocoeval.KeypointEval: csrc/oks.hip + numpy accumulation) on a val2017-sized synthetic problem: one JSON line.

`--images` images (default 5 000), each with 0..13 ground-truth people from synth.make_scene and 0..20 detections (ground truths plus
noise, and people of other scenes as false positives).  Timed: KeypointEval.evaluate end to end on the host clock (`--repeats` runs
after a warm-up, [median, min, max] in milliseconds: packing, one H2D copy, two launches, one D2H copy, the numpy accumulation), the two
launches alone with HIP events, and the numpy restatement of the specification (tests/cocoeval_common.py: Python loops, what
pycocotools' evaluateImg does in Python too) once on the first `--host-images` images, scaled to the whole problem.  The stats of both
are compared on that subset.

    python tools/cocoeval_bench.py [--images 5000] [--repeats 5] [--host-images 250] [--out profiles/cocoeval_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def problem(n_images, seed=0):
    """-> (ground_truth, results, image_ids) in load_ground_truth's / run_images' formats."""
    from offsetguided_amd import synth
    rng = synth.HashRng(seed)
    n_gt, n_det = rng.integers(n_images, 0, 13), rng.integers(n_images, 0, 20)
    gt, results, ids = {}, [], []
    for i in range(n_images):
        r = synth.HashRng(seed * 1000003 + i + 1)
        people = [synth.make_scene(r, 480, 640, 1) for _ in range(max(int(n_gt[i]), 1) + 3)]
        xy = np.concatenate([p[0] for p in people])
        vis = np.concatenate([p[1] for p in people])
        g = int(n_gt[i])
        kp = np.concatenate([xy[:g] * vis[:g, :, None], 2.0 * vis[:g, :, None]], 2)
        w, h = np.ptp(xy[:g, :, 0], axis=1), np.ptp(xy[:g, :, 1], axis=1)
        gt[i] = {'keypoints': kp, 'area': 0.5 * w * h, 'bbox': np.stack([xy[:g, :, 0].min(1), xy[:g, :, 1].min(1), w, h], 1),
                 'iscrowd': (r.uniform(g) < 0.05).astype(np.uint8), 'num_keypoints': vis[:g].sum(1)}
        noise = r.normal(int(n_det[i]) * 34).reshape(int(n_det[i]), 17, 2) * r.uniform(int(n_det[i]), 0.5, 12.0)[:, None, None]
        scores = r.uniform(int(n_det[i]), 0.02, 1.0)
        for j in range(int(n_det[i])):
            d = np.concatenate([xy[j % len(xy)] + noise[j], np.ones((17, 1))], 1)
            results.append({'image_id': i, 'category_id': 1, 'keypoints': d.reshape(-1).tolist(), 'score': float(scores[j])})
        ids.append(i)
    return gt, results, ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--host-images', type=int, default=250, help='images the Python restatement is timed on (scaled to --images)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from offsetguided_amd import _lib, cocoeval
    if not torch.cuda.is_available():
        raise SystemExit('cocoeval_bench needs a HIP device: a time is measured on the GPU or not at all')
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import cocoeval_common as cc
    dev = torch.device('cuda:0')
    gt, results, ids = problem(a.images)
    ev = cocoeval.KeypointEval(gt)
    ev.evaluate(results, ids)                                      # warm-up: library load, workspace, pinned allocation
    walls = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        ev.evaluate(results, ids)
        walls.append((time.perf_counter() - t0) * 1e3)
    # the two launches alone, on the packed problem of the last run
    lib = _lib.load()
    pack = cocoeval._Pack(ev._pack(results, ids))
    p = pack.to(dev)
    n_images, n_dets, n_gts, n_pairs = len(ids), int(ev.det_off[-1]), int(ev.gt_off[-1]), int(ev.pair_off[-1])
    A, T = len(ev.area_ranges), len(ev.iou_thrs)
    out = torch.zeros(max(6 * A * T * n_dets + A * n_gts, 16), dtype=torch.uint8, device=dev)
    ws_bytes = lib.og_oks_match_workspace_bytes(n_gts, A, T)
    ws = _lib.workspace(dev, ws_bytes, tag='oks_match')
    ranges, thrs = np.ascontiguousarray(ev.area_ranges, np.float64), np.ascontiguousarray(ev.iou_thrs, np.float64)
    import ctypes as C
    base, n_m, n_i = out.data_ptr(), 4 * A * T * n_dets, A * T * n_dets
    stream, st = torch.cuda.current_stream(dev), _lib.stream_ptr(dev)
    kernel_ms = {'oks_matrix': [], 'oks_match': []}
    for rep in range(a.repeats + 1):
        e = [_lib.TimingEvent() for _ in range(3)]
        e[0].record(stream)
        oks = cocoeval._launch_oks(lib, dev, p[:7], ev.sigmas, n_images, n_dets, n_gts, n_pairs)
        e[1].record(stream)
        _lib.check(lib.og_oks_match_i32(_lib.ptr(oks), p[4], p[5], p[6], p[2], p[7], p[8], p[9], ranges.ctypes.data_as(C.c_void_p), A,
                                        thrs.ctypes.data_as(C.c_void_p), T, n_images, n_dets, n_gts, n_pairs, C.c_void_p(base),
                                        C.c_void_p(base + n_m), C.c_void_p(base + n_m + n_i), _lib.ptr(ws), ws_bytes, st), lib)
        e[2].record(stream)
        torch.cuda.synchronize()
        if rep:                                                    # the first round warms the allocator
            kernel_ms['oks_matrix'].append(e[0].elapsed_time(e[1]))
            kernel_ms['oks_match'].append(e[1].elapsed_time(e[2]))
    sub = ids[:min(a.host_images, len(ids))]
    t0 = time.perf_counter()
    ref = cc.restate(gt, results, sub)
    host_s = time.perf_counter() - t0
    same = bool(np.array_equal(cocoeval.KeypointEval(gt).evaluate(results, sub).stats, ref['stats']))
    mmm = lambda v: [round(float(np.median(v)), 3), round(float(min(v)), 3), round(float(max(v)), 3)]   # noqa: E731
    res = {'metric': 'cocoeval', 'images': a.images, 'detections': n_dets, 'ground_truths': n_gts, 'pairs': n_pairs, 'repeats': a.repeats,
           'evaluate_wall_ms': mmm(walls), 'oks_matrix_kernel_ms': mmm(kernel_ms['oks_matrix']),
           'oks_match_kernel_ms': mmm(kernel_ms['oks_match']), 'restatement_images': len(sub), 'restatement_wall_s': round(host_s, 3),
           'restatement_wall_s_scaled': round(host_s * a.images / max(len(sub), 1), 2), 'stats_equal_on_subset': same,
           'stats': [round(float(v), 6) for v in ev.stats], 'unit': 'ms [median, min, max]'}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
