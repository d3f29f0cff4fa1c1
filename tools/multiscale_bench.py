"""Multi-scale test throughput (evaluate.run_images --test-scales): one JSON line.

Seeded raw uint8 host images (eight COCO-like sizes), --batch-size 8, --long-edge 640, bench.py's weights (bench_init):
  * run_images img/s for --test-scales 1, 0.5 1 1.5, and 0.5 1 1.5 with --flip-test;
  * in the same run, the single-scale img/s of every padded shape those scales use (--long-edge 384 / 640 / 1024: the engines of
    scales 0.5 / 1 / 1.5) and the harmonic combination 1 / sum(1 / R_s) of them -- what running the scales back to back would give;
  * the merge (og_scale_accumulate_f32) device time per scale from HIP events (a separate, profiled pass), its share of the device
    time of a multi-scale step, and its achieved bytes/s on the algorithmic bytes (source planes read + accumulator read and write).

    python tools/multiscale_bench.py [--batches 12] [--warm 4] [--out profiles/multiscale_bench.json]
A kernel trace: rocprofv3 --kernel-trace --stats -d DIR -o ms -- python tools/multiscale_bench.py (kernel name: scale_accumulate_kernel).
"""
import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = [(480, 640), (427, 640), (640, 480), (375, 500), (500, 375), (640, 640), (333, 500), (612, 612)]
C_HM, L = 17, 19


def run(model, dev, batch, long_edge, scales, flip, n_batches, warm, profile=False):
    """-> (img/s over the timed batches, {stage: [us]} when profiled)."""
    import torch
    from offsetguided_amd import _lib, evaluate
    rng = np.random.default_rng(0)
    base = [rng.integers(0, 256, size=hw + (3,), dtype=np.uint8) for hw in SIZES]
    argv = ['--no-pretrain', '--topk', '32', '--thre-hmp', '0.04', '--person-thre', '0.04', '--dist-max', '40', '--batch-size',
            str(batch), '--long-edge', str(long_edge), '--print-freq', '1000000000', '--test-scales', *map(str, scales)]
    args = evaluate.evaluate_cli(argv + (['--flip-test'] if flip else []))
    marks = {}

    def loader():
        for b in range(n_batches + warm + 1):
            if b in (warm, warm + n_batches):
                torch.cuda.synchronize(dev)
                if b == warm and profile:
                    _lib.profile_start()
                marks['t0' if b == warm else 't1'] = time.perf_counter()
            yield [base[(b + i) % len(base)] for i in range(batch)], [None] * batch, [{'image_id': b * batch + i} for i in range(batch)]
    with contextlib.redirect_stdout(sys.stderr):
        evaluate.run_images(args, loader(), model=model)
    torch.cuda.synchronize(dev)
    prof = _lib.profile_stop() if profile else None
    return n_batches * batch / (marks['t1'] - marks['t0']), prof


def merge_bytes(batch, flip, long_edge, scales):
    """Algorithmic bytes of the merge launches of one batch: each source plane read once (twice the images with flip), the
    accumulator written (first scale) or read and written (the others)."""
    from offsetguided_amd.transforms import multi_scale_sizes
    base_P = multi_scale_sizes(long_edge, 1.0)[1] // 4
    acc = batch * (C_HM + 2 * L) * base_P * base_P * 4
    total = 0
    for i, s in enumerate(scales):
        P = multi_scale_sizes(long_edge, s)[1] // 4
        total += (2 if flip else 1) * batch * (C_HM + 2 * L) * P * P * 4 + acc * (1 if i == 0 else 2)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--long-edge', type=int, default=640)
    ap.add_argument('--batches', type=int, default=12)
    ap.add_argument('--warm', type=int, default=4)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import bench
    from offsetguided_amd import models
    from offsetguided_amd.transforms import multi_scale_sizes
    dev = torch.device('cuda:0')
    p = argparse.ArgumentParser()
    models.net_cli(p)
    model, _ = models.model_factory(p.parse_args(['--no-pretrain']))
    bench.bench_init(model, 0)
    model = model.to(dev).eval()
    scales = [0.5, 1.0, 1.5]
    res = {'metric': 'multiscale_run_images', 'unit': 'images/sec', 'batch': a.batch, 'long_edge': a.long_edge, 'scales': scales,
           'batches_timed': a.batches}
    for flip in (False, True):
        tag = 'flip' if flip else 'noflip'
        single = {}
        for s in scales:
            P = multi_scale_sizes(a.long_edge, s)[1]
            single[str(P)] = round(run(model, dev, a.batch, P, [1.0], flip, a.batches, a.warm)[0], 2)
        multi = run(model, dev, a.batch, a.long_edge, scales, flip, a.batches, a.warm)[0]
        harmonic = 1.0 / sum(1.0 / v for v in single.values())
        _, prof = run(model, dev, a.batch, a.long_edge, scales, flip, a.batches, a.warm, profile=True)
        merge_us = prof.get('scale_merge', [])      # (the loader runs a batch ahead: a few launches more than batches x scales)
        per_batch_us = float(np.mean(merge_us)) * len(scales)
        step_us = 1e6 * a.batch / multi
        res[tag] = {
            'multi_scale': round(multi, 2),
            'single_scale_by_padded_size': single,
            'harmonic_of_single': round(harmonic, 2),
            'multi_over_harmonic': round(multi / harmonic, 4),
            'merge_us_per_scale': round(per_batch_us / len(scales), 2),
            'merge_launches_profiled': len(merge_us),
            'merge_share_of_step': round(per_batch_us / step_us, 5),
            'merge_bytes_per_s': round(merge_bytes(a.batch, flip, a.long_edge, scales) / (per_batch_us * 1e-6), 0),
        }
    res['single_scale_640'] = res['noflip']['single_scale_by_padded_size'][str(multi_scale_sizes(a.long_edge, 1.0)[1])]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
