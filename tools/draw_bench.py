"""Pose painter (og_draw_poses_u8, visualization.draw_poses) device time: one JSON line.

bs8 640x640 uint8 RGB, COCO skeleton, painter defaults (line width 2, marker radius 3, alpha 1), 1 / 8 / 32 seeded persons per image
(a person = 17 keypoints scattered in a box of 60...200 x 120...400 px somewhere in the image).  Per person count: HIP events around
`--launches` back-to-back launches of the C entry on one stream (tables resident, no host work between them) after a warm-up, `--repeats`
times; reported: median / min / max of the per-launch mean in microseconds.  Repainting the same buffer costs the same each time: coverage
does not depend on the pixels.  Next to it, timed the same way, the batch's own pass-through copy (a device-to-device copy of the
8 x 640 x 640 x 3 bytes: every byte read and written once) -- what touching every pixel once costs, to read the painter's time against.

    python tools/draw_bench.py [--launches 200] [--repeats 7] [--out profiles/draw_bench.json]
A kernel trace: rocprofv3 --kernel-trace --stats -d DIR -o draw -- python tools/draw_bench.py (kernel name: draw_poses_kernel).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, H, W, K = 8, 640, 640, 17


def persons(rng, count):
    """(N, count, K, 3) float32: x, y, v."""
    size = rng.uniform([60.0, 120.0], [200.0, 400.0], (N, count, 1, 2))
    corner = rng.uniform(0.0, 1.0, (N, count, 1, 2)) * (np.array([W, H]) - size)
    xy = corner + rng.uniform(0.0, 1.0, (N, count, K, 2)) * size
    return np.concatenate([xy, np.ones((N, count, K, 1))], axis=3).astype(np.float32)


def timed(fn, stream, launches, repeats, warm=20):
    """Per-call device time of fn() in microseconds: [median, min, max] over `repeats` windows of `launches` calls."""
    import torch
    from offsetguided_amd import _lib
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = _lib.TimingEvent(), _lib.TimingEvent()
        a.record(stream)
        for _ in range(launches):
            fn()
        b.record(stream)
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / launches)
    return [round(float(np.median(out)), 2), round(min(out), 2), round(max(out), 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from offsetguided_amd import _lib, visualization
    from offsetguided_amd.config import coco_data as cd
    if not torch.cuda.is_available():
        raise SystemExit('draw_bench needs a HIP device: a time is measured on the GPU or not at all')
    dev = torch.device('cuda:0')
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev)
    rng = np.random.default_rng(0)
    base = torch.from_numpy(rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)).to(dev)
    images, sink = base.clone(), torch.empty_like(base)
    skel = _lib.int_table(np.asarray(cd.COCO_PERSON_SKELETON).reshape(-1), dev)
    L = len(cd.COCO_PERSON_SKELETON)
    pal = torch.from_numpy(visualization.TAB20.copy()).to(dev)
    nbytes = base.numel()
    res = {'metric': 'draw_poses_launch', 'unit': 'us [median, min, max]', 'batch': N, 'height': H, 'width': W, 'launches': a.launches,
           'repeats': a.repeats, 'line_width': 2.0, 'marker_radius': 3.0, 'alpha': 1.0, 'image_bytes': nbytes}
    copy_us = timed(lambda: sink.copy_(base), stream, a.launches, a.repeats)
    res['copy_us'] = copy_us
    res['copy_bytes_per_s'] = round(2 * nbytes / (copy_us[0] * 1e-6), 0)      # read + write
    for count in (1, 8, 32):
        table = torch.from_numpy(persons(rng, count)).to(dev)
        counts = torch.full((N,), count, dtype=torch.int32, device=dev)

        def launch():
            _lib.check(lib.og_draw_poses_u8(_lib.ptr(images), _lib.ptr(table), _lib.ptr(counts), _lib.ptr(skel), _lib.ptr(pal), 20, N, H, W,
                                            count, K, L, 2.0, 3.0, 1.0, _lib.stream_ptr(dev)), lib)
        images.copy_(base)
        us = timed(launch, stream, a.launches, a.repeats)
        painted = float((images != base).any(dim=3).float().mean())
        res[f'persons_{count}'] = {'draw_us': us, 'draw_over_copy': round(us[0] / copy_us[0], 3), 'primitives_per_image': count * (L + K),
                                   'pixels_painted': round(painted, 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
