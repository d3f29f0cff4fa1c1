"""Model-inspection views (csrc/views.hip) device time per entry point: one JSON line.

bs8 640x640 uint8 RGB over 17 x 160 x 160 heat maps and 38 x 160 x 160 offsets (seeded: heat maps = a dozen Gaussian bumps per channel,
so that the NMS view has peaks and the arrow view a foreground).  Per case: HIP events around `--launches` back-to-back launches of the C
entry on one stream (tables resident, no host work between them) after a warm-up, `--repeats` times; reported: median / min / max of
the per-launch mean in microseconds.  Cases: og_draw_heatmap_u8 raw and with NMS; og_draw_segments_u8 at 100 / 900 / 8000 segments per
image (random segments 10...60 px long, painter defaults: width 2, both discs of radius 3, alpha 1); og_limbs_to_segments_f32
(19 x 48 candidate rows); og_offsets_to_segments_f32 (step 7, thre 0.2).  Beside them, timed the same way: a device-to-device copy of
the image batch (what touching every pixel once costs) and, for the NMS overlay, og_upsample_bicubic4_f32 + og_hmp_nms_f32 on the same
channel count (one channel per image: what building the view's x4 plane and its NMS in memory would cost before any painting).

    python tools/views_bench.py [--launches 200] [--repeats 7] [--out profiles/views_bench.json]
A kernel trace: rocprofv3 --kernel-trace --stats -d DIR -o views -- python tools/views_bench.py (kernel names: draw_heatmap_kernel,
draw_segments_kernel, limbs_to_segments_kernel, offsets_to_segments_kernel).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.draw_bench import timed  # noqa: E402

N, H, W, C, L, K = 8, 640, 640, 17, 19, 48


def bumps(rng, planes, h, w, count=12, sigma=2.5):
    """(planes, h, w) float32: `count` Gaussian bumps of height 0.3 ... 1 per plane."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out = np.zeros((planes, h, w), np.float32)
    for p in range(planes):
        for cy, cx, a in zip(rng.uniform(0, h, count), rng.uniform(0, w, count), rng.uniform(0.3, 1.0, count)):
            out[p] = np.maximum(out[p], a * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sigma * sigma)))
    return out


def random_segments(rng, count):
    """(N, count, 4) float32: x1, y1, x2, y2, 10 ... 60 px long, anywhere in the image."""
    a = rng.uniform([0.0, 0.0], [W, H], (N, count, 2))
    ang, length = rng.uniform(0, 2 * np.pi, (N, count)), rng.uniform(10.0, 60.0, (N, count))
    b = a + np.stack([np.cos(ang), np.sin(ang)], axis=2) * length[..., None]
    return np.concatenate([a, b], axis=2).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from offsetguided_amd import _lib, visualization
    if not torch.cuda.is_available():
        raise SystemExit('views_bench needs a HIP device: a time is measured on the GPU or not at all')
    dev = torch.device('cuda:0')
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev)
    st = _lib.stream_ptr(dev)
    rng = np.random.default_rng(0)
    base = torch.from_numpy(rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)).to(dev)
    images, sink = base.clone(), torch.empty_like(base)
    h, w = H // 4, W // 4
    hm = torch.from_numpy(bumps(rng, N * C, h, w).reshape(N, C, h, w)).to(dev)
    off = torch.from_numpy(rng.uniform(-30.0, 30.0, (N, 2 * L, h, w)).astype(np.float32)).to(dev)
    lut = torch.from_numpy(visualization.VIRIDIS.copy()).to(dev)
    res = {'metric': 'views_launch', 'unit': 'us [median, min, max]', 'batch': N, 'height': H, 'width': W, 'launches': a.launches,
           'repeats': a.repeats, 'image_bytes': base.numel()}
    run = lambda fn: timed(fn, stream, a.launches, a.repeats)      # noqa: E731
    copy_us = run(lambda: sink.copy_(base))
    res['copy_us'] = copy_us

    def over_copy(us):
        return round(us[0] / copy_us[0], 3)
    # ---- the heat-map overlay, raw and with NMS, against materialising the x4 plane (+ its NMS) of one channel per image
    for nms in (0, 1):
        us = run(lambda: _lib.check(lib.og_draw_heatmap_u8(_lib.ptr(images), _lib.ptr(hm), _lib.ptr(lut), 256, N, C, h, w, 3, 0.0, 1.0, 0.8,
                                                            nms, st), lib))
        res['heatmap_nms' if nms else 'heatmap_raw'] = {'draw_us': us, 'draw_over_copy': over_copy(us)}
    one = hm[:, 3].contiguous()
    hires, kept = torch.empty((N, H, W), device=dev), torch.empty((N, H, W), device=dev)

    def materialise():
        _lib.check(lib.og_upsample_bicubic4_f32(_lib.ptr(one), N, h, w, _lib.ptr(hires), st), lib)
        _lib.check(lib.og_hmp_nms_f32(_lib.ptr(hires), N, H, W, _lib.ptr(kept), st), lib)
    res['upsample_plus_nms_us'] = run(materialise)
    # ---- the segment painter
    for count in (100, 900, 8000):
        table = torch.from_numpy(random_segments(rng, count)).to(dev)
        counts = torch.full((N,), count, dtype=torch.int32, device=dev)
        images.copy_(base)
        us = run(lambda: _lib.check(lib.og_draw_segments_u8(_lib.ptr(images), _lib.ptr(table), _lib.ptr(counts), N, H, W, count, 255,
                                                             128 << 8, 2.0, 3.0, 3.0, 1.0, st), lib))
        painted = float((images != base).any(dim=3).float().mean())
        res[f'segments_{count}'] = {'draw_us': us, 'draw_over_copy': over_copy(us), 'primitives_per_image': 3 * count,
                                    'pixels_painted': round(painted, 4)}
    # ---- the two compactions
    limbs = torch.from_numpy(rng.uniform(-5.0, 60.0, (N, L, K, 13)).astype(np.float32)).to(dev)
    segs = torch.empty((N, L * K, 4), device=dev)
    n_segs = torch.empty((N,), dtype=torch.int32, device=dev)
    us = run(lambda: _lib.check(lib.og_limbs_to_segments_f32(_lib.ptr(limbs), N, L, K, -1, 20.0, _lib.ptr(segs), _lib.ptr(n_segs), st), lib))
    res['limbs_to_segments'] = {'us': us, 'rows_per_image': L * K, 'kept_per_image': round(float(n_segs.float().mean()), 1)}
    S = lib.og_offsets_segments_capacity(h, w, 7)
    segs = torch.empty((N, S, 4), device=dev)
    us = run(lambda: _lib.check(lib.og_offsets_to_segments_f32(_lib.ptr(hm), _lib.ptr(off), N, C, L, h, w, 5, 4, 7, 0.2, _lib.ptr(segs),
                                                                _lib.ptr(n_segs), st), lib))
    res['offsets_to_segments'] = {'us': us, 'grid_points_per_image': int(S), 'kept_per_image': round(float(n_segs.float().mean()), 1)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
