"""Photometric augmentation (csrc/photometric.h behind the warp, csrc/jpeg_sim.hip) device time per launch: one JSON line.

bs8, 512 x 512 crops from 640 x 480 uint8 sources, the sources and the eight seeded draws of tools/augment_bench.py.  All cases in ONE
run, timed as there: HIP events around `--launches` back-to-back launches of the C entry on one stream after a warm-up, `--repeats`
windows; reported: [median, min, max] of the per-launch mean in microseconds.  Cases: og_warp_affine_batch_u8 (the plain warp);
og_warp_affine_photo_batch_u8 with every image tinted (deltas +10, -40, +30), without and with the out_u8 copy the JPEG pass needs;
og_jpeg_roundtrip_batch_u8 at quality 50 on 1 and on 8 images; a device-to-device copy of the fp32 output (what any unfused second pass
over the batch costs at the least: it reads and writes every value once).  `tint_fused_vs_unfused_floor` = tinted launch / (plain launch
+ copy): below 1, fusing the tint into the warp's epilogue beats every two-pass arrangement.
--parent-lib PATH (a libog_decoder.so built from the parent commit): the plain entry of that library is timed in the same run,
alternating with this tree's, `plain_vs_parent` = ratio of the medians: the plain instantiation must not have changed.

    python tools/photometric_bench.py [--launches 200] [--repeats 7] [--parent-lib PATH] [--out profiles/photometric_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.augment_bench import H, N, S, W, sources  # noqa: E402
from tools.draw_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--parent-lib', default=None, help='libog_decoder.so of the parent commit: its plain warp is timed beside this one')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from offsetguided_amd import _lib, transforms
    from offsetguided_amd.config import data_mean, data_std
    if not torch.cuda.is_available():
        raise SystemExit('photometric_bench needs a HIP device: a time is measured on the GPU or not at all')
    dev = torch.device('cuda:0')
    lib = _lib.load()
    stream, st = torch.cuda.current_stream(dev), _lib.stream_ptr(dev)
    images = sources(np.random.default_rng(0))
    draws = random.Random(0)
    t = transforms.WarpAffineTransforms(S, aug_params=transforms.AugParams())
    params = [t.draw(draws) for _ in range(N)]
    mats = np.stack([t.affine_matrix(p, np.array([W // 2, H // 2], np.float32), np.array([W, H])) for p in params])
    D = np.ascontiguousarray(np.stack([transforms.inverse_rows(m, S) for m in mats]))
    raw = torch.from_numpy(np.stack(images).reshape(-1)).to(dev)
    offs, hw4 = (C.c_long * N)(), (C.c_int * (4 * N))()
    for i in range(N):
        offs[i] = i * H * W * 3
        hw4[4 * i:4 * i + 4] = [H, W, 0, 0]
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])  # noqa: E731
    mean, std, border = f3(data_mean), f3(data_std), (C.c_ubyte * 3)(124, 116, 104)
    out = torch.empty((N, 3, S, S), dtype=torch.float32, device=dev)
    sink = torch.empty_like(out)
    u8 = torch.empty((N, S, S, 3), dtype=torch.uint8, device=dev)
    Dp = D.ctypes.data_as(C.c_void_p)
    table = np.ascontiguousarray(np.tile(np.array([1, 10, -40, 30], np.int32), (N, 1)))
    tp = table.ctypes.data_as(C.c_void_p)
    sel = (C.c_int * N)(*range(N))
    run = lambda fn: timed(fn, stream, a.launches, a.repeats)      # noqa: E731

    def plain(library):
        return lambda: _lib.check(library.og_warp_affine_batch_u8(_lib.ptr(raw), offs, hw4, N, Dp, S, border, mean, std, _lib.ptr(out),
                                                                  None, st), lib)

    res = {'metric': 'photometric_launch', 'unit': 'us [median, min, max]', 'batch': N, 'crop': S, 'source': [H, W], 'launches': a.launches,
           'repeats': a.repeats, 'output_bytes': out.numel() * 4, 'tint': [10, -40, 30], 'jpeg_quality': 50}
    res['copy_us'] = run(lambda: sink.copy_(out))
    res['warp_us'] = run(plain(lib))
    if a.parent_lib:
        parent = C.CDLL(os.path.abspath(a.parent_lib))
        parent.og_warp_affine_batch_u8.restype, parent.og_warp_affine_batch_u8.argtypes = _lib.SIGNATURES['og_warp_affine_batch_u8']
        res['parent_warp_us'] = run(plain(parent))
        res['warp_us_again'] = run(plain(lib))                  # this tree, the parent, this tree: drift shows as a difference of the two
        res['plain_vs_parent'] = round((res['warp_us'][0] + res['warp_us_again'][0]) / 2 / res['parent_warp_us'][0], 4)
    res['warp_tint_us'] = run(lambda: _lib.check(lib.og_warp_affine_photo_batch_u8(_lib.ptr(raw), offs, hw4, N, Dp, S, border, mean, std,
                                                                                   _lib.ptr(out), None, tp, st), lib))
    res['warp_tint_u8_us'] = run(lambda: _lib.check(lib.og_warp_affine_photo_batch_u8(_lib.ptr(raw), offs, hw4, N, Dp, S, border, mean, std,
                                                                                      _lib.ptr(out), _lib.ptr(u8), tp, st), lib))
    torch.cuda.synchronize()                                     # u8 now holds the warped bytes the JPEG pass reads
    for count in (1, N):
        res[f'jpeg_{count}_us'] = run(lambda: _lib.check(lib.og_jpeg_roundtrip_batch_u8(_lib.ptr(u8), N, S, sel, count, 50, tp, mean, std,
                                                                                        _lib.ptr(out), st), lib))
    res['tint_fused_vs_unfused_floor'] = round(res['warp_tint_us'][0] / (res['warp_us'][0] + res['copy_us'][0]), 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
