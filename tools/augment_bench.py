"""Training augmentation (csrc/augment.hip) device time per entry point, and what --augment costs a training step: one JSON line.

Kernel part: bs8, 512 x 512 crops from 640 x 480 uint8 sources (seeded noise with flat blocks), eight seeded draws of the default
parameters (flip 0.5, rotate +-45, scale 0.5...2, stretch 0.95...1.05, translate +-150) round the image centre.  Per case: HIP events
around `--launches` back-to-back launches of the C entry on one stream (sources and tables resident, no host work between them) after
a warm-up, `--repeats` times; reported: median / min / max of the per-launch mean in microseconds.  Cases: og_warp_affine_batch_u8
(fp32 NCHW out), og_warp_affine_mask_u8, og_affine_joints_f32 (20 persons per image); beside them a device-to-device copy of the
same fp32 output bytes (what writing the batch once costs), and the host alternative that exists offline: PIL's
Image.transform(AFFINE, BICUBIC) of the same eight images with the same matrices on 16 threads, wall clock, image only, no
normalisation -- PIL, NOT the reference's cv2.warpAffine.

Step part (--parent DIR, a built checkout of the parent commit): `train_dist --no-pretrain --bench --augment` of this tree against
`train_dist --no-pretrain --bench` of DIR, alternating, --train-repeats runs each, every run a fresh process; both lists of
ms_per_step and their [min, max] intervals go into the line, with the mean augment_us the augmented runs report.

    python tools/augment_bench.py [--launches 200] [--repeats 7] [--parent DIR] [--out profiles/augment_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import random
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.draw_bench import timed  # noqa: E402

N, S, H, W, P = 8, 512, 480, 640, 20


def sources(rng):
    images = []
    for _ in range(N):
        im = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        im[100:300, 150:450] = rng.integers(0, 256, 3, dtype=np.uint8)
        images.append(im)
    return images


def pil_host(images, D, threads=16, repeats=5):
    """Wall-clock milliseconds [median, min, max] of PIL's bicubic affine transform of the batch on a thread pool."""
    try:
        from PIL import Image
    except ImportError:
        return None
    from concurrent.futures import ThreadPoolExecutor
    pil = [Image.fromarray(im) for im in images]

    def one(i):
        return np.asarray(pil[i].transform((S, S), Image.AFFINE, data=tuple(D[i].reshape(-1)), resample=Image.BICUBIC,
                                            fillcolor=(124, 116, 104)))
    out = []
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(one, range(N)))
        for _ in range(repeats):
            t0 = time.perf_counter()
            list(pool.map(one, range(N)))
            out.append((time.perf_counter() - t0) * 1e3)
    return [round(float(np.median(out)), 2), round(min(out), 2), round(max(out), 2)]


def train_runs(parent, repeats):
    """ms_per_step of `train_dist --bench --augment` here and `train_dist --bench` in the parent checkout, alternating."""
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE')}
    res = {'augment': [], 'parent': [], 'augment_us': []}
    for _ in range(repeats):
        for name, cwd, extra in (('parent', parent, []), ('augment', ROOT, ['--augment'])):
            r = subprocess.run([sys.executable, '-m', 'offsetguided_amd.train_dist', '--no-pretrain', '--bench'] + extra, cwd=cwd, env=env,
                               capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit(f'train_dist ({name}) failed:\n{r.stderr[-2000:]}')
            line = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
            res[name].append(line['ms_per_step'])
            if 'augment_us' in line:
                res['augment_us'].append(line['augment_us'])
    return {'workload': 'train_dist --no-pretrain --bench, bs8 512x512, one rank', 'repeats': repeats,
            'parent_ms_per_step': res['parent'], 'parent_interval': [min(res['parent']), max(res['parent'])],
            'augment_ms_per_step': res['augment'], 'augment_interval': [min(res['augment']), max(res['augment'])],
            'augment_us': res['augment_us']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--parent', default=None, help='built checkout of the parent commit: adds the training-step comparison')
    ap.add_argument('--train-repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from offsetguided_amd import _lib, transforms
    from offsetguided_amd.config import data_mean, data_std
    from offsetguided_amd.train_dist import synthetic_annotations
    if not torch.cuda.is_available():
        raise SystemExit('augment_bench needs a HIP device: a time is measured on the GPU or not at all')
    dev = torch.device('cuda:0')
    lib = _lib.load()
    stream, st = torch.cuda.current_stream(dev), _lib.stream_ptr(dev)
    rng = np.random.default_rng(0)
    images = sources(rng)
    draws = random.Random(0)
    t = transforms.WarpAffineTransforms(S, aug_params=transforms.AugParams())
    params = [t.draw(draws) for _ in range(N)]
    mats = np.stack([t.affine_matrix(p, np.array([W // 2, H // 2], np.float32), np.array([W, H])) for p in params])
    D = np.ascontiguousarray(np.stack([transforms.inverse_rows(m, S) for m in mats]))
    M = np.ascontiguousarray(mats[:, :2])
    raw = torch.from_numpy(np.stack(images).reshape(-1)).to(dev)
    masks = torch.from_numpy(rng.integers(0, 2, (N, H, W), dtype=np.uint8) * 255).to(dev)
    offs, moffs, hw4 = (C.c_long * N)(), (C.c_long * N)(), (C.c_int * (4 * N))()
    for i in range(N):
        offs[i], moffs[i] = i * H * W * 3, i * H * W
        hw4[4 * i:4 * i + 4] = [H, W, 0, 0]
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])  # noqa: E731
    mean, std, border = f3(data_mean), f3(data_std), (C.c_ubyte * 3)(124, 116, 104)
    out = torch.empty((N, 3, S, S), dtype=torch.float32, device=dev)
    sink = torch.empty_like(out)
    mout = torch.empty((N, S, S), dtype=torch.uint8, device=dev)
    Dp, Mp = D.ctypes.data_as(C.c_void_p), M.ctypes.data_as(C.c_void_p)
    joints, n_persons = synthetic_annotations(0, N, H, W)
    joints = np.ascontiguousarray(np.concatenate([joints, np.zeros((N, max(P - joints.shape[1], 0), 17, 4), np.float32)], axis=1)[:, :P])
    jd, jo = torch.from_numpy(joints).to(dev), torch.empty((N, P, 17, 4), dtype=torch.float32, device=dev)
    nd = torch.from_numpy(np.minimum(n_persons, P).astype(np.int32)).to(dev)
    flips = (C.c_int * N)(*[int(p[0]) for p in params])
    scales = (C.c_double * N)(*[float(np.sqrt((p[3] * p[2]) * (p[4] * p[2]))) for p in params])
    left, right = (C.c_int * 8)(*transforms.affine.LEFT_INDEX), (C.c_int * 8)(*transforms.affine.RIGHT_INDEX)
    run = lambda fn: timed(fn, stream, a.launches, a.repeats)      # noqa: E731
    res = {'metric': 'augment_launch', 'unit': 'us [median, min, max]', 'batch': N, 'crop': S, 'source': [H, W], 'launches': a.launches,
           'repeats': a.repeats, 'output_bytes': out.numel() * 4, 'draws': [[float(v) for v in p] for p in params]}
    res['copy_us'] = run(lambda: sink.copy_(out))
    res['warp_us'] = run(lambda: _lib.check(lib.og_warp_affine_batch_u8(_lib.ptr(raw), offs, hw4, N, Dp, S, border, mean, std, _lib.ptr(out),
                                                                        None, st), lib))
    res['warp_over_copy'] = round(res['warp_us'][0] / res['copy_us'][0], 3)
    res['mask_us'] = run(lambda: _lib.check(lib.og_warp_affine_mask_u8(_lib.ptr(masks), moffs, hw4, N, Dp, S, 255, _lib.ptr(mout), st), lib))
    res['joints_us'] = run(lambda: _lib.check(lib.og_affine_joints_f32(_lib.ptr(jd), _lib.ptr(nd), N, P, 17, Mp, flips, scales, float(S),
                                                                       float(S), left, right, 8, _lib.ptr(jo), st), lib))
    res['host_pil_bicubic_16_threads_ms'] = pil_host(images, D)
    res['host_note'] = 'PIL Image.transform(AFFINE, BICUBIC), image only, no normalisation: the host alternative available offline, not cv2'
    if a.parent:
        res['train_step'] = train_runs(os.path.abspath(a.parent), a.train_repeats)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
