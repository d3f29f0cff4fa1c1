"""scored_off device cost at bs8 640x640, --topk 32: one JSON line (and profiles/scored_offset_bench.json with --out).

HIP events on the launch stream, 60 warm-up + 30 timed launches each, one event pair round the 30 launches:
  (a) the torch-op formulation of decoder/offset.py on device tensors (gather, broadcasts, two avg_pool2d, divide);
  (b) og_scored_offset_f32, with GB/s over its algorithmic bytes (per (n, l): one heat-map plane + two offset planes read, two written);
  (c) K1-fused (LimbsCollect.generate_limbs_fused) with scored_ks 0 and 3;
  (d) K1-fused with the flip merge folded in (generate_limbs_fused_flip) with scored_ks 0 and 3.
(a) + (c, scored_ks 0) is what a scored_off request cost before the refinement moved into the pairing; (c, 3) is what it costs now.

    python tools/scored_offset_bench.py [--out profiles/scored_offset_bench.json]
"""
import argparse
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WARM, TIMED = 60, 30


def torch_formulation(hmp, off, jtypes_f, kernel_size):
    """decoder/offset.py's CPU formulation, run on whatever device the tensors are on."""
    import torch.nn.functional as F
    n, _, h, w = off.shape
    pad = (kernel_size - 1) // 2
    weight = hmp[:, jtypes_f]
    pairs = off.view(n, -1, 2, h, w)
    num = F.avg_pool2d((weight.unsqueeze(2) * pairs).view(n, -1, h, w), kernel_size, stride=1, padding=pad, divisor_override=1)
    den = F.avg_pool2d(weight, kernel_size, stride=1, padding=pad, divisor_override=1)
    return (num.view(n, -1, 2, h, w) / (den.unsqueeze(2) + 1e-6)).view(n, -1, h, w)


def timed_us(fn, dev):
    import torch
    from offsetguided_amd import _lib
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize(dev)
    a, b = _lib.TimingEvent(), _lib.TimingEvent()
    st = torch.cuda.current_stream(dev)
    a.record(st)
    for _ in range(TIMED):
        fn()
    b.record(st)
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) * 1e3 / TIMED


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--topk', type=int, default=32)
    ap.add_argument('--out', default=None)
    ap.add_argument('--commit', default=None, help='recorded in the JSON (default: git rev-parse of the checkout)')
    a = ap.parse_args()
    import torch
    from offsetguided_amd import _lib, synth
    from offsetguided_amd.config.coco_data import COCO_KEYPOINTS, COCO_PERSON_SKELETON, heatmap_hflip, offset_hflip
    from offsetguided_amd.decoder.collect import LimbsCollect
    from offsetguided_amd.decoder.offset import pack_jtypes, scored_offset_device
    dev = torch.device('cuda:0')
    _lib.load()
    hm, off = synth.synth_batch(1, a.batch, a.size, a.size, flip=True)
    hm2, off2 = torch.from_numpy(hm).to(dev), torch.from_numpy(off).to(dev)
    hm1, off1 = hm2[:a.batch].contiguous(), off2[:a.batch].contiguous()
    skel = COCO_PERSON_SKELETON
    jf, _ = pack_jtypes(skel)
    kp = heatmap_hflip(COCO_KEYPOINTS)
    perm, rev = offset_hflip(COCO_KEYPOINTS, skel)
    keep = [1 if l in rev else 0 for l in range(len(skel))]
    col = LimbsCollect(4, 4, topk=a.topk, thre_hmp=0.04, min_len=0.5)
    h = w = a.size // 4
    alg_bytes = a.batch * len(skel) * 5 * h * w * 4
    res = {'metric': 'scored_offset_device_cost', 'unit': 'us per launch', 'batch': a.batch, 'size': a.size, 'topk': a.topk,
           'warmup': WARM, 'timed': TIMED, 'box': socket.gethostname(),
           'commit': a.commit or subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None}
    res['torch_ops_ks3'] = round(timed_us(lambda: torch_formulation(hm1, off1, jf, 3), dev), 2)
    for ks in (3, 7):
        us = timed_us(lambda: scored_offset_device(hm1, off1, jf, ks), dev)
        res[f'kernel_ks{ks}'] = round(us, 2)
        res[f'kernel_ks{ks}_GBps'] = round(alg_bytes / us / 1e3, 1)
    res['kernel_algorithmic_bytes'] = alg_bytes
    for ks in (0, 3):
        res[f'k1f_scored_ks{ks}'] = round(timed_us(lambda: col.generate_limbs_fused(hm1, off1, scored_ks=ks), dev), 2)
        res[f'k1f_flip_scored_ks{ks}'] = round(timed_us(lambda: col.generate_limbs_fused_flip(hm2, off2, kp, perm, keep, scored_ks=ks), dev), 2)
    res['request_before'] = round(res['torch_ops_ks3'] + res['k1f_scored_ks0'], 2)      # torch passes + K1f
    res['request_now'] = res['k1f_scored_ks3']
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
