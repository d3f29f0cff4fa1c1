"""Device cost of the keypoint-scale / jitter heads under flip-test and --test-scales at bs8 640x640, --topk 32, both heads: one JSON
line (and profiles/heads_tta_bench.json with --out).

Two libraries are timed in ONE session, in child processes that alternate (parent, this, parent, this, ...; --rounds of each): this
checkout's libog_decoder.so and the PARENT commit's, built beside it (--parent-lib, default tools/build/libog_parent.so):

    git archive HEAD~1 offsetguided_amd include | tar -x -C tools/build/parent_src
    python tools/build/parent_src/offsetguided_amd/build.py && cp tools/build/parent_src/offsetguided_amd/libog_decoder.so tools/build/libog_parent.so

Every figure is the median of TIMED (40) launches after WARM (40), each launch between its own pair of HIP timing events; per arm the
median over the rounds is reported with the min..max of the rounds (the spread of repeating the same command on the same code).
  (i)   a flip-test request with both heads up to the limbs: the parent's route (K0 og_flip_merge_f32 + the torch-op head merges +
        K1-fused, restated here on the parent's library) against this commit's folded route (the scale / jitter pairs in the descriptor);
  (ii)  the same with the fold off: K0 + og_flip_merge_heads_f32 + K1-fused;
  (iii) the scale-merge launch of one scale (flip pair, 96 x 96 -> 160 x 160): four maps against the two-map launch;
  (iv)  K1-fused without heads, plain and folded flip, on both libraries.
The parent's library lacks the new entry points: its arm types what the library has and runs only what the parent could run.
Both arms call through this checkout's decoder.collect, i.e. with the descriptor of ABI 4: a parent library built before ABI 4 can no
longer be loaded for the A/B (profiles/heads_tta_bench.json was recorded against an ABI 3 parent, before the descriptor).

    python tools/heads_tta_bench.py [--out profiles/heads_tta_bench.json]
"""
import argparse
import ctypes
import json
import os
import socket
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WARM, TIMED = 40, 40


def load_library(path):
    """This checkout's library through _lib.load(); a foreign one (the parent's) typed for the entry points it has."""
    from offsetguided_amd import _lib
    if path is None:
        return _lib.load()
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    _lib._lib = lib
    return lib


def median_us(fn, dev):
    import torch
    from offsetguided_amd import _lib
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize(dev)
    st = torch.cuda.current_stream(dev)
    pairs = []
    for _ in range(TIMED):
        a, b = _lib.TimingEvent(), _lib.TimingEvent()
        a.record(st)
        fn()
        b.record(st)
        pairs.append((a, b))
    torch.cuda.synchronize(dev)
    return statistics.median(a.elapsed_time(b) * 1e3 for a, b in pairs)


def arm(a):
    import numpy as np
    import torch
    from offsetguided_amd import decoder, synth
    from offsetguided_amd.config.coco_data import COCO_KEYPOINTS, heatmap_hflip
    from offsetguided_amd.decoder import multiscale
    is_parent = a.arm == 'parent'
    load_library(a.parent_lib if is_parent else None)
    dev = torch.device('cuda:0')
    p = argparse.ArgumentParser()
    decoder.decoder_cli(p)
    d = p.parse_args(['--topk', str(a.topk), '--thre-hmp', '0.04', '--person-thre', '0.04', '--dist-max', '40', '--min-len', '0.5'])
    d.headnets, d.strides, d.batch_size = ['hmp', 'omp'], [4, 4], a.batch
    d.include_scale = d.include_jitter_offset = True
    proc = decoder.decoder_factory(d)
    g = a.size // 4
    hm, off = synth.synth_batch(1, a.batch, a.size, a.size, flip=True)
    nb = hm.shape[0]
    scl = (synth.noise_batch(6, (nb, 17, g, g)) * 20 + 25).astype(np.float32)
    jit = ((synth.noise_batch(10, (nb, 2, g, g)) - 0.5) * 3.0).astype(np.float32)
    hm2, off2, scl2, jit2 = (torch.from_numpy(x).to(dev) for x in (hm, off, scl, jit))
    feats = [([None, hm2], [[], []], [None, jit2]), ([None, off2], [[], []], [None, scl2])]
    n, kp = a.batch, heatmap_hflip(COCO_KEYPOINTS)
    col = proc.limb_collect
    res = {}

    def parent_request():      # flip_augment as the parent had it: K0, then the torch ops per head, then K1-fused
        proc.include_scale = proc.include_jitter_offset = False
        mh, _, mo, _, _ = proc.flip_augment(hm2, [], off2, [], False, 2)
        proc.include_scale = proc.include_jitter_offset = True
        fl = torch.flip(jit2[n:], [-1])
        fl[:, ::2] *= -1
        mj = (jit2[:n] + fl) / 2
        ms = (scl2[:n] + torch.flip(scl2[n:], [-1])[:, kp]) / 2
        return col.generate_limbs_fused(mh, mo, 2, ms, 'bicubic', mj)

    if is_parent:
        res['i_request_parent_route'] = median_us(parent_request, dev)
    else:
        proc.fold_flip = True
        res['i_request_folded'] = median_us(lambda: proc.generate_limbs(feats, flip_test=True), dev)
        proc.fold_flip = False
        res['ii_request_unfolded'] = median_us(lambda: proc.generate_limbs(feats, flip_test=True), dev)
        exp = parent_request()
        proc.fold_flip = True
        assert torch.equal(proc.generate_limbs(feats, flip_test=True), exp), 'folded route differs from the parent route'
    # (iii) one scale of the multi-scale merge, flip pair
    hs, L = 96, 19
    gen = torch.Generator().manual_seed(2)
    m_hm, m_off = torch.randn(2 * n, 17, hs, hs, generator=gen).to(dev), torch.randn(2 * n, 2 * L, hs, hs, generator=gen).to(dev)
    m_scl, m_jit = torch.rand(2 * n, 17, hs, hs, generator=gen).to(dev), torch.randn(2 * n, 2, hs, hs, generator=gen).to(dev)
    aff = torch.tensor([[0.6, -0.2, 0.6, -0.2, 1 / 0.6, 1 / 0.6]] * n, dtype=torch.float32, device=dev)
    acc = tuple(torch.empty(n, ch, g, g, device=dev) for ch in (17, 2 * L, 17, 2))
    res['iii_scale_merge_two_maps'] = median_us(lambda: multiscale.accumulate_scale(m_hm, m_off, aff, acc[:2], 0, 1.0, True), dev)
    if not is_parent:
        res['iii_scale_merge_four_maps'] = median_us(
            lambda: multiscale.accumulate_scale(m_hm, m_off, aff, acc, 0, 1.0, True, scl=m_scl, jit=m_jit), dev)
    # (iv) K1-fused without heads
    hm1, off1 = hm2[:n].contiguous(), off2[:n].contiguous()
    perm, rev = proc.limbs_flips
    keep = [1 if l in rev else 0 for l in range(len(perm))]
    res['iv_k1f_no_heads'] = median_us(lambda: col.generate_limbs_fused(hm1, off1), dev)
    res['iv_k1f_flip_no_heads'] = median_us(lambda: col.generate_limbs_fused_flip(hm2, off2, kp, perm, keep), dev)
    print('ARM ' + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--topk', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--parent-lib', default=os.path.join(ROOT, 'tools', 'build', 'libog_parent.so'))
    ap.add_argument('--arm', choices=['parent', 'this'], default=None, help='(internal) run one arm in this process')
    ap.add_argument('--out', default=None)
    ap.add_argument('--commit', default=None)
    a = ap.parse_args()
    if a.arm:
        return arm(a)
    if not os.path.exists(a.parent_lib):
        sys.exit(f'{a.parent_lib} is missing: build the parent commit\'s library first (see the docstring)')
    runs = {'parent': [], 'this': []}
    for _ in range(a.rounds):
        for which in ('parent', 'this'):      # alternating, a fresh process each (one library per process)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--arm', which, '--batch', str(a.batch), '--size', str(a.size),
                                  '--topk', str(a.topk), '--parent-lib', a.parent_lib], capture_output=True, text=True, timeout=240)
            if out.returncode != 0:
                sys.exit(f'arm {which} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}')
            runs[which].append(json.loads([l for l in out.stdout.splitlines() if l.startswith('ARM ')][-1][4:]))
    res = {'metric': 'heads_tta_device_cost', 'unit': 'us per launch (median of launches; median [min, max] over rounds)', 'batch': a.batch,
           'size': a.size, 'topk': a.topk, 'warmup': WARM, 'timed': TIMED, 'rounds': a.rounds, 'box': socket.gethostname(),
           'commit': a.commit or subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None}
    for which, rs in runs.items():
        for key in rs[0]:
            v = [r[key] for r in rs]
            res[f'{which}.{key}'] = [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
