"""The weight average fused into the device step (optim.ModelEma, og_adam_step_ema_f32 in csrc/optim.hip) on the Hourglass-104
parameter list, clip and loss guard on: one JSON line.

Part 1, HIP events after a warm-up, `--repeats` times, [median, min, max] in microseconds.  Each tree is timed in a child process of
its own (`--parent-tree DIR`: a built checkout of the parent commit; its package and its library, named through OG_DECODER_LIB, are
what that child imports), the arms of a tree interleaved repetition by repetition:
  (a) step_ema:            this tree, DeviceAdam.step(loss=, max_grad_norm=, ema=ModelEma(model))
  (b) step:                this tree, the same step without ema
  (c) parent_step_lerp:    the parent, its step followed by torch._foreach_lerp_(shadow, params, 1 - decay) -- what a user of the parent
                           would write (every parameter of this list has a gradient, so the shadow is the parameter list)
  (d) parent_step:         the parent, its step alone
  (e) device_copy:         this tree's process, a device copy of the bytes (a) moves: the step's 32 B per parameter and the average's
                           8 B, so the copy reads and writes 20 B per parameter
Conditions: (a) below (c) with disjoint [min, max] intervals ("device_time_win"; otherwise the feature is reported as no device-time
win, which says nothing about its correctness); (b)'s interval overlaps (d)'s (the template does not slow the existing path).
Part 2, `--train-repeats` times each, alternating, every run a process of its own: `train_dist --no-pretrain --bench --device-step`
without and with `--ema-decay 0.9998`; ms_per_step of each run.
Without a HIP device the tool refuses: a time is measured on the GPU or not at all.

    python tools/ema_bench.py [--repeats 50] [--parent-tree DIR] [--train-repeats 3] [--out profiles/ema_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# argv: tree, repeats, max_grad_norm, decay.  Prints one JSON line {arm: [us, ...]}.
CHILD = r'''
import argparse, json, sys
sys.path.insert(0, sys.argv[1])
import torch
from offsetguided_amd import _lib, models, optim
repeats, max_grad_norm, decay = int(sys.argv[2]), float(sys.argv[3]), float(sys.argv[4])
dev = torch.device('cuda:0')
p = argparse.ArgumentParser()
models.net_cli(p)
model, _ = models.model_factory(p.parse_args(['--no-pretrain']))
model = model.to(dev).to(memory_format=torch.channels_last)
params = [q for q in model.parameters() if q.requires_grad]
torch.manual_seed(0)
for q in params:
    q.grad = torch.randn_like(q, memory_format=torch.preserve_format) * 1e-3
n_params = sum(q.numel() for q in params)
opt = optim.DeviceAdam(params, lr=2.5e-4)
loss = torch.tensor(3.0, device=dev)
fused = hasattr(optim, 'ModelEma')
arms = {}
if fused:
    ema = optim.ModelEma(model, decay=decay, warmup=False)
    arms['step_ema'] = lambda: opt.step(loss=loss, max_grad_norm=max_grad_norm, ema=ema)
    arms['step'] = lambda: opt.step(loss=loss, max_grad_norm=max_grad_norm)
    src = torch.empty(5 * n_params, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    arms['device_copy'] = lambda: dst.copy_(src)
else:
    shadow = [q.detach().clone(memory_format=torch.preserve_format) for q in params]
    plain = [q.detach() for q in params]
    def step_lerp():
        opt.step(loss=loss, max_grad_norm=max_grad_norm)
        torch._foreach_lerp_(shadow, plain, 1.0 - decay)
    arms['parent_step_lerp'] = step_lerp
    arms['parent_step'] = lambda: opt.step(loss=loss, max_grad_norm=max_grad_norm)
stream = torch.cuda.current_stream(dev)
us = {n: [] for n in arms}
for rep in range(repeats + 3):
    for name, fn in arms.items():
        a, b = _lib.TimingEvent(), _lib.TimingEvent()
        a.record(stream)
        fn()
        b.record(stream)
        torch.cuda.synchronize()
        if rep >= 3:
            us[name].append(a.elapsed_time(b) * 1e3)
print(json.dumps({'us': us, 'tensors': len(params), 'parameters': n_params, 'table_chunks': opt._n_chunks,
                  'dropped_steps': int(opt.dropped_steps), 'lerp_rows': ema._n_rows if fused else None}))
'''


def spread(v):
    return [round(float(np.median(v)), 1), round(float(min(v)), 1), round(float(max(v)), 1)]


def child(tree, a, env):
    out = subprocess.run([sys.executable, '-c', CHILD, tree, str(a.repeats), str(a.max_grad_norm), str(a.decay)], cwd=tree, env=env,
                         capture_output=True, text=True, timeout=a.child_timeout)
    if out.returncode != 0:
        raise SystemExit(f'the timing child of {tree} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}')
    return json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])


def kernel_part(a):
    env = {k: v for k, v in os.environ.items() if k != 'OG_DECODER_LIB'}
    mine = child(ROOT, a, env)
    res = {k: mine[k] for k in ('tensors', 'parameters', 'table_chunks', 'dropped_steps', 'lerp_rows')}
    res.update(max_grad_norm=a.max_grad_norm, decay=a.decay, repeats=a.repeats, unit='us [median, min, max]')
    us = {n: spread(v) for n, v in mine['us'].items()}
    if a.parent_tree:
        tree = os.path.abspath(a.parent_tree)
        lib = os.path.join(tree, 'offsetguided_amd', 'libog_decoder.so')
        if not os.path.exists(lib):
            raise SystemExit(f'{lib} is missing: --parent-tree must be a BUILT checkout of the parent commit')
        us.update({n: spread(v) for n, v in child(tree, a, dict(env, OG_DECODER_LIB=lib))['us'].items()})
    res['us'] = us
    n = res['parameters']
    res['bytes_moved'] = {'step_ema': 40 * n, 'parent_step_lerp': 44 * n, 'step': 32 * n}
    res['step_ema_GBps'] = round(40 * n / us['step_ema'][0] / 1e3, 1)
    res['device_copy_GBps'] = round(40 * n / us['device_copy'][0] / 1e3, 1)
    res['ema_minus_step_median_us'] = round(us['step_ema'][0] - us['step'][0], 1)
    if 'parent_step_lerp' in us:
        res['device_time_win'] = bool(us['step_ema'][2] < us['parent_step_lerp'][1])
        res['step_overlaps_parent_step'] = bool(us['step'][1] <= us['parent_step'][2] and us['parent_step'][1] <= us['step'][2])
    return res


def train_part(a):
    runs = {'device_step': [], 'device_step_ema': []}
    lines = {}
    for _ in range(a.train_repeats):
        for name, extra in (('device_step', []), ('device_step_ema', ['--ema-decay', str(a.decay)])):
            cmd = [sys.executable, '-m', 'offsetguided_amd.train_dist', '--no-pretrain', '--bench', '--device-step', *extra]
            out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.train_timeout)
            if out.returncode != 0:
                raise SystemExit(f'{" ".join(cmd)} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}')
            line = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
            runs[name].append(line['ms_per_step'])
            lines[name] = line
    spread_ms = max(runs['device_step']) - min(runs['device_step'])
    delta = float(np.median(runs['device_step_ema']) - np.median(runs['device_step']))
    return {'command': f'train_dist --no-pretrain --bench --device-step [--ema-decay {a.decay}]', 'ms_per_step': runs,
            'device_step_spread_ms': round(spread_ms, 2), 'ema_minus_device_step_median_ms': round(delta, 2), 'last_line': lines}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--max-grad-norm', type=float, default=1.0)
    ap.add_argument('--decay', type=float, default=0.9998)
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--child-timeout', type=int, default=300)
    ap.add_argument('--train-repeats', type=int, default=3)
    ap.add_argument('--train-timeout', type=int, default=400)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('ema_bench needs a HIP device: a time is measured on the GPU or not at all')
    res = {'metric': 'ema_step', 'runs': 'one run', 'step': kernel_part(a)}
    if a.train_repeats > 0:
        res['train_bench'] = train_part(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
