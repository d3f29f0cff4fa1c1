"""The device-side optimizer step (offsetguided_amd.optim, csrc/optim.hip) on the Hourglass-104 parameter list: one JSON line.

Part 1, HIP events after a warm-up, `--repeats` times, [median, min, max] in microseconds, all in this one process:
  * DeviceAdam.step(loss=..., max_grad_norm=...) -- sum of squares, scale block and update, the clip and the loss guard on;
  * what it replaces: torch.nn.utils.clip_grad_norm_(foreach=True) and torch.optim.Adam(fused=True).step() on a copy of the same
    parameters and gradients (in training order: clip, then step);
  * the bandwidth floor: a device copy that moves the same bytes.  The update reads p, g, m, v and writes p, m, v (7 x 4 B per
    parameter), the norm reads g (4 B): 32 B per parameter, so the copy reads and writes 16 B per parameter.
Part 2, `--train-repeats` times each, alternating, every run a process of its own: `train_dist --no-pretrain --bench` without and
with `--device-step`; ms_per_step of each run, and the spread (max - min) of the flagless runs.
Without a HIP device the tool refuses: a time is measured on the GPU or not at all.

    python tools/optim_bench.py [--repeats 20] [--train-repeats 3] [--out profiles/optim_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def kernel_part(a):
    import torch
    from offsetguided_amd import _lib, models, optim
    dev = torch.device('cuda:0')
    p = argparse.ArgumentParser()
    models.net_cli(p)
    model, _ = models.model_factory(p.parse_args(['--no-pretrain']))
    model = model.to(dev).to(memory_format=torch.channels_last)
    ours = [q for q in model.parameters() if q.requires_grad]
    theirs = [torch.nn.Parameter(q.detach().clone(memory_format=torch.preserve_format)) for q in ours]
    torch.manual_seed(0)
    for q, t in zip(ours, theirs):
        q.grad = torch.randn_like(q, memory_format=torch.preserve_format) * 1e-3
        t.grad = q.grad.clone(memory_format=torch.preserve_format)
    n_params = sum(q.numel() for q in ours)
    d_opt = optim.DeviceAdam(ours, lr=2.5e-4)
    t_opt = torch.optim.Adam(theirs, lr=2.5e-4, fused=True)
    loss = torch.tensor(3.0, device=dev)
    src = torch.empty(4 * n_params, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    stream = torch.cuda.current_stream(dev)
    names = ['device_step', 'torch_clip_then_fused_adam', 'device_copy']
    us = {n: [] for n in names}
    for rep in range(a.repeats + 3):
        e = [_lib.TimingEvent() for _ in range(4)]
        e[0].record(stream)
        d_opt.step(loss=loss, max_grad_norm=a.max_grad_norm)
        e[1].record(stream)
        torch.nn.utils.clip_grad_norm_(theirs, a.max_grad_norm, foreach=True)
        t_opt.step()
        e[2].record(stream)
        dst.copy_(src)
        e[3].record(stream)
        torch.cuda.synchronize()
        if rep >= 3:
            for j, n in enumerate(names):
                us[n].append(e[j].elapsed_time(e[j + 1]) * 1e3)
    mmm = lambda v: [round(float(np.median(v)), 1), round(float(min(v)), 1), round(float(max(v)), 1)]   # noqa: E731
    med = {n: float(np.median(us[n])) for n in names}
    return {'tensors': len(ours), 'parameters': n_params, 'table_chunks': d_opt._n_chunks, 'max_grad_norm': a.max_grad_norm,
            'grad_norm': round(float(d_opt.last_grad_norm), 6), 'scale': round(float(d_opt.last_scale), 6),
            'dropped_steps': int(d_opt.dropped_steps), 'repeats': a.repeats, 'unit': 'us [median, min, max]',
            'us': {n: mmm(us[n]) for n in names}, 'bytes_moved': 32 * n_params,
            'device_step_GBps': round(32 * n_params / med['device_step'] / 1e3, 1),
            'device_copy_GBps': round(32 * n_params / med['device_copy'] / 1e3, 1),
            'device_step_not_above_torch_pair': bool(med['device_step'] <= med['torch_clip_then_fused_adam'])}


def train_part(a):
    runs = {'flagless': [], 'device_step': []}
    lines = {}
    for _ in range(a.train_repeats):
        for name, extra in (('flagless', []), ('device_step', ['--device-step'])):
            cmd = [sys.executable, '-m', 'offsetguided_amd.train_dist', '--no-pretrain', '--bench', *extra]
            out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.train_timeout)
            if out.returncode != 0:
                raise SystemExit(f'{" ".join(cmd)} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}')
            line = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
            runs[name].append(line['ms_per_step'])
            lines[name] = line
    spread = max(runs['flagless']) - min(runs['flagless'])
    delta = float(np.median(runs['device_step']) - np.median(runs['flagless']))
    return {'command': 'train_dist --no-pretrain --bench [--device-step]', 'ms_per_step': runs,
            'flagless_spread_ms': round(spread, 2), 'device_minus_flagless_median_ms': round(delta, 2),
            'device_step_not_above_flagless_by_more_than_its_spread': bool(delta <= spread),
            'last_line': lines}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--max-grad-norm', type=float, default=1.0)
    ap.add_argument('--train-repeats', type=int, default=3)
    ap.add_argument('--train-timeout', type=int, default=400)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('optim_bench needs a HIP device: a time is measured on the GPU or not at all')
    res = {'metric': 'optim_step', 'runs': 'one run', 'step': kernel_part(a)}
    torch.cuda.empty_cache()
    if a.train_repeats > 0:
        res['train_bench'] = train_part(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
