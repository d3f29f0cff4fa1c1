"""fp16 training with the device-side loss scaler (offsetguided_amd.optim.DeviceLossScaler, csrc/optim.hip): one JSON line.

Part 1, HIP events after a warm-up, `--repeats` times, [median, min, max] in microseconds, both in this one process, alternating:
og_step_scale_f32 and og_step_scale_amp_f32 over the partials of the Hourglass-104 parameter list (`--partials`, 23 229 chunks).  Both
are one workgroup over the same doubles; no target is set.
Part 2, `--train-repeats` times each, alternating, every run a process of its own under its own time limit: `train_dist --no-pretrain
--bench --device-step` as it is (bf16 autocast) and with `--opt-level O1` (fp16 autocast, dynamic loss scaler); ms_per_step of each
run, the spread (max - min) of each, the final loss scale and the overflow count.  The first run that fails ends the tool.
Without a HIP device the tool refuses: a time is measured on the GPU or not at all.

    python tools/amp_bench.py [--repeats 50] [--train-repeats 3] [--out profiles/amp_bench.json]
"""
import argparse
import json
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def kernel_part(a):
    import torch
    from offsetguided_amd import _lib, optim
    dev = torch.device('cuda:0')
    lib = _lib.load()
    nbytes = lib.og_optim_workspace_bytes(a.partials)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    ws[16:].view(torch.float64).copy_(torch.rand(a.partials, dtype=torch.float64) * 1e6)
    scaler = optim.DeviceLossScaler(device=dev)
    loss = torch.tensor(3.0, device=dev)
    stream_t, stream = torch.cuda.current_stream(dev), _lib.stream_ptr(dev)

    def plain():
        _lib.check(lib.og_step_scale_f32(a.partials, _lib.ptr(loss), 1e8, a.max_grad_norm, _lib.ptr(ws), nbytes, stream), lib)

    def amp():
        _lib.check(lib.og_step_scale_amp_f32(a.partials, _lib.ptr(loss), 1e8, a.max_grad_norm, _lib.ptr(scaler._block), 1,
                                             scaler.scale_factor, scaler.scale_window, scaler.min_loss_scale, scaler.max_loss_scale,
                                             _lib.ptr(ws), nbytes, stream), lib)

    names = {'og_step_scale_f32': plain, 'og_step_scale_amp_f32': amp}
    us = {n: [] for n in names}
    for rep in range(a.repeats + 3):
        for n, fn in names.items():
            e0, e1 = _lib.TimingEvent(), _lib.TimingEvent()
            e0.record(stream_t)
            fn()
            e1.record(stream_t)
            torch.cuda.synchronize()
            if rep >= 3:
                us[n].append(e0.elapsed_time(e1) * 1e3)
    mmm = lambda v: [round(float(np.median(v)), 2), round(float(min(v)), 2), round(float(max(v)), 2)]   # noqa: E731
    return {'partials': a.partials, 'max_grad_norm': a.max_grad_norm, 'repeats': a.repeats, 'unit': 'us [median, min, max]',
            'us': {n: mmm(v) for n, v in us.items()},
            'amp_minus_plain_median_us': round(float(np.median(us['og_step_scale_amp_f32']) - np.median(us['og_step_scale_f32'])), 2),
            'scaler_after': scaler.state_dict()}


def train_part(a):
    runs = {'bf16': [], 'fp16_O1': []}
    lines = {}
    for _ in range(a.train_repeats):
        for name, extra in (('bf16', []), ('fp16_O1', ['--opt-level', 'O1'])):
            cmd = ['timeout', '-k', '10', str(a.train_timeout), sys.executable, '-m', 'offsetguided_amd.train_dist', '--no-pretrain',
                   '--bench', '--device-step', *extra]
            out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
            if out.returncode != 0:                    # nothing more is started on the device after a failure
                raise SystemExit(f'{" ".join(cmd)} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}')
            line = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
            runs[name].append(line['ms_per_step'])
            lines[name] = line
            print(f'{name}: {line["ms_per_step"]} ms per step', file=sys.stderr, flush=True)
    spread = {n: round(max(v) - min(v), 2) for n, v in runs.items()}
    return {'command': 'train_dist --no-pretrain --bench --device-step [--opt-level O1]', 'ms_per_step': runs, 'spread_ms': spread,
            'fp16_minus_bf16_median_ms': round(float(np.median(runs['fp16_O1']) - np.median(runs['bf16'])), 2),
            'final_loss_scale': lines['fp16_O1'].get('loss_scale'), 'overflow_steps': lines['fp16_O1'].get('overflow_steps'),
            'last_line': lines}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--partials', type=int, default=23229, help='chunk count of the Hourglass-104 parameter list')
    ap.add_argument('--max-grad-norm', type=float, default=math.inf)
    ap.add_argument('--train-repeats', type=int, default=3)
    ap.add_argument('--train-timeout', type=int, default=300)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('amp_bench needs a HIP device: a time is measured on the GPU or not at all')
    res = {'metric': 'amp_step_scale', 'runs': 'one run', 'scale_block': kernel_part(a)}
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
