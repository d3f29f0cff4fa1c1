"""What the range report costs (include/og_decoder.h "range report", csrc/range.hip, InferenceEngine(probe=True)): one JSON line.

By HIP events, `--repeats` times after a warm-up, [median, min, max]:
  (a) probe_us / probe_copy_us:   og_range_probe on a bs8 160 x 160 x 256 fp16 activation, beside a device copy of the same tensor
                                  (the probe only reads: half the copy's traffic);
  (b) stats_us / stats_copy_us:   og_range_stats over the Hourglass-104 weight table (every _Conv.w of the bundle, one launch),
                                  beside a device copy of the same bytes;
  (c) replay_ms / replay_probe_ms: a graph replay of the bs8 640 x 640 fp16 engine without and with probe=True;
  (d) parent_replay_ms:           with --parent-tree DIR (a built checkout of the parent commit), the same replay of ITS engine, timed
                                  in a child process of this run: the non-probing replay must stay within its run-to-run spread.
Without a HIP device the tool refuses: a time is measured on the GPU or not at all.

    python tools/range_report_bench.py [--repeats 20] [--parent-tree DIR] [--out profiles/range_report_bench.json]
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

# the replay timing alone, runnable against any checkout of the project (argv: tree, batch, size, repeats): one JSON list of ms
REPLAY = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
import argparse, torch
from offsetguided_amd import _lib, models
batch, size, repeats = (int(v) for v in sys.argv[2:5])
dev = torch.device('cuda:0')
p = argparse.ArgumentParser()
models.net_cli(p)
torch.manual_seed(0)
model, _ = models.model_factory(p.parse_args(['--no-pretrain']))
engine = models.InferenceEngine(model, batch, size, size, device=dev)
x = torch.randn(batch, 3, size, size, device=dev)
stream, times = torch.cuda.current_stream(dev), []
for rep in range(repeats + 3):
    a, b = _lib.TimingEvent(), _lib.TimingEvent()
    a.record(stream)
    engine.forward_raw(x)
    b.record(stream)
    torch.cuda.synchronize(dev)
    if rep >= 3:
        times.append(a.elapsed_time(b))
print(json.dumps(times))
'''


def spread(values):
    return [round(float(np.median(values)), 3), round(float(min(values)), 3), round(float(max(values)), 3)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--repeats', default=20, type=int)
    ap.add_argument('--batch', default=8, type=int)
    ap.add_argument('--size', default=640, type=int)
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        sys.exit('range_report_bench: no HIP device')
    from offsetguided_amd import _lib, models
    from offsetguided_amd.models import range_report
    dev = torch.device('cuda:0')
    stream = torch.cuda.current_stream(dev)

    def timed(fn, repeats=a.repeats, warm=3):
        out = []
        for rep in range(repeats + warm):
            e0, e1 = _lib.TimingEvent(), _lib.TimingEvent()
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize(dev)
            if rep >= warm:
                out.append(e0.elapsed_time(e1))
        return out

    res = {'what': f'range report: probe, weight table and probing replay, bs{a.batch} {a.size}x{a.size} fp16', 'repeats': a.repeats}
    if a.parent_tree:       # first, while this process holds no engine of its own
        child = subprocess.run([sys.executable, '-c', REPLAY, os.path.abspath(a.parent_tree), str(a.batch), str(a.size), str(a.repeats)],
                               check=True, capture_output=True, text=True, env={k: v for k, v in os.environ.items() if k != 'OG_DECODER_LIB'})
        res['parent_replay_ms'] = spread(json.loads(child.stdout.strip().splitlines()[-1]))
    # (a) one activation of the 160-wide level
    act = torch.randn(a.batch, 256, a.size // 4, a.size // 4, device=dev).to(torch.float16).contiguous(memory_format=torch.channels_last)
    row = torch.zeros((1, 9), dtype=torch.int64, device=dev)
    dst = torch.empty_like(act)
    res['probe_elements'] = act.numel()
    res['probe_us'] = spread([t * 1e3 for t in timed(lambda: range_report.probe(act, torch.float16, row, 0))])
    res['probe_copy_us'] = spread([t * 1e3 for t in timed(lambda: dst.copy_(act))])
    res['probe_gb_per_s'] = round(act.numel() * 2 / res['probe_us'][0] / 1e3, 1)
    del act, dst
    # (b), (c) the model
    p = argparse.ArgumentParser()
    models.net_cli(p)
    torch.manual_seed(0)
    model, _ = models.model_factory(p.parse_args(['--no-pretrain']))
    plain = models.InferenceEngine(model, a.batch, a.size, a.size, device=dev)
    probing = models.InferenceEngine(model, a.batch, a.size, a.size, device=dev, like=plain, probe=True)
    weights = [c.w for c, _ in plain._layers._convs()]
    stats = torch.zeros((len(weights), 9), dtype=torch.int64, device=dev)
    flat = torch.empty(sum(w.numel() for w in weights), dtype=torch.float16, device=dev)
    flat_dst = torch.empty_like(flat)
    res['weight_tensors'], res['weights'] = len(weights), flat.numel()
    res['stats_us'] = spread([t * 1e3 for t in timed(lambda: range_report.range_stats(weights, torch.float16, out=stats))])
    res['stats_copy_us'] = spread([t * 1e3 for t in timed(lambda: flat_dst.copy_(flat))])
    del flat, flat_dst
    x = torch.randn(a.batch, 3, a.size, a.size, device=dev)
    res['replay_ms'] = spread(timed(lambda: plain.forward_raw(x)))
    res['replay_probe_ms'] = spread(timed(lambda: probing.forward_raw(x)))
    res['probe_points'] = int(probing.probe_stats.shape[0])
    res['probing_over_plain'] = round(res['replay_probe_ms'][0] / res['replay_ms'][0], 3)
    if 'parent_replay_ms' in res:
        lo, hi = res['parent_replay_ms'][1:]
        res['replay_within_parent_spread'] = bool(res['replay_ms'][0] <= hi)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
