"""Refreshing an inference engine's weights in place (models.InferenceEngine.refresh, csrc/fold.hip) against building the engines
again, at bs8 640x640 fp16, two engines of one shape (run_images' two lanes): one JSON line.

All in this one process, `--repeats` times after one warm-up round, [median, min, max]; the module's weights are moved between rounds:
  (a) refresh_ms:        engine.refresh() on the host clock, its two device waits included (what a training loop pays per validation);
  (b) fold_us / launches_us: by HIP events, the og_fold_bn_w16 launch alone, and the span from that launch to the last re-pack launch
                         (the span holds the host's queueing gaps between ~300 small launches);
  (c) copy_us:           a device copy that reads and writes the same bytes as (b)'s launches (fold: 4 B read + 2 B written per weight;
                         a re-packed image: 2 B + 2 B per element);
  (d) rebuild_ms:        what refresh replaces: invalidate_engine_cache() + two new engines (fold by torch ops, packing, two warm-up
                         forwards and a graph capture each), on the host clock with a device wait at the end.
The one condition is (a) < (d).  Without a HIP device the tool refuses: a time is measured on the GPU or not at all.

    python tools/engine_refresh_bench.py [--repeats 5] [--out profiles/engine_refresh_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def spread(values):
    return [round(float(np.median(values)), 3), round(float(min(values)), 3), round(float(max(values)), 3)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--repeats', default=5, type=int)
    ap.add_argument('--batch', default=8, type=int)
    ap.add_argument('--size', default=640, type=int)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        sys.exit('engine_refresh_bench: no HIP device')
    from offsetguided_amd import _lib, models
    from offsetguided_amd.models import engine as eng_mod
    dev = torch.device('cuda:0')
    p = argparse.ArgumentParser()
    models.net_cli(p)
    model, _ = models.model_factory(p.parse_args(['--no-pretrain']))
    model = model.to(dev).to(memory_format=torch.channels_last)
    params = [q for q in model.parameters()]

    def move():      # an optimizer step's worth of change: every parameter differs afterwards
        with torch.no_grad():
            torch._foreach_mul_(params, 1.0009765625)

    def build():
        first = models.InferenceEngine(model, a.batch, a.size, a.size, device=dev)
        return first, models.InferenceEngine(model, a.batch, a.size, a.size, device=dev, like=first)

    x = torch.randn(a.batch, 3, a.size, a.size, device=dev)
    first, second = build()
    layers = first._layers
    n_weights = sum(c.w.numel() for c, _ in layers._convs())
    images = sum(t.numel() for c, _ in layers._convs() for t in (c.w_tiled, c.w_band, c.w_alt) if t is not None)
    images += layers.stem_w.numel() + layers.heads_w.numel() + (layers.heads_tiled[0].numel() if layers.heads_tiled else 0)
    moved = 6 * n_weights + 4 * images
    src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    stream = torch.cuda.current_stream(dev)
    out = {k: [] for k in ('refresh_ms', 'fold_us', 'launches_us', 'copy_us', 'rebuild_ms')}
    for rep in range(a.repeats + 1):
        move()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        first.refresh()
        refresh_ms = (time.perf_counter() - t0) * 1e3
        move()
        torch.cuda.synchronize(dev)
        events, end = [], _lib.TimingEvent()
        layers.refresh(model, events)
        end.record(stream)
        c0, c1 = _lib.TimingEvent(), _lib.TimingEvent()
        c0.record(stream)
        dst.copy_(src)
        c1.record(stream)
        torch.cuda.synchronize(dev)
        first.refresh()          # the bundle's cache entry follows the weights again
        second.forward_raw(x)
        move()
        del first, second
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        eng_mod.invalidate_engine_cache()
        first, second = build()
        torch.cuda.synchronize(dev)
        rebuild_ms = (time.perf_counter() - t0) * 1e3
        layers = first._layers
        if rep:      # the first round warms allocator, pinned slot and table
            out['refresh_ms'].append(refresh_ms)
            out['fold_us'].append(events[0][0].elapsed_time(events[0][1]) * 1e3)
            out['launches_us'].append(events[0][0].elapsed_time(end) * 1e3)
            out['copy_us'].append(c0.elapsed_time(c1) * 1e3)
            out['rebuild_ms'].append(rebuild_ms)
    res = {'what': f'engine weight refresh in place vs rebuild, bs{a.batch} {a.size}x{a.size} fp16, two engines of one shape',
           'repeats': a.repeats, 'weights': n_weights, 'repacked_image_elements': images, 'bytes_moved': moved,
           **{k: spread(v) for k, v in out.items()}}
    res['refresh_over_rebuild'] = round(res['refresh_ms'][0] / res['rebuild_ms'][0], 4)
    res['launches_over_copy'] = round(res['launches_us'][0] / res['copy_us'][0], 3)
    res['fold_over_copy_of_its_bytes'] = round(res['fold_us'][0] / (res['copy_us'][0] * 6 * n_weights / moved), 3)
    res['refresh_below_rebuild'] = bool(res['refresh_ms'][0] < res['rebuild_ms'][0])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
