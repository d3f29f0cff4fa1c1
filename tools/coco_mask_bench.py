"""mask_miss / mask_all on the device (data.device_masks: csrc/coco_mask.hip) on a val-like synthetic batch: one JSON line.

The batch: `--images` images (default 8) of 640 x 480, each with 8 persons of 2 polygons of 40 vertices and one crowd RLE.  Timed with
HIP events after a warm-up, `--repeats` times, [median, min, max] in microseconds:
  * og_coco_masks_u8's launches one by one (the descriptor's `stages`) and the whole call;
  * the floor of any implementation: a device memset of the output bytes and a device copy of them;
  * what the tree did before for the same batch: the same planes, built beforehand on the host, packed into a pinned buffer (host
    clock) and copied to the device (HIP events) -- DeviceAugment's staging of a mask_miss list.
Without a HIP device the tool refuses: a time is measured on the GPU or not at all.

    python tools/coco_mask_bench.py [--images 8] [--repeats 50] [--train-json FILE ...] [--out profiles/coco_mask_bench.json]
--train-json: JSON lines of `train_dist --bench --augment` runs (this tree, the parent commit) to record beside the figures.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def batch_records(n_images, h=480, w=640, persons=8, polygons=2, vertices=40, seed=0):
    """load_annotations-style records: persons as pairs of 40-gons round random centres, one crowd RLE of a few hundred runs."""
    rs = np.random.RandomState(seed)
    records = []
    for i in range(n_images):
        segs, crowd, nk, area = [], [], [], []
        for _ in range(persons):
            polys = []
            for _ in range(polygons):
                cx, cy, r = rs.uniform(0, w), rs.uniform(0, h), rs.uniform(15, 90)
                ang = np.sort(rs.uniform(0, 2 * np.pi, vertices))
                rad = r * rs.uniform(0.6, 1.0, vertices)
                xy = np.stack([cx + rad * np.cos(ang), cy + 1.6 * rad * np.sin(ang)], 1)
                polys.append([float(v) for v in np.round(xy, 2).reshape(-1)])
            segs.append(polys)
            crowd.append(0)
            nk.append(int(rs.randint(0, 17)))
            area.append(float(rs.uniform(500, 40000)))
        runs = rs.randint(1, 2 * h * w // 400, 399)
        runs = [int(v) for v in runs[:int(np.searchsorted(np.cumsum(runs), h * w))]]
        segs.append({'size': [h, w], 'counts': runs + [h * w - sum(runs)]})
        crowd.append(1)
        nk.append(0)
        area.append(5000.0)
        records.append({'height': h, 'width': w, 'image_id': i, 'segmentation': segs, 'iscrowd': np.array(crowd, np.uint8),
                        'num_keypoints': np.array(nk, np.int64), 'area': np.array(area, np.float64)})
    return records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=8)
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--train-json', nargs='*', default=[])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from offsetguided_amd import _lib, data
    from offsetguided_amd.data import masks
    if not torch.cuda.is_available():
        raise SystemExit('coco_mask_bench needs a HIP device: a time is measured on the GPU or not at all')
    dev = torch.device('cuda:0')
    lib = _lib.load()
    records = batch_records(a.images)
    tables = data.mask_tables(records)
    dm = data.device_masks(tables, dev)                         # warm-up: library load, workspace, pinned allocation
    host_planes = [dm.plane(i).cpu().numpy() for i in range(len(dm))]        # "built beforehand on the host"
    stream, st = torch.cuda.current_stream(dev), _lib.stream_ptr(dev)
    dev_tables = torch.from_numpy(tables.buffer).to(dev)
    miss = torch.empty(tables.out_bytes, dtype=torch.uint8, device=dev)
    every = torch.empty(tables.out_bytes, dtype=torch.uint8, device=dev)
    other = torch.empty(tables.out_bytes, dtype=torch.uint8, device=dev)
    pinned = torch.empty(tables.out_bytes, dtype=torch.uint8).pin_memory()
    pinned_np = pinned.numpy()

    def desc(stages):
        d = masks.descriptor(tables, tables.buffer.ctypes.data, dev_tables, miss, every)
        d.stages = stages
        return d
    descs = [desc(s) for s in (1, 2, 4, 8, 0)]
    ws_bytes = lib.og_coco_mask_workspace_bytes(C.byref(descs[-1]))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    names = ['zero', 'toggle', 'fill', 'compose', 'call', 'memset', 'copy', 'parent_h2d']
    us = {n: [] for n in names}
    pack_us = []
    for rep in range(a.repeats + 3):
        e = [_lib.TimingEvent() for _ in range(len(names) + 1)]
        e[0].record(stream)
        for j, d in enumerate(descs):
            _lib.check(lib.og_coco_masks_u8(C.byref(d), _lib.ptr(ws), ws_bytes, st), lib)
            e[j + 1].record(stream)
        other.zero_()
        e[6].record(stream)
        other.copy_(miss)
        e[7].record(stream)
        t0 = time.perf_counter()
        o = 0
        for p in host_planes:
            np.copyto(pinned_np[o:o + p.size].reshape(p.shape), p)
            o += p.size
        pack = (time.perf_counter() - t0) * 1e6
        e2 = [_lib.TimingEvent(), _lib.TimingEvent()]
        e2[0].record(stream)
        other.copy_(pinned, non_blocking=True)
        e2[1].record(stream)
        torch.cuda.synchronize()
        if rep >= 3:
            for j, n in enumerate(names[:7]):
                us[n].append(e[j].elapsed_time(e[j + 1]) * 1e3)
            us['parent_h2d'].append(e2[0].elapsed_time(e2[1]) * 1e3)
            pack_us.append(pack)
    same = all(np.array_equal(dm.plane(i).cpu().numpy(), p) for i, p in enumerate(host_planes))
    mmm = lambda v: [round(float(np.median(v)), 1), round(float(min(v)), 1), round(float(max(v)), 1)]   # noqa: E731
    res = {'metric': 'coco_mask', 'images': a.images, 'size': [480, 640], 'annotations': tables.counts[1], 'pieces': tables.counts[2],
           'vertices': tables.counts[3], 'rle_runs': tables.counts[4], 'output_bytes_per_mask': tables.out_bytes,
           'table_bytes': int(tables.buffer.nbytes), 'workspace_bytes': int(ws_bytes), 'repeats': a.repeats,
           'launch_us': {n: mmm(us[n]) for n in ('zero', 'toggle', 'fill', 'compose')}, 'call_us': mmm(us['call']),
           'floor_us': {'memset': mmm(us['memset']), 'device_copy': mmm(us['copy'])},
           'parent_us': {'pack_into_pinned_host_clock': mmm(pack_us), 'h2d_copy': mmm(us['parent_h2d'])},
           'call_over_parent_h2d': round(float(np.median(us['call']) / np.median(us['parent_h2d'])), 2),
           'planes_repeatable': bool(same), 'unit': 'us [median, min, max]',
           'train_bench': [json.loads(open(f).read().strip().splitlines()[-1]) | {'file': os.path.basename(f)} for f in a.train_json]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
