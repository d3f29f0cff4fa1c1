"""numpy restatement of og_coco_masks_u8 (include/og_decoder.h) with straight loops, written in the SORT-AND-MERGE RUN-LENGTH form
(collect the toggle positions, append h w, sort, take differences, merge zero-length runs, paint the runs) -- the kernels use the XOR
form, so the two formulations check each other --, mask_mask restated with boolean planes in list order, and the directed cases.
Bit parity with pycocotools is not claimed: what is pinned is the header's text and this file."""
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'coco_tiny.json')


def polygon_positions(poly, h, w):
    """Toggle positions x h + y of one polygon [x0, y0, x1, y1, ...] (steps 1-3 of the header), in emission order."""
    k = len(poly) // 2
    X = [int(5 * float(poly[2 * j]) + .5) for j in range(k)]
    Y = [int(5 * float(poly[2 * j + 1]) + .5) for j in range(k)]
    X.append(X[0])
    Y.append(Y[0])
    us, vs = [], []
    for j in range(k):
        xs, xe, ys, ye = X[j], X[j + 1], Y[j], Y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx == 0 and dy == 0:
            us.append(xs)
            vs.append(ys)
            continue
        if dx >= dy:
            s = float(ye - ys) / dx
            for d in range(dx + 1):
                t = dx - d if flip else d
                us.append(t + xs)
                vs.append(int(ys + s * t + .5))
        else:
            s = float(xe - xs) / dy
            for d in range(dy + 1):
                t = dy - d if flip else d
                vs.append(t + ys)
                us.append(int(xs + s * t + .5))
    out = []
    for j in range(1, len(us)):
        if us[j] == us[j - 1]:
            continue
        xd = float(us[j] if us[j] < us[j - 1] else us[j] - 1)
        xd = (xd + .5) / 5 - .5
        if math.floor(xd) != xd or xd < 0 or xd > w - 1:
            continue
        yd = float(vs[j] if vs[j] < vs[j - 1] else vs[j - 1])
        yd = (yd + .5) / 5 - .5
        yd = 0.0 if yd < 0 else (float(h) if yd > h else yd)
        out.append(int(xd) * h + int(math.ceil(yd)))
    return out


def runs_from_positions(positions, h, w):
    """The run lengths maskApi's rleFrPoly ends with: positions + [h w], sorted, differences, zero-length runs merged away (the run
    before and the run after a zero-length run are one run; a leading zero-length run stays: the first run is a 0-run)."""
    a = sorted(list(positions) + [h * w])
    diffs, prev = [], 0
    for t in a:
        diffs.append(t - prev)
        prev = t
    runs = [diffs[0]]
    j = 1
    while j < len(diffs):
        if diffs[j] > 0:
            runs.append(diffs[j])
            j += 1
        else:
            j += 1
            if j < len(diffs):
                runs[-1] += diffs[j]
                j += 1
    return runs


def paint_runs(runs, h, w):
    """Column-major runs, the first a 0-run -> bool (h, w).  Runs beyond h w are cut."""
    flat = np.zeros(h * w, bool)
    at, value = 0, False
    for r in runs:
        flat[at:min(at + r, h * w)] = value
        at += r
        value = not value
    return flat.reshape(w, h).T.copy()


def plane_runs(positions, h, w):
    return paint_runs(runs_from_positions(positions, h, w), h, w)


def plane_xor(positions, h, w):
    """The kernels' formulation: bit a = XOR of the toggles at positions <= a."""
    toggles = np.zeros(h * w + 1, np.int64)
    for p in positions:
        toggles[min(p, h * w)] += 1
    return ((np.cumsum(toggles)[:h * w] & 1) == 1).reshape(w, h).T.copy()


def string_to_runs(s):
    runs, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = (c & 0x20) != 0
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(runs) > 2:
            x += runs[-2]
        runs.append(x)
    return runs


def runs_to_string(runs):
    """maskApi's rleToString (the inverse of string_to_runs)."""
    out = []
    for i, x in enumerate(runs):
        if i > 2:
            x -= runs[i - 2]
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
    return ''.join(out)


def annotation_mask(seg, h, w):
    """bool (h, w): the union of the polygons' planes, or the RLE's plane."""
    if isinstance(seg, dict):
        counts = seg['counts']
        return paint_runs(string_to_runs(counts) if isinstance(counts, str) else list(counts), h, w)
    m = np.zeros((h, w), bool)
    for poly in seg:
        m |= plane_runs(polygon_positions(poly, h, w), h, w)
    return m


def mask_mask(record):
    """(mask_miss, mask_all) uint8 (h, w) of one image's record (data.load_annotations' keys): CocoKeypoints.mask_mask as set algebra,
    every crowd annotation adding its own term."""
    h, w = record['height'], record['width']
    persons, miss, crowd = (np.zeros((h, w), bool) for _ in range(3))
    for j in range(len(record['area'])):
        m = annotation_mask(record['segmentation'][j], h, w)
        if record['iscrowd'][j] == 1:
            crowd |= m & ~persons
            continue
        persons |= m
        if record['num_keypoints'][j] <= 0 or record['area'][j] <= 32 * 32:
            miss |= m
    return (~(miss | crowd)).astype(np.uint8) * 255, (persons | crowd).astype(np.uint8) * 255


def record(h, w, anns, image_id=0):
    """A load_annotations-style record from [(segmentation, iscrowd, num_keypoints, area)]."""
    return {'height': h, 'width': w, 'image_id': image_id, 'segmentation': [a[0] for a in anns],
            'iscrowd': np.array([a[1] for a in anns], np.uint8), 'num_keypoints': np.array([a[2] for a in anns], np.int64),
            'area': np.array([a[3] for a in anns], np.float64)}


def rect(x0, y0, wd, ht):
    return [x0, y0, x0 + wd, y0, x0 + wd, y0 + ht, x0, y0 + ht]


RECT_AREAS = [(rect(3, 5, 4, 4), 16), (rect(10, 2, 5, 6), 30), (rect(2.5, 3.5, 5, 4), 20)]

# (name, h, w, polygons of ONE annotation): the images are 29 x 37, 48 x 64, 33 x 31 and 1 x 1 -- nothing a multiple of 32
POLYGON_CASES = [
    ('rect 4x4', 29, 37, [rect(3, 5, 4, 4)]),
    ('rect 5x6', 29, 37, [rect(10, 2, 5, 6)]),
    ('rect half-integer 5x4', 29, 37, [rect(2.5, 3.5, 5, 4)]),
    ('triangle steep + shallow', 48, 64, [[5, 40, 9, 3, 60, 30]]),
    ('triangle, other winding', 48, 64, [[5, 40, 60, 30, 9, 3]]),
    ('leaves on the left', 33, 31, [[-6, 4, 9, 8, -3.5, 20]]),
    ('leaves on the right', 33, 31, [[25, 4, 40.5, 9, 22, 21]]),
    ('leaves at the top', 33, 31, [[4, -7, 20, -2.5, 12, 14]]),
    ('leaves at the bottom', 33, 31, [[4, 25, 22.5, 27, 12, 41]]),
    ('wholly outside', 33, 31, [[40, 40, 50, 41, 45, 60]]),
    ('clamped to y = h: a toggle on the next column', 29, 37, [[4, 20, 15, 20, 15, 35, 4, 35]]),
    ('clamped in the last column: a toggle at h w', 29, 37, [[30, 10, 40, 10, 40, 35, 30, 35]]),
    ('repeated vertex', 48, 64, [[10, 10, 30, 12, 30, 12, 22, 40, 10, 10]]),
    ('one vertex', 29, 37, [[7, 7]]),
    ('two vertices', 29, 37, [[3, 3, 20, 15]]),
    ('two overlapping polygons: a union', 48, 64, [rect(8, 8, 20, 20), rect(18, 18, 25, 22)]),
    ('1 x 1 covered', 1, 1, [rect(-1, -1, 3, 3)]),
    ('1 x 1 missed', 1, 1, [rect(2, 2, 3, 3)]),
]


def polygon_case_records():
    return [record(h, w, [(polys, 0, 5, 4000.0)], image_id=i) for i, (_, h, w, polys) in enumerate(POLYGON_CASES)]


def random_polygon_records(n=300, seed=20240613):
    """n seeded random polygons, one annotation each: 3-12 vertices, coordinates in [-0.2, 1.2] of the image, 0-2 decimals."""
    rs = np.random.RandomState(seed)
    sizes = [(29, 37), (48, 64), (33, 31), (1, 1)]
    out = []
    for i in range(n):
        h, w = sizes[rs.randint(len(sizes))] if i % 25 else (1, 1)
        k, dec = rs.randint(3, 13), rs.randint(0, 3)
        xs = np.round(rs.uniform(-0.2, 1.2, k) * w, dec)
        ys = np.round(rs.uniform(-0.2, 1.2, k) * h, dec)
        poly = [float(v) for xy in zip(xs, ys) for v in xy]
        out.append(record(h, w, [([poly], 0, 5, 4000.0)], image_id=i))
    return out


def tiny_records():
    """The records of tests/golden/coco_tiny.json through the package's own loader, in file order."""
    from offsetguided_amd import data
    return list(data.load_annotations(GOLDEN).values())


def tiny_json():
    with open(GOLDEN) as f:
        return json.load(f)


_reference = {}


def reference_masks(key, records):
    """[(mask_miss, mask_all)] of the records, computed once per key and shared between the tests (read-only arrays)."""
    if key not in _reference:
        out = [mask_mask(r) for r in records]
        for a, b in out:
            a.setflags(write=False)
            b.setflags(write=False)
        _reference[key] = out
    return _reference[key]
