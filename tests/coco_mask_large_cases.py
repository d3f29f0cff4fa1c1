"""Cases for og_coco_masks_u8 beyond one chunk of a plane: coco_fill_kernel walks a piece's bit plane 256 words (8192 pixels) at a
time and carries the running parity from chunk to chunk, coco_toggle_kernel's lanes take a second pass from the 257th cumulative sum
of an RLE and the 257th point of a polygon edge, and coco_compose_kernel's grid is sized by the largest image of the batch.  Plain data
and small builders, no GPU; the expected planes come from coco_mask_common (mask_mask / paint_runs / plane_runs) alone.
A record carries a 'name' beside load_annotations' keys; GROUPS maps a group's name to its builder."""
import functools

import numpy as np

import coco_mask_common as cm

CHUNK_WORDS = 256                 # coco_fill_kernel: one word per thread and turn
CHUNK = 32 * CHUNK_WORDS          # 8192 pixels
LANES = 256                       # coco_toggle_kernel's stride over cumulative sums and over an edge's points


def chunks_of(hw):
    return ((hw + 31) // 32 + CHUNK_WORDS - 1) // CHUNK_WORDS


def rle(h, w, runs):
    runs = [int(r) for r in runs]
    assert sum(runs) == h * w and min(runs) >= 0, (h, w, sum(runs))
    return {'size': [h, w], 'counts': runs}


def toggles_rle(h, w, positions):
    """The uncompressed RLE whose cumulative sums are `positions` (ascending; a repeat is a zero-length run) and then h w."""
    runs, prev = [], 0
    for p in positions:
        runs.append(p - prev)
        prev = p
    return rle(h, w, runs + [h * w - prev])


def named(name, h, w, anns, image_id=0):
    r = cm.record(h, w, anns, image_id=image_id)
    r['name'] = f'{name} ({h} x {w})'
    return r


def one_piece(name, h, w, seg, image_id=0):
    """One annotation of one piece: an RLE as a crowd, a polygon as a person without keypoints -- either way mask_all is the piece's
    plane and mask_miss its complement, so both outputs show every bit of it."""
    crowd = isinstance(seg, dict)
    return named(name, h, w, [(seg if crowd else [seg], int(crowd), 0, 4000.0)], image_id)


def pieces(record):
    """[(kind, piece)] of a record in table order: ('rle', run lengths) or ('polygon', [x0, y0, ...])."""
    out = []
    for seg in record['segmentation']:
        if isinstance(seg, dict):
            counts = seg['counts']
            out.append(('rle', cm.string_to_runs(counts) if isinstance(counts, str) else list(counts)))
        else:
            out.extend(('polygon', poly) for poly in seg)
    return out


def piece_positions(kind, piece, h, w):
    """The toggle positions the kernels XOR into the piece's plane (those at h w have no effect)."""
    return [int(c) for c in np.cumsum(piece)] if kind == 'rle' else cm.polygon_positions(piece, h, w)


def tagged_positions(poly, h, w):
    """cm.polygon_positions with the kernel's loop indices: ([(position, edge j, point i on that edge)], [(n, along_x, flip)] per
    edge), the same integer arithmetic.  Point i of edge j is what lane i % 256 handles in pass i // 256 of coco_toggle_kernel."""
    k = len(poly) // 2
    X = [int(5 * float(poly[2 * j]) + .5) for j in range(k)]
    Y = [int(5 * float(poly[2 * j + 1]) + .5) for j in range(k)]
    X.append(X[0])
    Y.append(Y[0])
    pts, edges = [], []
    for j in range(k):
        xs, xe, ys, ye = X[j], X[j + 1], Y[j], Y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        n = max(dx, dy)
        edges.append((n, dx >= dy, flip))
        s = 0.0 if n == 0 else (float(ye - ys) / dx if dx >= dy else float(xe - xs) / dy)
        for i in range(n + 1):
            t = n - i if flip else i
            pts.append((t + xs, int(ys + s * t + .5), j, i) if dx >= dy else (int(xs + s * t + .5), t + ys, j, i))
    out = []
    for a in range(1, len(pts)):
        (u, v, j, i), (u0, v0) = pts[a], pts[a - 1][:2]
        if u == u0:
            continue
        xd = (float(u if u < u0 else u - 1) + .5) / 5 - .5
        if np.floor(xd) != xd or xd < 0 or xd > w - 1:
            continue
        yd = (float(min(v, v0)) + .5) / 5 - .5
        yd = 0.0 if yd < 0 else (float(h) if yd > h else yd)
        out.append((int(xd) * h + int(np.ceil(yd)), j, i))
    return out, edges


def random_polygon(rs, h, w, k, dec):
    xs = np.round(rs.uniform(-0.2, 1.2, k) * w, dec)
    ys = np.round(rs.uniform(-0.2, 1.2, k) * h, dec)
    return [float(v) for xy in zip(xs, ys) for v in xy]


def random_runs(rs, hw, n):
    """n run lengths >= 1 that sum to hw."""
    cuts = np.sort(rs.choice(hw - 1, n - 1, replace=False) + 1)
    return [int(v) for v in np.diff(np.concatenate([[0], cuts, [hw]]))]


# ---- chunk boundaries of the fill: (h, w, chunks of a plane) ----
CHUNK_BOUNDARY_SIZES = [
    (96, 85, 1),         # 8160: 255 words
    (8191, 1, 1),        # 8191: one chunk less one pixel, the last word short; one column
    (1, 8191, 1),        # the same plane, 8191 columns of one pixel
    (64, 128, 1),        # 8192: exactly one chunk
    (3, 2731, 2),        # 8193: a second chunk of one word with one bit
    (32, 257, 2),        # 8224: 257 words
    (128, 128, 2),       # 16384: two full chunks
    (145, 113, 3),       # 16385: two full chunks plus one bit
    (131, 97, 2),        # 12707: a partial last chunk, hw no multiple of 32
]


@functools.lru_cache(None)
def chunk_boundary_records():
    """Per size: a random person, a band without keypoints across every column, a crowd RLE, a random person after the crowd."""
    out = []
    for i, (h, w, _) in enumerate(CHUNK_BOUNDARY_SIZES):
        rs = np.random.RandomState(8160 + i)
        band = cm.rect(-1, round(0.25 * h, 1), w + 2, round(0.5 * h, 1))
        crowd = rle(h, w, random_runs(rs, h * w, 38))
        out.append(named('chunk boundary, hw = %d' % (h * w), h, w,
                         [([random_polygon(rs, h, w, 7, 1)], 0, 5, 4000.0), ([band], 0, 0, 4000.0), (crowd, 1, 0, 900.0),
                          ([random_polygon(rs, h, w, 5, 2)], 0, 3, 2000.0)], image_id=i))
    return out


# ---- directed toggles by RLE ----
DIRECTED_SIZES = [(145, 113), (160, 200)]          # 16385 pixels: 3 chunks, the last of one bit; 32000: 4 chunks, the last of 232 words


@functools.lru_cache(None)
def directed_toggle_records():
    out = []
    for h, w in DIRECTED_SIZES:
        hw = h * w
        # one toggle: everything after it is filled.  2048 pixels are one wave's 64 words; 32 * 200 lies in wave 3 of chunk 0,
        # CHUNK + 32 * 250 in wave 3 of chunk 1
        for p in (0, 2047, 2048, 4095, 4096, 6143, 6144, 8191, 8192, hw - 1, 32 * 200, CHUNK + 32 * 250):
            out.append(one_piece('toggle at %d' % p, h, w, toggles_rle(h, w, [p])))
        # open in one chunk, close two chunks later: the carry passes a whole chunk of toggle-free words
        pairs = [(100, 2 * CHUNK), (8191, 2 * CHUNK)]
        if hw > 3 * CHUNK:
            pairs += [(4097, 2 * CHUNK + 37), (CHUNK + 5000, 3 * CHUNK + 4000), (31, hw - 1)]
        for a, b in pairs:
            out.append(one_piece('open at %d, close at %d' % (a, b), h, w, toggles_rle(h, w, [a, b])))
        out.append(one_piece('a toggle in each wave of two chunks', h, w,
                             toggles_rle(h, w, [1000, 3000, 5000, 7000, CHUNK + 1000, CHUNK + 3000, CHUNK + 5000, CHUNK + 7001])))
        # zero-length runs stack two toggles on 8191 (nothing) and three on 8192 (one): 4096 pixels from 8192 on
        out.append(one_piece('stacked toggles', h, w, rle(h, w, [8191, 0, 1, 0, 0, 4096, hw - 8192 - 4096])))
    for i, r in enumerate(out):
        r['image_id'] = i
    return out


# ---- the whole image covered: one toggle at position 0, every chunk depends on the carry alone ----
WHOLE_SIZES = [(131, 97), (145, 113), (160, 200)]


@functools.lru_cache(None)
def whole_image_records():
    return [one_piece('whole image covered', h, w, cm.rect(-1, -1, w + 2, h + 2), image_id=i) for i, (h, w) in enumerate(WHOLE_SIZES)]


# ---- long RLEs: the lanes' second, third and fourth pass over the cumulative sums ----
LONG_RLE_RUNS = [256, 257, 258, 513, 1000]          # the last cumulative sum is h w: the 257th is the first to set a toggle


def compressed_rle_runs(h=480, w=640):
    """303 runs for the compressed string: most below 300, three above 2^15 and the last above 2^16, so that rleToString's deltas
    to the count two back take four characters and both signs."""
    rs = np.random.RandomState(307200)
    runs = [int(v) for v in rs.randint(1, 300, 299)]
    for at, v in ((10, 40000), (11, 70000), (150, 33000)):
        runs.insert(at, v)
    rest = h * w - sum(runs)
    assert rest > 1 << 16
    return runs + [rest]


@functools.lru_cache(None)
def long_rle_records():
    out = []
    for i, n in enumerate(LONG_RLE_RUNS):
        out.append(one_piece('RLE of %d runs' % n, 160, 200, rle(160, 200, random_runs(np.random.RandomState(n), 32000, n)), image_id=i))
    runs = compressed_rle_runs()
    out.append(one_piece('compressed RLE of %d runs' % len(runs), 480, 640, {'size': [480, 640], 'counts': cm.runs_to_string(runs)},
                         image_id=len(out)))
    return out


# ---- long edges on the x5 grid of a 128 x 160 image (640 x 800 grid points) ----
def grid(g):
    """A coordinate whose grid value (int)(5 p + .5) is g: the sum lands a quarter inside g's cell, on the side the truncation keeps."""
    return (g - .25) / 5 if g >= 0 else (g - .75) / 5


# (name, n, along_x, triangle A B C in grid units): the subject is edge A -> B of n + 1 points (flip = False), and edge B -> A of the
# other winding [B, A, C] (flip = True).  A toggle falls where the grid x is 2 modulo 5, so xs and dx are chosen modulo 5 such that,
# for n >= 256, a point of the second pass sets a toggle in either winding -- for n = 256 that is the single point 256: the end B one
# way, the start A the other way (tests/test_coco_mask_large_cpu.py checks that).  n = 255 is the longest edge of a single pass, and
# those two triangles have no longer edge.
LONG_EDGES = [
    ('shallow 256 points', 255, True, [(102, 40), (357, 137), (229, 287)]),
    ('shallow 257 points', 256, True, [(302, 300), (558, 397), (430, 547)]),
    ('shallow 512 points, leaves left and top', 511, True, [(-98, -60), (413, 37), (157, 187)]),
    ('shallow 513 points, leaves right and bottom', 512, True, [(402, 500), (914, 597), (658, 747)]),
    ('steep 256 points', 255, False, [(103, 50), (303, 305), (303, 100)]),
    ('steep 257 points', 256, False, [(402, 300), (603, 556), (753, 428)]),
    ('steep 512 points, leaves left and top', 511, False, [(-70, -80), (130, 431), (280, 175)]),
    ('steep 513 points, leaves right and bottom', 512, False, [(680, 220), (880, 732), (1030, 476)]),
]
LONG_EDGE_SIZE = (128, 160)


def long_edge_polygons():
    """[(name, n, along_x, flip, polygon)]: every LONG_EDGES triangle in both windings."""
    out = []
    for name, n, along_x, (a, b, c) in LONG_EDGES:
        for flip, order in ((False, (a, b, c)), (True, (b, a, c))):
            out.append((name + (', reversed' if flip else ''), n, along_x, flip, [grid(g) for p in order for g in p]))
    return out


def many_vertex_polygon(k=320):
    """A wobbling ring of k vertices round (80, 64): the serial edge loop of coco_toggle_kernel, two to four grid points an edge."""
    rs = np.random.RandomState(k)
    ang = 2 * np.pi * np.arange(k) / k
    rad = 50 + rs.uniform(-4, 4, k)
    xy = np.stack([80 + rad * np.cos(ang), 64 + rad * np.sin(ang)], 1)
    return [float(v) for v in np.round(xy, 2).reshape(-1)]


@functools.lru_cache(None)
def long_edge_records():
    h, w = LONG_EDGE_SIZE
    out = [one_piece(name, h, w, poly) for name, _, _, _, poly in long_edge_polygons()]
    out.append(one_piece('320 vertices', h, w, many_vertex_polygon()))
    for i, r in enumerate(out):
        r['image_id'] = i
    return out


# ---- COCO sizes: one batch of unequal images, the content of tools/coco_mask_bench.py's generator restated ----
COCO_SIZES = [(480, 640), (640, 480), (427, 640)]
CROWD_AT = 4                      # the crowd's place in the annotation list: four persons before it, four after


def coco_like_record(h, w, seed, image_id, persons=8, polygons=2, vertices=40):
    """Persons as pairs of 40-gons round random centres and one crowd RLE of a few hundred runs in the middle of the list.  The
    miss rule (no keypoints, or area <= 32 * 32) is met from both sides, before and after the crowd."""
    rs = np.random.RandomState(seed)
    anns = []
    for _ in range(persons):
        polys = []
        for _ in range(polygons):
            cx, cy, r = rs.uniform(0, w), rs.uniform(0, h), rs.uniform(15, 90)
            ang = np.sort(rs.uniform(0, 2 * np.pi, vertices))
            rad = r * rs.uniform(0.6, 1.0, vertices)
            xy = np.stack([cx + rad * np.cos(ang), cy + 1.6 * rad * np.sin(ang)], 1)
            polys.append([float(v) for v in np.round(xy, 2).reshape(-1)])
        anns.append([polys, 0, int(rs.randint(1, 17)), float(rs.uniform(1100, 40000))])
    for at, nk, area in ((0, 0, 30000.0), (1, 9, 1024.0), (2, 1, 1025.0), (5, 12, 500.0), (6, 0, 0.0)):
        anns[at][2:] = [nk, area]
    runs = rs.randint(1, 2 * h * w // 400, 399)
    runs = [int(v) for v in runs[:int(np.searchsorted(np.cumsum(runs), h * w))]]
    anns.insert(CROWD_AT, [rle(h, w, runs + [h * w - sum(runs)]), 1, 0, 5000.0])
    return named('COCO-like', h, w, [tuple(a) for a in anns], image_id)


@functools.lru_cache(None)
def coco_size_records():
    out = [coco_like_record(h, w, seed=640 + i, image_id=i) for i, (h, w) in enumerate(COCO_SIZES)]
    return out + [named('no annotations', 1, 1, [], image_id=len(out))]


# ---- random polygons at size ----
@functools.lru_cache(None)
def random_at_size_records(n=60, seed=20241021):
    """n seeded polygons, one annotation each, like cm.random_polygon_records on images of two and of four chunks."""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        h, w = ((131, 97), (160, 200))[rs.randint(2)]
        k, dec = rs.randint(3, 13), rs.randint(0, 3)
        out.append(named('random %d-gon' % k, h, w, [([random_polygon(rs, h, w, k, dec)], 0, 5, 4000.0)], image_id=i))
    return out


GROUPS = {
    'chunk boundaries': chunk_boundary_records,
    'directed toggles': directed_toggle_records,
    'whole image': whole_image_records,
    'long RLEs': long_rle_records,
    'long edges': long_edge_records,
    'COCO sizes': coco_size_records,
    'random at size': random_at_size_records,
}


def reference(group):
    """[(mask_miss, mask_all)] of a group, computed once (cm.reference_masks: read-only arrays)."""
    return cm.reference_masks(('large', group), GROUPS[group]())
