"""CPU-only: the large mask cases (tests/coco_mask_large_cases.py) reach what they name -- more than one 256-word chunk of a plane,
a carry of 1 into a chunk without toggles, all four waves of a chunk, a second pass of the lanes over an RLE's cumulative sums and
over an edge's points in every along_x / flip combination -- and the restatement's two formulations agree at these sizes."""
import ctypes as C
import functools

import numpy as np

import coco_mask_common as cm
import coco_mask_large_cases as lc
from offsetguided_amd import _lib, data
from offsetguided_amd.data import annotations, masks


@functools.lru_cache(None)
def every_piece():
    """[(group, record name, h, w, kind, piece, positions, column-major bits of the filled plane)] of the whole table."""
    out = []
    for group, build in lc.GROUPS.items():
        for r in build():
            h, w = r['height'], r['width']
            for kind, piece in lc.pieces(r):
                pos = lc.piece_positions(kind, piece, h, w)
                out.append((group, r['name'], h, w, kind, piece, pos, cm.plane_runs(pos, h, w).T.reshape(-1)))
    return out


def test_formulations_agree_on_every_piece():
    assert len(every_piece()) > 150
    for group, name, h, w, kind, piece, pos, flat in every_piece():
        assert np.array_equal(cm.plane_xor(pos, h, w).T.reshape(-1), flat), (group, name)
        if kind == 'rle':
            assert np.array_equal(cm.paint_runs(piece, h, w).T.reshape(-1), flat), (group, name)


def test_sizes_are_the_chunk_counts_they_name():
    assert [h * w for h, w, _ in lc.CHUNK_BOUNDARY_SIZES] == [8160, 8191, 8191, 8192, 8193, 8224, 16384, 16385, 12707]
    for h, w, chunks in lc.CHUNK_BOUNDARY_SIZES:
        # a plane of up to 8192 pixels is one chunk by definition; every size beyond it takes the fill loop's second turn
        assert lc.chunks_of(h * w) == chunks and (chunks >= 2) == (h * w > lc.CHUNK)
    assert [(r['height'], r['width']) for r in lc.chunk_boundary_records()] == [s[:2] for s in lc.CHUNK_BOUNDARY_SIZES]
    assert [lc.chunks_of(h * w) for h, w in lc.DIRECTED_SIZES] == [3, 4] and lc.DIRECTED_SIZES[0][0] * lc.DIRECTED_SIZES[0][1] == 16385
    for group in ('directed toggles', 'whole image', 'long RLEs', 'long edges', 'random at size'):
        assert all(lc.chunks_of(r['height'] * r['width']) >= 2 for r in lc.GROUPS[group]()), group
    assert [lc.chunks_of(r['height'] * r['width']) for r in lc.coco_size_records()] == [38, 38, 34, 1]
    assert (427 * 640 + 31) // 32 % lc.CHUNK_WORDS != 0                     # a partial last chunk after 33 full ones


def test_carry_is_exercised_both_ways():
    before_boundary = set()
    free_chunk_with_carry, all_waves = [], []
    for group, name, h, w, kind, piece, pos, flat in every_piece():
        hw = h * w
        for c in range(1, lc.chunks_of(hw)):
            before_boundary.add(int(flat[lc.CHUNK * c - 1]))
            if flat[lc.CHUNK * c - 1] and not any(lc.CHUNK * c <= p < min(lc.CHUNK * (c + 1), hw) for p in pos):
                free_chunk_with_carry.append((group, c + 1 < lc.chunks_of(hw)))
        odd = np.zeros(hw + 1, np.int64)
        np.add.at(odd, np.minimum(pos, hw), 1)
        odd = (odd[:hw] & 1).astype(bool)
        for c in range(lc.chunks_of(hw)):
            waves = [odd[lc.CHUNK * c + 2048 * v:lc.CHUNK * c + 2048 * (v + 1)].any() for v in range(4)]
            if all(waves):
                all_waves.append((name, c))
    assert before_boundary == {0, 1}
    # a chunk without toggles entered with a carry of 1: with chunks after it (the carry passes through), and as the last one
    assert ('directed toggles', True) in free_chunk_with_carry and ('whole image', False) in free_chunk_with_carry
    assert any(c >= 1 for _, c in all_waves) and any(c == 0 for _, c in all_waves)


def test_directed_toggles_fill_what_they_say():
    want = {'toggle at 0': lambda hw: hw, 'toggle at 8191': lambda hw: hw - 8191, 'toggle at 8192': lambda hw: hw - 8192,
            'open at 100, close at 16384': lambda hw: 16284, 'open at 8191, close at 16384': lambda hw: 8193,
            'stacked toggles': lambda hw: 4096, 'whole image covered': lambda hw: hw}
    seen = set()
    for group, name, h, w, kind, piece, pos, flat in every_piece():
        key = name.split(' (')[0]
        if group in ('directed toggles', 'whole image') and key in want:
            assert int(flat.sum()) == want[key](h * w), name
            seen.add(key)
        if key == 'toggle at %d' % (h * w - 1):
            assert int(flat.sum()) == 1 and flat[-1]
        if group == 'whole image':                   # every toggle but the one at position 0 cancels
            odd = [p for p in set(pos) if pos.count(p) % 2 and p < h * w]
            assert odd == [0] and kind == 'polygon', name
    assert seen == set(want)
    stacked = [p for g, n, h, w, k, p, *_ in every_piece() if n.startswith('stacked')]
    assert len(stacked) == 2 and all(p[:6] == [8191, 0, 1, 0, 0, 4096] for p in stacked)


def test_rle_lanes_take_more_than_one_pass():
    rles = [(name, h, w, piece, flat) for g, name, h, w, kind, piece, _, flat in every_piece() if g == 'long RLEs']
    assert [len(p) for _, _, _, p, _ in rles] == lc.LONG_RLE_RUNS + [303]
    for name, h, w, piece, flat in rles:
        # what a single pass of 256 lanes would leave: the plane of the first 256 cumulative sums (the last sum, h w, sets nothing)
        single = cm.plane_xor([int(c) for c in np.cumsum(piece)[:lc.LANES]], h, w).T.reshape(-1)
        assert np.array_equal(single, flat) == (len(piece) <= lc.LANES + 1), name
    crowd = [len(p) for g, _, _, _, kind, p, *_ in every_piece() if g == 'COCO sizes' and kind == 'rle']
    assert len(crowd) == 3 and all(lc.LANES < n <= 400 for n in crowd)


def test_edge_lanes_take_more_than_one_pass_in_every_orientation():
    h, w = lc.LONG_EDGE_SIZE
    polygons = lc.long_edge_polygons()
    assert sorted((n, along_x, flip) for _, n, along_x, flip, _ in polygons) == \
        sorted((n, a, f) for n in (255, 256, 511, 512) for a in (False, True) for f in (False, True))
    outside = set()
    for name, n, along_x, flip, poly in polygons:
        tagged, edges = lc.tagged_positions(poly, h, w)
        assert [p for p, _, _ in tagged] == cm.polygon_positions(poly, h, w), name          # the same arithmetic
        assert edges[0] == (n, along_x, flip), (name, edges)
        first_pass = [p for p, _, i in tagged if i < lc.LANES]
        changed = not np.array_equal(cm.plane_xor(first_pass, h, w), cm.plane_xor([p for p, _, _ in tagged], h, w))
        if n < lc.LANES:
            assert max(e[0] for e in edges) < lc.LANES and not changed, name
        else:
            assert any(j == 0 and i >= lc.LANES for _, j, i in tagged) and changed, name
        xs, ys = poly[0::2], poly[1::2]
        outside |= {s for s, out in (('left', min(xs) < 0), ('right', max(xs) > w), ('top', min(ys) < 0), ('bottom', max(ys) > h)) if out}
    assert outside == {'left', 'right', 'top', 'bottom'}
    ring = lc.many_vertex_polygon()
    tagged, edges = lc.tagged_positions(ring, h, w)
    assert len(edges) >= 300 and len(ring) == 2 * len(edges) and [p for p, _, _ in tagged] == cm.polygon_positions(ring, h, w)
    assert 6000 < int(cm.plane_runs(cm.polygon_positions(ring, h, w), h, w).sum()) < 9500          # pi 46^2 .. pi 54^2, plus the rim
    # the random set at size has second passes of its own: an edge of more than 256 points is no longer luck
    longest = [max(e[0] for e in lc.tagged_positions(r['segmentation'][0][0], r['height'], r['width'])[1]) for r in lc.random_at_size_records()]
    assert len(longest) == 60 and sum(n >= lc.LANES for n in longest) >= 20


def test_compressed_string_round_trip():
    runs = lc.compressed_rle_runs()
    s = lc.long_rle_records()[-1]['segmentation'][0]['counts']
    assert isinstance(s, str) and cm.string_to_runs(s) == runs == data.rle_counts(s) and cm.runs_to_string(runs) == s
    assert sum(runs) == 480 * 640 and len(runs) == 303 and sum(v > 1 << 15 for v in runs) == 4 and runs[-1] > 1 << 16
    deltas = [runs[i] - runs[i - 2] for i in range(3, len(runs))]
    assert min(deltas) < -(1 << 15) and max(deltas) > 1 << 15 and len(s) > len(runs) + 100          # values of more than one character


def _counts(records):
    n_pieces = sum(len(lc.pieces(r)) for r in records)
    n_vertices = sum(len(p) // 2 for r in records for kind, p in lc.pieces(r) if kind == 'polygon')
    n_cums = sum(len(p) for r in records for kind, p in lc.pieces(r) if kind == 'rle')
    return len(records), sum(len(r['area']) for r in records), n_pieces, n_vertices, n_cums


def test_mask_tables_accepts_every_record_and_so_does_the_library():
    lib = _lib.load()
    for group, build in lc.GROUPS.items():
        records = build()
        tables = data.mask_tables(records)
        assert tables.counts == _counts(records), group
        assert tables.sizes == [(r['height'], r['width']) for r in records] and tables.out_bytes == sum(h * w for h, w in tables.sizes)
        desc = masks.descriptor(tables, tables.buffer.ctypes.data, 16, 16, 16)          # validated on the host, nothing launched
        words = sum((r['height'] * r['width'] + 31) // 32 * len(lc.pieces(r)) for r in records)
        assert lib.og_coco_mask_workspace_bytes(C.byref(desc)) == (4 * words + 15) // 16 * 16 + 16, (group, lib.og_last_error())
    assert _counts(lc.coco_size_records())[:3] == (4, 27, 51)
    assert _counts(lc.directed_toggle_records())[:3] == (35, 35, 35) and _counts(lc.long_edge_records())[:4] == (17, 17, 17, 16 * 3 + 320)


def test_coco_batch_reaches_both_states_and_both_crowd_overlaps():
    records = lc.coco_size_records()
    assert [(r['height'], r['width']) for r in records] == lc.COCO_SIZES + [(1, 1)] and len(records[-1]['area']) == 0
    for r, (miss, every) in zip(records[:3], lc.reference('COCO sizes')):
        h, w = r['height'], r['width']
        assert miss.shape == every.shape == (h, w)
        assert set(np.unique(miss)) == {0, 255} and set(np.unique(every)) == {0, 255}
        assert list(r['iscrowd']) == [0] * lc.CROWD_AT + [1] + [0] * 4
        planes = [cm.annotation_mask(s, h, w) for s in r['segmentation']]
        crowd = planes[lc.CROWD_AT]
        before, after = np.logical_or.reduce(planes[:lc.CROWD_AT]), np.logical_or.reduce(planes[lc.CROWD_AT + 1:])
        assert (crowd & before).any() and (crowd & after & ~before).any()
        # a labelled person listed before the crowd takes the crowd's term back, one listed after does not
        labelled = ~np.logical_or.reduce([planes[j] for j in (0, 1, 6, 7)])          # list places 0, 1, 6 and 7 fall under the miss rule
        assert (miss[crowd & before & labelled] == 255).all() and (miss[crowd & ~before] == 0).all()
        tables = data.mask_tables([r])
        flags = list(tables.buffer[tables.at[1]:tables.at[1] + 9 * annotations.ANN_DT.itemsize].view(annotations.ANN_DT)['flags'])
        assert flags == [annotations.MISS, annotations.MISS, 0, 0, annotations.CROWD, 0, annotations.MISS, annotations.MISS, 0]
        assert list(r['area'][[1, 2]]) == [1024.0, 1025.0] and list(r['num_keypoints'][[0, 7]]) == [0, 0]
    miss, every = lc.reference('COCO sizes')[3]
    assert miss.tolist() == [[255]] and every.tolist() == [[0]]
