"""CPU: the numpy restatements of the model-inspection views (tests/views_common.py) checked against themselves in fp64 and against
plain Python loops, the VIRIDIS table, and the command line.  The HIP kernels are held to the fp32 restatements bit for bit in
tests/test_gpu_views.py."""
import numpy as np
import pytest

import views_common as vc
from offsetguided_amd import evaluate, visualization

# fp32 against fp64, both restatements on the same fp32 maps: the colour index t * (n - 1) + 0.5 and the blend carry ~1e-7 relative
# error, so a pixel changes only where one of the two floors sits within that of a step -- with a 2-colour table the index step is a
# whole colour, which is why the share is stated and the cases are seeded: no pixel may differ by more than one level, and at most one
# in a thousand by that
SHARE = 1e-3


def _levels(a, b):
    return np.abs(a.astype(np.int16) - b.astype(np.int16)).max(axis=-1)


@pytest.mark.parametrize('name', sorted(vc.HEATMAP_CASES))
def test_heatmap_fp32_restatement_within_one_level_of_fp64(name):
    a, b = vc.heatmap_expected(name, np.float32), vc.heatmap_expected(name, np.float64)
    diff = _levels(a, b)
    assert diff.max() <= 1 and (diff > 0).mean() <= SHARE, (name, int(diff.max()), float((diff > 0).mean()))
    assert (a != vc.HEATMAP_CASES[name]['images']).any(), 'the case paints nothing'


@pytest.mark.parametrize('name', sorted(vc.SEGMENT_CASES))
def test_segments_fp32_restatement_within_one_level_of_fp64(name):
    """As the pose painter's (test_draw_cpu.py): positions carry ~1e-4 px of fp32 error, the blend a few 1e-5 of a level per primitive --
    the final rounding can land on either side of a .5, by one level, on few pixels."""
    a, b = vc.segments_expected(name, np.float32), vc.segments_expected(name, np.float64)
    diff = _levels(a, b)
    assert diff.max() <= 1 and (diff > 0).mean() <= 10 * SHARE, (name, int(diff.max()), float((diff > 0).mean()))
    assert (a != vc.SEGMENT_CASES[name]['images']).any(), 'the case paints nothing'


def test_heatmap_cases_hold_what_they_are_for():
    kept = lambda name: vc.heatmap_expected(name) != vc.HEATMAP_CASES[name]['images']       # noqa: E731
    # the plateau: every pixel is its window's maximum -> painted with the colour of 0.5 at alpha 1
    c = vc.HEATMAP_CASES['plateau']
    assert (vc.hires(c) == 0.5).all()
    assert (vc.heatmap_expected('plateau') == c['lut'][int(np.floor(0.5 * 255 + 0.5))]).all()
    # negative everywhere: the border loses to the zero padding (u = -0 -> t = 0.5), the interior keeps -0.25 (t = 0.25)
    c = vc.HEATMAP_CASES['negative']
    out = vc.heatmap_expected('negative')
    assert (out[0, 1:-1, 1:-1] == c['lut'][64]).all() and (out[0, 0] == c['lut'][128]).all() and (out[0, :, -1] == c['lut'][128]).all()
    # the peaks: maxima on the four corners, on every edge, and equal pairs across the tile seams X = 63 | 64 and Y = 15 | 16
    v = vc.hires(vc.HEATMAP_CASES['peaks'])[0]
    H, W = v.shape
    padded = np.zeros((H + 2, W + 2), np.float32)
    padded[1:-1, 1:-1] = v
    peak = (np.max([padded[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], axis=0) == v) & (v > 0.5)
    assert peak[0, 0] and peak[0, W - 1] and peak[H - 1, 0] and peak[H - 1, W - 1]
    assert peak[0, 1:-1].any() and peak[H - 1, 1:-1].any() and peak[1:-1, 0].any() and peak[1:-1, W - 1].any()
    assert (peak[:, vc.TILE_W - 1] & peak[:, vc.TILE_W]).any() and (peak[vc.TILE_H - 1] & peak[vc.TILE_H]).any()
    assert peak[vc.TILE_H - 1:vc.TILE_H + 1, vc.TILE_W - 1:vc.TILE_W + 1].all()
    # NaN leaves pixels alone, the rest is painted (alpha 0.8 over random pixels changes nearly all of them)
    for nms in (0, 1):
        c = vc.HEATMAP_CASES[f'nonfinite_nms{nms}']
        v = vc.hires(c)
        assert np.isnan(v).any() and np.isposinf(v).any()
        assert not kept(f'nonfinite_nms{nms}')[np.isnan(v)].any()
    # several tiles, partial on both axes
    assert vc.HEATMAP_CASES['multi_nms1']['images'].shape[1:3] == (36, 140) and 36 % vc.TILE_H and 140 % vc.TILE_W


def test_segment_order_matters():
    ab, ba = vc.segments_expected('order_ab'), vc.segments_expected('order_ba')
    assert (ab != ba).any()
    # b's start disc lies on a's line: a then b leaves the disc's green there, b then a the line's red
    assert tuple(ab[0, 9, 20]) == (0, 128, 0) and tuple(ba[0, 9, 20]) == (255, 0, 0)


def test_segment_cases_hold_what_they_are_for():
    c = vc.SEGMENT_CASES['basic']
    out = vc.segments_expected('basic')
    assert c['n_segs'][0] > c['segs'].shape[1] and c['n_segs'][1] == 0
    assert np.array_equal(out[1], c['images'][1]) and (out[0] != c['images'][0]).any() and (out[2] != c['images'][2]).any()
    assert tuple(out[0, 9, 12]) == (0, 128, 0)                                   # the zero-length segment: its discs
    c = vc.SEGMENT_CASES['overflow']
    assert c['segs'].shape[1] == vc.LIST_CAP + 1 and c['r_start'] == 0 and c['r_end'] == 0
    xy = c['segs'][0].reshape(-1, 2)
    assert (xy[:, 0] >= 32).all() and (xy[:, 0] <= 63).all() and (xy[:, 1] >= 0).all() and (xy[:, 1] <= 7).all()   # all through tile (1, 0)
    # a non-finite coordinate skips the whole segment: painting only the finite rows gives the same picture
    c = vc.SEGMENT_CASES['nonfinite_rstart0']
    finite = np.isfinite(c['segs'][0]).all(axis=1)
    assert 0 < finite.sum() < len(finite)
    only = vc.segments_reference(**{**c, 'segs': c['segs'][:, finite], 'n_segs': [int(finite.sum())]}, dtype=np.float32)
    assert np.array_equal(only, vc.segments_expected('nonfinite_rstart0'))


@pytest.mark.parametrize('name', sorted(vc.LIMB_TABLES))
def test_limbs_compaction_against_a_plain_loop(name):
    c = vc.LIMB_TABLES[name]
    got = vc.limbs_expected(name)
    for n, table in enumerate(c['limbs']):
        rows = []
        for l in range(table.shape[0]):
            for i in range(table.shape[1]):
                r = table[l, i]
                if (c['limb'] is None or l == c['limb']) and r[0] > 0 and r[3] > 0 and r[8] <= np.float32(c['dist_max']):
                    rows.append([r[0], r[1], r[3], r[4]])
        assert len(rows) == len(got[n]) and np.array_equal(np.array(rows, np.float32).reshape(-1, 4), got[n])
    if name == 'random':
        first = got[0][0]                  # of the hand-set rows (0, 0 ... 4) only (0, 1), col8 == dist_max, survives
        assert tuple(first[[0, 2]]) == (5.0, 5.0) and 0 < len(got[0]) < 19 * 48 and len(got[0]) != len(got[1])
    if name in ('nothing', 'one_filtered'):
        assert all(len(g) == 0 for g in got)
    if name == 'one':
        assert np.array_equal(got[0], [[3.0, 4.0, 5.0, 6.0]])


@pytest.mark.parametrize('name', sorted(vc.OFFSET_FIELDS))
def test_offsets_compaction_against_a_plain_loop(name):
    c = vc.OFFSET_FIELDS[name]
    heat, U, V = vc.offset_planes(c)
    got = vc.offsets_expected(name)
    N, H, W = heat.shape
    for n in range(N):
        rows = []
        for Y in range(0, H, c['step']):
            for X in range(0, W, c['step']):
                if heat[n, Y, X] >= np.float32(c['thre']) and np.isfinite(U[n, Y, X]) and np.isfinite(V[n, Y, X]):
                    rows.append([np.float32(X), np.float32(Y), np.float32(X) + U[n, Y, X], np.float32(Y) + V[n, Y, X]])
        assert len(rows) == len(got[n]) and np.array_equal(np.array(rows, np.float32).reshape(-1, 4), got[n])
        assert len(got[n]) <= -(-H // c['step']) * -(-W // c['step'])
    if name == 'step7':
        assert H % 7 and W % 7 and heat[0, 7, 21] == np.float32(0.25) == np.float32(c['thre'])       # heat == thre ...
        assert any(tuple(r[:2]) == (21.0, 7.0) for r in got[0])                                      # ... is kept
        assert len(got[0]) != len(got[1]) and len(got[0]) > 0
    if name == 'step1':
        dropped = ~(np.isfinite(U[0]) & np.isfinite(V[0])) & (heat[0] >= np.float32(c['thre']))
        assert dropped.any(), 'no infinite offset under a hot pixel: the case does not test the drop'
    if name == 'dense':
        assert len(got[0]) > 2 * vc.ROUND


def test_viridis_table():
    v = visualization.VIRIDIS
    assert v.shape == (256, 3) and v.dtype == np.uint8
    anchors = np.array([[68, 1, 84], [71, 45, 123], [59, 82, 139], [44, 114, 142], [33, 144, 140], [39, 173, 129], [93, 200, 99],
                        [170, 220, 50], [253, 231, 37]], np.uint8)
    positions = [0, 32, 64, 96, 128, 159, 191, 223, 255]
    assert np.array_equal(v[positions], anchors)
    assert (np.abs(np.diff(v.astype(np.int16), axis=0)) <= 3).all()           # linear in between: no jumps


def test_cli_view_flags():
    a = evaluate.evaluate_cli(['--no-pretrain'])
    assert a.show_hmp_idx is None and a.show_limb_idx is None and not a.show_all_limbs
    a = evaluate.evaluate_cli(['--no-pretrain', '--show-hmp-idx', '16', '--show-limb-idx', '18', '--show-all-limbs', '--show-dir', 'x',
                               '--flip-test', '--test-scales', '1.0', '0.5'])
    assert a.show_hmp_idx == 16 and a.show_limb_idx == 18 and a.show_all_limbs and a.show_dir == 'x'
    for flags in (['--show-hmp-idx', '0'], ['--show-limb-idx', '0'], ['--show-all-limbs']):
        with pytest.raises(SystemExit):
            evaluate.evaluate_cli(['--no-pretrain', '--cat-flip-offset', '--flip-test'] + flags)
    for flags in (['--show-hmp-idx', '17'], ['--show-hmp-idx', '-1'], ['--show-limb-idx', '19'], ['--show-limb-idx', '-1']):
        with pytest.raises(SystemExit):
            evaluate.evaluate_cli(['--no-pretrain'] + flags)
    evaluate.evaluate_cli(['--no-pretrain', '--cat-flip-offset', '--flip-test'])        # without a view the flag stays accepted
