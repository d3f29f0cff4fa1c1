"""CPU side of the input-chain cases (tests/input_chain_common.py): the oracle's resize against a second, independent restatement;
the coverage the table's path labels claim; the bound that keeps the fused kernel's LDS writes in range; the constants."""
import os
import re

import numpy as np
import pytest

import input_chain_common as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, 'offsetguided_amd', 'csrc', 'preprocess.hip')


# ---------------------------------------------------------------------------------------------- a second restatement of the resize
def _coeffs(x):
    """OpenCV's interpolateCubic (imgproc/resize.cpp) in np.float32, operation by operation, then saturate_cast<short>(c * 2048):
    round half to even."""
    f = np.float32
    x = np.asarray(x, np.float32)
    A = f(-0.75)
    c0 = ((A * (x + f(1)) - f(5) * A) * (x + f(1)) + f(8) * A) * (x + f(1)) - f(4) * A
    c1 = ((A + f(2)) * x - (A + f(3))) * x * x + f(1)
    c2 = ((A + f(2)) * (f(1) - x) - (A + f(3))) * (f(1) - x) * (f(1) - x) + f(1)
    c3 = f(1) - c0 - c1 - c2
    c = np.stack([c0, c1, c2, c3], -1)
    assert c.dtype == np.float32
    return np.clip(np.rint(c * f(2048)), -32768, 32767).astype(np.int64)


def _axis(n_src, n_new, scale):
    """-> (clamped source indices (n_new, 4), fixed-point taps (n_new, 4)): fx = (float)((dx + 0.5) * scale_x - 0.5), sx = cvFloor(fx),
    fx -= sx; taps sx - 1 .. sx + 2, replicated border."""
    f = ((np.arange(n_new, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    idx = np.clip(s.astype(np.int64)[:, None] - 1 + np.arange(4), 0, n_src - 1)
    return idx, _coeffs(f - s.astype(np.float32))


def resize_np(img, nh, nw, sy=None, sx=None):
    """cv::resize(INTER_CUBIC) for 8-bit images as resizeGeneric_ does it: horizontal pass to int rows, vertical pass,
    (sum + 2^21) >> 22, saturate.  Sums in int64, with OpenCV's int range asserted.  (h, w, C) -> (nh, nw, C)."""
    h, w = img.shape[:2]
    yi, yt = _axis(h, nh, h / nh if sy is None else sy)
    xi, xt = _axis(w, nw, w / nw if sx is None else sx)
    rows = np.unique(yi)
    src = img.astype(np.int64)[rows]                                          # only the rows some tap reads
    hs = (src[:, xi, :] * xt[None, :, :, None]).sum(2)                        # (rows, nw, C)
    yi = np.searchsorted(rows, yi)
    acc = (hs[yi] * yt[:, :, None, None]).sum(1)                              # (nh, nw, C)
    assert np.abs(hs).max() < 2 ** 31 and np.abs(acc).max() < 2 ** 31 - 2 ** 21
    return np.clip((acc + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def shrink_np(mask, stride):
    """encoder/heatmap.py:56-60: cv2.resize(mask, (0, 0), fx=1 / stride, fy=1 / stride, INTER_CUBIC).astype(float32) / 255 > 0.7.
    cv::resize with an empty dsize: dsize = cvRound(size * fx) (half to even), scale = 1 / fx."""
    fx = 1 / stride
    nh, nw = int(np.rint(mask.shape[0] * fx)), int(np.rint(mask.shape[1] * fx))
    res = resize_np(mask[:, :, None], nh, nw, 1 / fx, 1 / fx)[:, :, 0]
    return res.astype(np.float32) / np.float32(255) > np.float32(0.7)


def test_second_restatement_has_the_resize_properties():
    """Before it judges the oracle: identity at equal size, constants stay constant, the taps sum to 2048 at x = 0 and 0.5."""
    im = ic.image('noise', 9, 13)
    assert np.array_equal(resize_np(im, 9, 13), im)
    assert (resize_np(np.full((7, 5, 3), 201, np.uint8), 19, 11) == 201).all()
    assert _coeffs(np.float32(0)).tolist() == [0, 2048, 0, 0] and _coeffs(np.float32(0.5)).tolist() == [-192, 1216, 1216, -192]


def test_oracle_resize_equals_the_second_restatement_on_the_table():
    """oracle.resize_cubic_u8 == resize_np, bit for bit, on every (source, resized) pair of the table: all three image kinds where the
    source is small, noise alone above 2^17 pixels."""
    import oracle
    done = 0
    for h, w, nh, nw in ic.pairs():
        for kind in ic.KINDS if h * w <= 1 << 17 else ('noise',):
            im = ic.image(kind, h, w)
            got, ref = oracle.resize_cubic_u8(im, nh, nw), resize_np(im, nh, nw)
            bad = np.argwhere((got != ref).any(2))
            assert not len(bad), f'{(h, w)} -> {(nh, nw)} {kind}: {len(bad)} pixels differ, first (row, col) {bad[:5].tolist()}'
            done += 1
    assert done >= 3 * 40


def test_oracle_mask_shrink_equals_the_second_restatement():
    """oracle.shrink_mask_miss_u8 == shrink_np on the mask cases: sizes that the stride does not divide scale by the stride, not by
    size / rounded size (cv::resize keeps fx when dsize is empty), and halves round to even."""
    import oracle
    sizes = {}
    for stride, (h, w), kind in ic.MASK_CASES:
        m = ic.mask(kind, 3, h, w)
        for n in range(3):
            got, ref = oracle.shrink_mask_miss_u8(m[n], stride), shrink_np(m[n], stride)
            assert got.shape == ref.shape and got.dtype == bool, (stride, h, w)
            assert np.array_equal(got, ref), (stride, h, w, kind, n, np.argwhere(got != ref)[:5].tolist())
        sizes[stride, h, w] = ref.shape
        if kind.startswith('const'):
            assert ref.all() == (int(kind[5:]) >= 179) and ref.all() == ref.any(), kind
    assert sizes[4, 130, 134] == (32, 34) and sizes[16, 40, 72] == (2, 4) and sizes[4, 4, 4] == (1, 1) and sizes[2, 33, 47] == (16, 24)
    assert {s for s, _, _ in ic.MASK_CASES} == {1, 2, 4, 8, 16}
    # the grey cases do sit on both sides of the threshold, and 'near' crowds it
    near = resize_np(ic.mask('near', 1, 37, 53)[0][:, :, None], 9, 13, 4.0, 4.0)
    assert (near >= 179).any() and (near < 179).any() and (np.abs(near.astype(int) - 179) <= 3).sum() >= 5


# ------------------------------------------------------------------------------------------------------ what the table covers
def test_every_label_is_the_restated_decision_and_both_paths_meet_both_paddings():
    seen = set()
    for c in ic.CASES:
        assert c.label == ic.label_of(c.h, c.w, c.nh, c.nw), c.name
        assert c.nh <= c.TH and c.nw <= c.TW and max(c.TH, c.TW) <= 256, c.name
        seen.add((c.label, c.corner))
    assert seen == {('lds', 0), ('lds', 1), ('direct', 0), ('direct', 1)}
    assert len({c.name for c in ic.CASES}) == len(ic.CASES)
    labels = {(h, w, nh, nw): lab for h, w, nh, nw, lab in ic.mixed_launch()}
    assert {'lds', 'direct'} == set(labels.values()) and len(labels) >= 40
    s = ic.seventy()
    assert len(s) == 70 and [ic.label_of(*s[i]) for i in (63, 64, 65)] == ['lds', 'direct', 'lds']
    assert all(nh <= 130 and nw <= 200 for _, _, nh, nw in s)
    # the existing test's large reduction, 3000 x 2000 -> 640, stays on the LDS path; the size added next to it does not
    from offsetguided_amd import transforms
    tw, th = transforms.rescale_size(2000, 3000, 640)
    assert ic.estimate(3000, 2000, th, tw) == (308, 26) and ic.takes_lds(3000, 2000, th, tw)
    tw, th = transforms.rescale_size(2200, 3300, 640)
    assert not ic.takes_lds(3300, 2200, th, tw)


def test_geometry_the_table_promises():
    """Centre padding: left % 64 in {0, 1, 63} and top % 4 in {0, 1, 2, 3}; resized images that end on a tile's last and first
    column / row; targets that are no multiple of the tile; sources below the four taps; resized images of one row / column / pixel."""
    centre = [c for c in ic.CASES if not c.corner]
    lt = [ic.pad_left_top(c.nh, c.nw, c.TH, c.TW, 0) for c in centre]
    assert {0, 1, 63} <= {l % 64 for l, _ in lt if l >= 63} | {l for l, _ in lt if l == 0} and {t % 4 for _, t in lt} == {0, 1, 2, 3}
    for corner in (0, 1):
        ends = [((l + c.nw - 1) % 64, (t + c.nh - 1) % 4) for c in ic.CASES if c.corner == corner and c.nw > 1 and c.nh > 1
                for l, t in [ic.pad_left_top(c.nh, c.nw, c.TH, c.TW, corner)]]
        assert {0, 63} <= {x for x, _ in ends} and {0, 3} <= {y for _, y in ends}, corner
    assert any(c.TW % 64 and c.TH % 4 for c in ic.CASES) and any((c.TH, c.TW) == (70, 130) and c.label == 'direct' for c in ic.CASES)
    small = {(c.h, c.w) for c in ic.CASES if min(c.h, c.w) <= 3}
    assert {(1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (3, 5)} <= small
    for hw in ((1, 7), (7, 1), (2, 2), (3, 3)):
        grows = {c.nh * c.nw > c.h * c.w for c in ic.CASES if (c.h, c.w) == hw}
        assert grows == {True, False}, hw
    shapes = {(min(c.nh, 2), min(c.nw, 2)) for c in ic.CASES if c.TH * c.TW > c.nh * c.nw}
    assert {(1, 1), (1, 2), (2, 1)} <= shapes
    assert any(c.h * 2 == c.nh and c.w * 2 == c.nw for c in ic.CASES) and any(c.h * 4 == c.nh and c.w * 4 == c.nw for c in ic.CASES)
    assert any(ic.tap_start(0, c.w / c.nw) == -2 for c in ic.CASES)
    # anisotropic on both paths
    assert {c.label for c in ic.CASES if max(c.w / c.nw, c.h / c.nh) > 8 * min(c.w / c.nw, c.h / c.nh)} == {'lds', 'direct'}


def test_limit_pairs_are_the_enumerated_maxima_and_straddle_the_threshold():
    for (src, new), (fsrc, fnew), aspect in ((ic.LIMIT_SQUARE, ic.FLIP_SQUARE, (1, 1)), (ic.LIMIT_LONG, ic.FLIP_LONG, (3, 2)),
                                             (ic.LIMIT_LONG_2, ic.FLIP_LONG_2, (3, 2))):
        best, found = ic.limit_pairs(*aspect)
        assert best == ic.LIMIT_BYTES and (*src, *new) in found, aspect
        if src != ic.LIMIT_LONG_2[0]:
            assert (*src, *new) == found[0], 'the smallest source that reaches the maximum'
        fw, fh = ic.estimate(*src, *new)
        assert (fw, fh) == (311, 26) and fw * fh * 3 == best <= ic.LDS_BYTES
        assert fnew == new and fsrc == ic.flip_neighbour(*src, *new, *aspect)
        fw, fh = ic.estimate(*fsrc, *fnew)
        assert fw * fh * 3 > ic.LDS_BYTES
    fw, fh = ic.estimate(*ic.LIMIT_EXACT[0], *ic.LIMIT_EXACT[1])
    assert (fw, fh) == (256, 32) and fw * fh * 3 == ic.LDS_BYTES                   # '<=': equality is still the LDS path
    fw, fh = ic.estimate(*ic.FLIP_EXACT[0], *ic.FLIP_EXACT[1])
    assert (fw, fh) == (256, 33)
    in_table = {(c.h, c.w, c.nh, c.nw): c.label for c in ic.CASES}
    for pair, lab in ((ic.LIMIT_SQUARE, 'lds'), (ic.FLIP_SQUARE, 'direct'), (ic.LIMIT_LONG, 'lds'), (ic.FLIP_LONG, 'direct'),
                      (ic.LIMIT_LONG_2, 'lds'), (ic.FLIP_LONG_2, 'direct'), (ic.LIMIT_EXACT, 'lds'), (ic.FLIP_EXACT, 'direct')):
        assert in_table[(*pair[0], *pair[1])] == lab


# ----------------------------------------------------------------------------------------------------------- the footprint bound
def test_staged_footprint_of_every_lds_case_fits():
    """What the kernel writes to its 24 KiB LDS image is lh * lw * 3 bytes from float32 tap positions; what the launcher tests is
    fw * fh * 3.  Every tile of every 'lds' case: lw <= fw, lh <= fh, lh * lw * 3 <= 24 576."""
    worst = 0
    for c in ic.CASES:
        if c.label != 'lds':
            continue
        fw, fh = ic.estimate(c.h, c.w, c.nh, c.nw)
        lws, lhs = ic.tile_footprints(c.h, c.w, c.nh, c.nw, c.TH, c.TW, c.corner)
        assert lws and lhs, c.name
        assert max(lws) <= fw and max(lhs) <= fh, (c.name, max(lws), fw, max(lhs), fh)
        assert max(lws) * max(lhs) * 3 <= ic.LDS_BYTES, c.name
        worst = max(worst, max(lws) * max(lhs) * 3)
    print(f'largest staged footprint of the table: {worst} bytes')
    # the limit pairs stage (63 s + 5) x (3 s + 5) pixels at s = 4.7368: 303 x 19 x 3 bytes.  (The estimate's margin is what the sweep
    # below measures; the decision is not tight.)
    assert worst == 303 * 19 * 3, 'the table no longer holds the largest footprint the LDS path is given'


def _sweep(tile, max_src, max_new, chunk=50):
    """max over (n_src <= max_src, n_new <= max_new, every window a tile can cut) of staged extent - estimate, and the argmax.

    A tile at offset `lead` in [0, tile) covers resized indices a = max(t * tile - lead, 0) .. b = min(t * tile + tile - 1 - lead,
    n_new - 1).  Over every lead and t these are the windows [a, min(a + tile - 1, n_new - 1)] for every a >= 0, and the first tile's
    shorter windows [0, tile - 1 - lead], whose extent is no larger than that of [0, tile - 1] because the tap start never decreases
    with the index (asserted).  So every lead in [0, tile) is covered by every window start a."""
    new = np.arange(1, max_new + 1)
    d = np.arange(max_new)
    worst, where = -10 ** 9, None
    for first in range(1, max_src + 1, chunk):
        src = np.arange(first, min(first + chunk, max_src + 1))
        scale = src[:, None] / new[None, :]                                                     # (S, N) double
        i0 = np.floor(((d[None, None, :] + 0.5) * scale[:, :, None] - 0.5).astype(np.float32)).astype(np.int64) - 1
        assert (np.diff(i0, axis=2) >= 0).all()
        b = np.minimum(d[None, :] + tile - 1, new[:, None] - 1)                                 # (N, D) window ends
        ext = np.take_along_axis(i0, np.broadcast_to(b[None], i0.shape), 2) + 3 - i0 + 1        # (S, N, D)
        ext = np.where(d[None, None, :] < new[None, :, None], ext, 0)
        est = (tile * scale).astype(np.int64) + 8
        over = ext.max(2) - est
        if over.max() > worst:
            s, n = np.unravel_index(over.argmax(), over.shape)
            worst, where = int(over.max()), (int(src[s]), int(new[n]))
    return worst, where


@pytest.mark.parametrize('tile, name', [(ic.TILE_W, 'lw'), (ic.TILE_H, 'lh')])
def test_footprint_estimate_bounds_the_staged_extent_in_a_sweep(tile, name):
    """lw <= (long)(64 s) + 8 and lh <= (long)(4 s) + 8 for every source size up to 700, resized size up to 256 and tile offset: the
    invariant that keeps the kernel's LDS writes in range (the two factors bound the product)."""
    worst, where = _sweep(tile, 700, 256)
    print(f'{name}: the staged extent exceeds the estimate by at most {worst} (source, resized = {where})')
    assert worst <= 0, (name, worst, where)


# --------------------------------------------------------------------------------------------------------------------- constants
def test_constants_and_decision_match_the_source():
    text = open(SOURCE).read()
    m = re.search(r'constexpr int kPrepTW = (\d+), kPrepTH = (\d+), kPrepLds = (\d+) \* (\d+);', text)
    assert m, 'the constexpr line of preprocess.hip changed: update tests/input_chain_common.py with it'
    tw, th, a, b = map(int, m.groups())
    assert (tw, th, a * b) == (ic.TILE_W, ic.TILE_H, ic.LDS_BYTES)
    # the launcher and the batch kernel compute the decision with the same two lines
    assert text.count('const long fw = (long)(kPrepTW * sx) + 8, fh = (long)(kPrepTH * sy) + 8;') == 2
    assert text.count('const int use_lds = fw * fh * 3 <= kPrepLds;') == 2
    assert re.search(r'constexpr int kPrepBatchMax = 64;', text)
