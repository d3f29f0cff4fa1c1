#!/usr/bin/env python3
"""Sweep fixture for the ground-truth encoder (tests/golden/encoder_sweep.npz) from the imported reference: what
tests/golden/encoder.npz (tools/gen_golden_encoder.py: square inputs, <= 30 persons, one skeleton, default flags) leaves
out -- a non-square input with a tail block, the four other skeletons, strides 2 and 8, every encoder flag, min_jscale
with joint scales below / on / above it, person counts past the kernels' LDS staging rounds (512 for the offsets, 1020 for
the heat maps) and a hand-planted case of exact ties and window edges.  Build container only, like its sibling: asserts
oracle == reference for every case it stores; stores joints, parameters and the reference's five outputs."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
import oracle  # noqa: E402
from offsetguided_amd import synth  # noqa: E402
from offsetguided_amd.config import coco_data as cd  # noqa: E402
from tools.gen_golden_encoder import GOLD, load_reference_generators, random_joints  # noqa: E402

SKELETONS = {'omp': cd.COCO_PERSON_SKELETON, 'omp16': cd.KINEMATIC_TREE_SKELETON,
             'omp31': cd.COCO_PERSON_WITH_REDUNDANT_SKELETON, 'omp44': cd.DENSER_COCO_PERSON_SKELETON,
             'omp25': cd.REDUNDANT_CONNECTIONS}
PARAMS = ('in_w', 'in_h', 'stride', 'sigma', 'clip', 'fill_jitter', 'fill_scale', 'min_jscale')
DEFAULTS = dict(stride=4, sigma=7, clip=0.01, fill_jitter=3, fill_scale=7, min_jscale=1.0, head='omp')


def joints_wh(seed, persons, in_w, in_h, min_jscale, keep=1.0):
    """random_joints on a (in_w, in_h) input: y shrunk to the height (eighths kept); a fifth of the scales exactly ON
    min_jscale (the rest fall on both sides of it); `keep` < 1 drops joints so that a crowd does not saturate the maps."""
    j = random_joints(seed, persons, in_w)
    if persons == 0:
        return j
    j[:, :, 1] = np.round(j[:, :, 1] * (in_h / in_w) * 8) / 8
    rng = synth.HashRng(seed + 1000)
    j[:, :, 3] = np.where(rng.uniform(persons * 17).reshape(persons, 17) < 0.2, np.float32(min_jscale), j[:, :, 3])
    if keep < 1:   # the dropped joints are zeroed whole (a crowd of random rows would not compress); garbage behind v == 0 stays elsewhere
        j *= (rng.uniform(persons * 17).reshape(persons, 17) < keep)[:, :, None]
    return j


def planted(in_w=128, in_h=96):
    """Hand-built persons for stride 4, jitter fill 4 (even), scale fill 7 (odd), min_jscale 1, COCO skeleton.  Cell (i, j) has its
    centre at (4 i + 1.5, 4 j + 1.5).  Every coordinate is a small dyadic number, so a*a + b*b == b*b + a*a bit for bit."""
    rows = []

    def person(**kp):
        p = np.zeros((17, 4), np.float32)
        for k, (x, y, s) in kp.items():
            p[int(k[1:])] = (x, y, 2, s)
        rows.append(p)
        return p

    def centre(i, j):
        return 4 * i + 1.5, 4 * j + 1.5

    def tied_pair(i, j, first, second, s_first, s_second, fr=5, to=7):
        """Two persons sharing the from-joint at the centre of cell (i, j); their to-joints at `first` / `second` from
        that centre (transposed: equal length at every cell of the diagonal through (i, j))."""
        cx, cy = centre(i, j)
        for (a, b), s in ((first, s_first), (second, s_second)):
            person(**{f'k{fr}': (cx, cy, s), f'k{to}': (cx + a, cy + b, 3.0)})

    a, b = 9.0, 21.0
    # the staging boundary of the offsets kernel (512 persons a round): unlabelled fillers with garbage coordinates in
    # front, the tied pair at indices 511 and 512; the earlier one is below min_jscale, so the keypoint scale is NaN
    for k in range(511):
        p = np.zeros((17, 4), np.float32)
        p[:, 0], p[:, 1], p[:, 3] = (np.arange(17) * 7 + k) % in_w, (np.arange(17) * 5 + k) % in_h, 1 + k % 8
        rows.append(p)
    tied_pair(5, 5, (a, b), (b, a), 0.999, 5.0)
    assert len(rows) == 513
    # the same pair in both person orders, windows apart from each other (fill 7 = cells c-3 .. c+3)
    tied_pair(14, 5, (a, b), (b, a), 0.999, 5.0)
    tied_pair(24, 5, (b, a), (a, b), 0.999, 5.0)
    tied_pair(5, 14, (a, b), (b, a), 5.0, 0.999, fr=12, to=14)
    # jitter ties (fill 4: cells c-2 .. c+1 round a keypoint): the same channel in person order, and across channels
    # (channel-major: the lower channel keeps the tie although its person comes later)
    cx, cy = centre(14, 10)
    person(k0=(cx + 1, cy + 3, 2.0))
    person(k0=(cx + 3, cy + 1, 2.0))
    cx, cy = centre(24, 10)
    person(k4=(cx + 1, cy + 3, 2.0))
    person(k3=(cx + 3, cy + 1, 2.0))
    # two identical persons (all joints annotated)
    twin = random_joints(5, 1, 96)[0]
    twin[:, 2] = 1
    rows += [twin, twin.copy()]
    # the last limb from a joint decides its scale map: (5, 6) gives 6.0, then (5, 7) of a person below min_jscale
    # makes it NaN over the earlier limb's valid value; and the other way round ((11, 12) NaN, then (11, 13) valid)
    cx, cy = centre(5, 20)
    person(k5=(cx, cy, 6.0), k6=(cx + 10, cy, 6.0))
    person(k5=(cx, cy, 0.5), k7=(cx, cy + 10, 6.0))
    cx, cy = centre(14, 20)
    person(k11=(cx, cy, 0.5), k12=(cx + 10, cy, 6.0))
    person(k11=(cx, cy, 6.0), k13=(cx, cy + 10, 6.0))
    # window edges on exact halves: x / 4 -+ 3.5 (scale fill 7) for x = 4 k, x / 4 -+ 2 (jitter fill 4) for x = 4 k + 2 and
    # x / 4 -+ 6 (Gaussian window 12) for x = 4 k + 2, with even and odd integer parts; rint goes to the even neighbour
    for k, (x, y) in enumerate(((88, 60), (92, 64), (90, 62), (94, 66), (100, 84), (104, 88), (102, 86), (106, 90))):
        person(**{'k6': (x, y, 1.0 + k), 'k8': (x + 6.0, y - 10.0, 2.0)})
    # windows that end at x_max == 0 (empty), x_max < 0 (skipped) and x_min >= out_w, for each of the three window sizes,
    # in x and in y; the to-joints are inside the image
    for v in (-8.0, -14.0, -24.0, -30.0, -40.0, -9.0, -15.0, -25.0):
        person(k13=(v, 40.0, 2.0), k15=(20.0, 44.0, 2.0))
        person(k14=(60.0, v, 2.0), k16=(64.0, 20.0, 2.0))
    for v in (6.0, 14.0, 22.0, 40.0):
        person(k13=(in_w + v, 50.0, 2.0), k15=(in_w - 20.0, 54.0, 2.0))
        person(k14=(70.0, in_h + v, 2.0), k16=(74.0, in_h - 20.0, 2.0))
    return np.stack(rows).astype(np.float32)


def cases():
    """name -> (joints, params)."""
    out = {}

    def add(name, seed, persons, in_w, in_h, keep=1.0, **kw):
        prm = dict(DEFAULTS, in_w=in_w, in_h=in_h, **kw)
        out[name] = (joints_wh(seed, persons, in_w, in_h, prm['min_jscale'], keep), prm)

    add('nonsquare', 21, 9, 200, 136)                                                  # 50 x 34 cells: a tail block
    add('omp44', 22, 5, 96, 72, head='omp44')                                          # 24 x 18
    add('omp16_s8', 23, 8, 256, 192, head='omp16', stride=8, sigma=9, clip=0.05, fill_jitter=4, fill_scale=8,
        min_jscale=4.0)
    add('omp25_s2', 24, 6, 96, 64, head='omp25', stride=2, sigma=5, fill_jitter=2, fill_scale=6, min_jscale=2.5)
    add('omp31_odd', 25, 7, 120, 88, head='omp31', clip=0.002, fill_jitter=5, fill_scale=5)
    add('crowd1100', 26, 1100, 64, 48, keep=0.12)                                      # > 1020: heat-map round 2
    add('crowd700', 27, 700, 72, 40, keep=0.15, head='omp16', fill_jitter=4, fill_scale=6, min_jscale=2.5)
    out['planted'] = (planted(), dict(DEFAULTS, in_w=128, in_h=96, fill_jitter=4))
    return out


def reference_outputs(gens, j, prm):
    HeatMapGenerator, OffsetMapGenerator = gens
    meta = {'joint_num': 17}
    size = [prm['in_w'], prm['in_h']]
    hg = HeatMapGenerator(size, prm['stride'], prm['fill_jitter'], prm['sigma'], prm['clip'])
    og = OffsetMapGenerator(size, prm['stride'], prm['fill_scale'], prm['min_jscale'], SKELETONS[prm['head']])
    off, sc, ps = og.create_offsetmaps(j, meta)
    return hg.create_heatmaps(j, meta), hg.create_jitter_offset(j, meta), off, sc, ps


def oracle_outputs(j, prm):
    hm = oracle.encode_heatmaps(j, prm['in_w'], prm['in_h'], prm['stride'], prm['sigma'], prm['clip'])
    jit = oracle.encode_jitter(j, prm['in_w'], prm['in_h'], prm['stride'], prm['fill_jitter'])
    off, sc, ps = oracle.encode_offsets(j, SKELETONS[prm['head']], cd.COCO_PERSON_SIGMAS, prm['in_w'], prm['in_h'],
                                        prm['stride'], prm['fill_scale'], prm['min_jscale'])
    return hm, jit, off, sc, ps


def check_planted(j, prm):
    """The planted inputs do what they were planted for: reversing the persons changes offsets, scales and jitter at
    the tied cells (a `<=` would show), and the scale of the tied cells follows the earlier person."""
    _, jit, off, sc, _ = oracle_outputs(j, prm)
    _, r_jit, r_off, r_sc, _ = oracle_outputs(j[::-1], prm)
    limb = cd.COCO_PERSON_SKELETON.index((5, 7))
    for i, first in ((5, (9.0, 21.0)), (14, (9.0, 21.0)), (24, (21.0, 9.0))):
        assert (off[2 * limb, 5, i], off[2 * limb + 1, 5, i]) == first, (i, off[2 * limb:2 * limb + 2, 5, i])
        assert (r_off[2 * limb, 5, i], r_off[2 * limb + 1, 5, i]) == first[::-1]
        assert np.isnan(sc[5, 5, i]) and r_sc[5, 5, i] == 5.0
    assert sc[12, 14, 5] == 5.0 and np.isnan(r_sc[12, 14, 5])
    assert (jit[0, 10, 14], jit[1, 10, 14]) == (1.0, 3.0) and (r_jit[0, 10, 14], r_jit[1, 10, 14]) == (3.0, 1.0)
    assert (jit[0, 10, 24], jit[1, 10, 24]) == (3.0, 1.0) == (r_jit[0, 10, 24], r_jit[1, 10, 24])   # channel 3 before channel 4
    assert np.isnan(sc[5, 20, 5]) and sc[11, 20, 14] == 6.0


def main():
    gens = load_reference_generators()
    out = {'cases': np.array(list(cases()))}
    for name, (j, prm) in cases().items():
        ref = reference_outputs(gens, j, prm)
        got = oracle_outputs(j, prm)
        # offsets / scales / jitter: bit-exact.  heatmaps: numpy's SIMD float32 exp vs libm expf differ by <= 2 ulp, and a
        # pixel whose value sits at the clip threshold may fall on the other side of it (at most 2 per stored case)
        assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]), name
        assert np.array_equal(got[3], ref[3], equal_nan=True) and np.array_equal(got[4], ref[4]), name
        d = np.abs(got[0] - ref[0])
        clipped = (np.minimum(got[0], ref[0]) == 0) & (np.maximum(got[0], ref[0]) < prm['clip'] * (1 + 1e-5))
        worst = float(d[~clipped].max()) if (~clipped).any() else 0.0
        edge = int((clipped & (d > 0)).sum())
        assert worst <= 1e-6 and edge <= 2, (name, worst, edge)
        sc = j[:, :, 3][j[:, :, 2] > 0]
        if prm['min_jscale'] > 1:
            assert (sc < prm['min_jscale']).any() and (sc == prm['min_jscale']).any() and (sc > prm['min_jscale']).any(), name
        if name == 'planted':
            check_planted(j, prm)
        if j.shape[0] > 512:    # persons past the first staging round of the offsets kernel decide cells
            cut = oracle_outputs(j[:512], prm)
            assert not np.array_equal(cut[2], got[2]) and not np.array_equal(cut[3], got[3], equal_nan=True), name
        if j.shape[0] > 1020:   # ... and past the first round of the heat-map kernel
            assert not np.array_equal(oracle_outputs(j[:1020], prm)[0], got[0]), name
        print(f"case {name}: P={j.shape[0]} {prm['in_w']}x{prm['in_h']} stride {prm['stride']} {prm['head']}: hm max err "
              f"{worst:.2e}, {edge} clip-edge pixels, offsets/scales/jitter bit-exact; {int(np.isfinite(ref[2]).sum())} "
              f"finite offsets, {int(np.isfinite(ref[3]).sum())} finite scales, {int((ref[0] > 0).sum())} heat-map cells")
        out[f'{name}_joints'] = j
        out[f'{name}_head'] = np.array(prm['head'])
        for k in PARAMS:
            out[f'{name}_{k}'] = np.float64(prm[k]) if k in ('clip', 'min_jscale') else np.int64(prm[k])
        for k, v in zip(('hm', 'jitter', 'off', 'scale', 'pscale'), ref):
            out[f'{name}_{k}'] = np.ascontiguousarray(v)
    path = os.path.join(GOLD, 'encoder_sweep.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= os.path.getsize(os.path.join(GOLD, 'grouping_adversarial.npz')), size   # the largest fixture so far
    print(f'{path}: {size} bytes')


if __name__ == '__main__':
    main()
