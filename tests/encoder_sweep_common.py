"""Shared by tests/test_encoder_sweep.py (CPU) and tests/test_gpu_encoder.py: the sweep fixture of the ground-truth encoder
(tests/golden/encoder_sweep.npz, tools/gen_golden_encoder_sweep.py), the oracle called with a case's parameters, and the
seeded configurations of the fuzz test."""
import os

import numpy as np

import oracle
from offsetguided_amd import synth
from offsetguided_amd.config import coco_data as cd
from helpers import GOLDEN

SWEEP_CASES = ["nonsquare", "omp44", "omp16_s8", "omp25_s2", "omp31_odd", "crowd1100", "crowd700", "planted"]
PARAMS = ("in_w", "in_h", "stride", "sigma", "clip", "fill_jitter", "fill_scale", "min_jscale")
HEADS = ["omp", "omp16", "omp31", "omp44", "omp25"]
CANARY = -12345.0      # no encoder output can hold it: heat maps / background are in [0, 1], the rest is compared bit for bit


def load_sweep():
    return np.load(os.path.join(GOLDEN, "encoder_sweep.npz"))


def case_params(g, case):
    prm = {k: (float if k in ("clip", "min_jscale") else int)(g[f"{case}_{k}"]) for k in PARAMS}
    prm["head"] = str(g[f"{case}_head"])
    return prm


def skeleton_of(head):
    from offsetguided_amd.decoder.factory import parse_heads
    return parse_heads(head, 4)["skeleton"]


def oracle_outputs(j, prm):
    """(hm, jitter, off, scale, pscale) of one image's persons from the C oracle."""
    hm = oracle.encode_heatmaps(j, prm["in_w"], prm["in_h"], prm["stride"], prm["sigma"], prm["clip"])
    jit = oracle.encode_jitter(j, prm["in_w"], prm["in_h"], prm["stride"], prm["fill_jitter"])
    off, sc, ps = oracle.encode_offsets(j, skeleton_of(prm["head"]), cd.COCO_PERSON_SIGMAS, prm["in_w"], prm["in_h"],
                                        prm["stride"], prm["fill_scale"], prm["min_jscale"])
    return hm, jit, off, sc, ps


def heatmap_figures(got, ref, clip):
    """(worst |got - ref| away from the clip edge, cells that sit on the other side of the clip threshold): the two figures
    test_encoder.heatmaps_match bounds by 1e-6 and 2."""
    d = np.abs(got - ref)
    edge = (np.minimum(got, ref) == 0) & (np.maximum(got, ref) < clip * (1 + 1e-5))
    return (float(d[~edge].max()) if (~edge).any() else 0.0), int((edge & (d > 0)).sum())


# ---- seeded fuzz configurations ---------------------------------------------------------------------------------------
FUZZ_SEEDS = list(range(40))
# (w, h) output grids the seeds walk through first: 1, 255, 256 and 257 cells (one block less a thread, one full block, one block
# and one live thread in the tail), then grids drawn at random
EDGE_GRIDS = [(1, 1), (17, 15), (255, 1), (16, 16), (32, 8), (257, 1), (1, 257), (3, 85)]


def fuzz_joints(rng, persons, in_w, in_h, stride, min_jscale):
    """(P,17,4) fp32 [x, y, v, scale] on quarter pixels (window edges land on exact halves), people partly outside the input,
    a fifth of the joints unlabelled with their coordinates left in place, a fifth of the scales exactly on min_jscale; every
    fourth person is a copy of the one before it with other scales (an exact tie in every cell the two cover)."""
    u = lambda n, lo, hi: rng.uniform(n, lo, hi)  # noqa: E731
    reach = max(in_w, in_h) / 2 + 4 * stride
    cx, cy = u(persons, -3 * stride, in_w + 3 * stride), u(persons, -3 * stride, in_h + 3 * stride)
    ext = u(persons, stride, reach)
    j = np.zeros((persons, 17, 4), np.float32)
    j[:, :, 0] = cx[:, None] + u(persons * 17, -1, 1).reshape(persons, 17) * ext[:, None]
    j[:, :, 1] = cy[:, None] + u(persons * 17, -1, 1).reshape(persons, 17) * ext[:, None]
    j[:, :, :2] = np.round(j[:, :, :2] * 4) / 4
    j[:, :, 2] = (u(persons * 17, 0, 1) > 0.2).reshape(persons, 17) * np.round(u(persons * 17, 0.51, 2.49)).reshape(persons, 17)
    j[:, :, 3] = u(persons * 17, 0.2, 3 * min_jscale).reshape(persons, 17)
    j[:, :, 3] = np.where(u(persons * 17, 0, 1).reshape(persons, 17) < 0.2, np.float32(min_jscale), j[:, :, 3])
    for p in range(3, persons, 4):
        j[p, :, :3] = j[p - 1, :, :3]
    return j


def fuzz_config(seed):
    """-> (prm, [joints of image 0, joints of image 1, ...]) for a seed: the whole parameter space of the encoder flags, input
    sizes that are not multiples of the stride, batches of mixed person counts."""
    rng = synth.HashRng(9000 + seed)
    pick = lambda seq: seq[int(rng.integers(1, 0, len(seq) - 1)[0])]  # noqa: E731
    stride = pick([2, 4, 8])
    w, h = EDGE_GRIDS[seed] if seed < len(EDGE_GRIDS) else (int(rng.integers(1, 1, 40)[0]), int(rng.integers(1, 1, 40)[0]))
    prm = dict(in_w=w * stride + int(rng.integers(1, 0, stride - 1)[0]), in_h=h * stride + int(rng.integers(1, 0, stride - 1)[0]),
               stride=stride, sigma=int(rng.integers(1, 2, 10)[0]), clip=pick([0.002, 0.01, 0.05, 0.2]),
               fill_jitter=int(rng.integers(1, 1, 9)[0]), fill_scale=int(rng.integers(1, 1, 9)[0]),
               min_jscale=pick([1.0, 2.5, 4.0]), head=pick(HEADS))
    counts = [pick([0, 1, 2, 5, 13, 40]) for _ in range(int(rng.integers(1, 2, 4)[0]))]
    if w * h <= 300 and seed % 3 == 0:      # past the staging rounds of the offsets (512) and heat-map (1020) kernels
        counts[0] = pick([512, 513, 700, 1020, 1021, 1100])
    return prm, [fuzz_joints(rng, n, prm["in_w"], prm["in_h"], stride, prm["min_jscale"]) for n in counts]
