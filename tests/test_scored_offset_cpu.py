"""scored_off without a GPU: the command-line switch, the fixtures against the CPU formulation (a drifted generator is told apart
from a parity failure), and the summation contract the HIP kernels are written against, spelled out as a numpy loop."""
import numpy as np
import pytest
import torch

from offsetguided_amd import evaluate, synth
from offsetguided_amd.config import coco_data as cd
from offsetguided_amd.decoder.offset import pack_jtypes, scored_offset
from helpers import GOLDEN, flip_tables, sha


def test_cli_switch_parses_and_defaults_to_false():
    assert evaluate.evaluate_cli(['--no-pretrain']).scored_off is False
    assert evaluate.evaluate_cli(['--no-pretrain', '--scored-off']).scored_off is True
    assert evaluate.evaluate_cli(['--no-pretrain', '--scored-off', '--flip-test', '--test-scales', '0.5', '1']).scored_off is True


def test_scored_fn_fixture_is_the_cpu_formulation():
    from tools.gen_golden_scored import FN_KS, FN_SHAPES, fn_inputs
    g = np.load(f"{GOLDEN}/scored_fn.npz")
    assert [tuple(s) for s in g["shapes"]] == FN_SHAPES and list(g["ks"]) == FN_KS
    jf, jt = pack_jtypes(cd.COCO_PERSON_SKELETON)
    for i, shape in enumerate(FN_SHAPES):
        hm, off = fn_inputs(shape, 700 + 10 * i)
        assert [sha(hm), sha(off)] == list(g[f"in_sha_{i}"]), "synthetic input generator drifted (not a parity failure)"
        assert (hm < 0).any() and not hm[:, 5].any()
        for ks in FN_KS:
            out = scored_offset(torch.from_numpy(hm), torch.from_numpy(off), jf, jt, kernel_size=ks).numpy()
            assert sha(out) == str(g[f"sha_{i}_k{ks}"])


def test_scored256_flip_fixture_is_the_cpu_formulation_on_the_merged_maps():
    g = np.load(f"{GOLDEN}/scored256_flip.npz")
    hm, off = synth.synth_batch(int(g["seed"]), int(g["batch"]), int(g["size"]), int(g["size"]), flip=True,
                                n_persons=int(g["n_persons"]))
    assert [sha(hm), sha(off)] == list(g["in_sha"]), "synthetic input generator drifted (not a parity failure)"
    assert all(n >= 3 for n in g["n_poses"]) and g["poses"].shape == (int(g["n_poses"].sum()), 17, 6)
    # flip_augment (reference decoder/factory.py:98-146, the averaged form) restated on numpy
    kp, perm, rev = flip_tables()
    n = len(hm) // 2
    m_hm = (hm[:n] + hm[n:, :, :, ::-1][:, kp]) / np.float32(2)
    o = off.reshape(2 * n, -1, 2, *off.shape[2:])
    fl = o[n:, :, :, :, ::-1].copy()
    fl[:, :, 0] *= np.float32(-1)
    m = (o[:n] + fl[:, perm]) / np.float32(2)
    m[:, rev] = o[:n, rev]
    m_off = np.ascontiguousarray(m.reshape(n, -1, *off.shape[2:]))
    jf, jt = pack_jtypes(cd.COCO_PERSON_SKELETON)
    out = scored_offset(torch.from_numpy(np.ascontiguousarray(m_hm)), torch.from_numpy(m_off), jf, jt, kernel_size=3).numpy()
    assert sha(out) == str(g["scored_sha"])


def loop_formulation(hm, off, jf, ks):
    """The contract: products rounded to fp32 before any sum; num and den start at +0 and add the in-bounds cells of the window
    row-major (y' outer, x' inner), one after the other, in fp32; out = num / (den + 1e-6f), a correctly rounded divide."""
    n, _, h, w = hm.shape
    p = (ks - 1) // 2
    out = np.empty_like(off)
    f32 = np.float32
    with np.errstate(all='ignore'):
        for i in range(n):
            for l, j in enumerate(jf):
                prod = [(hm[i, j] * off[i, 2 * l + c]).astype(f32) for c in (0, 1)]
                for y in range(h):
                    for x in range(w):
                        den, num = f32(0), [f32(0), f32(0)]
                        for yy in range(max(y - p, 0), min(y + p, h - 1) + 1):
                            for xx in range(max(x - p, 0), min(x + p, w - 1) + 1):
                                den = f32(den + hm[i, j, yy, xx])
                                num = [f32(num[c] + prod[c][yy, xx]) for c in (0, 1)]
                        for c in (0, 1):
                            out[i, 2 * l + c, y, x] = f32(num[c] / f32(den + f32(1e-6)))
    return out


@pytest.mark.parametrize("ks", [3, 5, 7])
def test_row_major_sequential_sum_is_the_cpu_formulation(ks):
    skel = cd.COCO_PERSON_SKELETON[:4]
    jf, jt = pack_jtypes(skel)
    hm = synth.noise_batch(3, (2, 17, 9, 13), 0.3)
    hm[:, jf[1]] = 0.0
    off = synth.noise_batch(4, (2, 2 * len(skel), 9, 13), 4.0)
    exp = scored_offset(torch.from_numpy(hm), torch.from_numpy(off), jf, jt, kernel_size=ks).numpy()
    got = loop_formulation(hm, off, jf, ks)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
