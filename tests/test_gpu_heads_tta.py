"""GPU: the keypoint-scale and jitter-offset heads on HIP under flip-test and --test-scales, and hmp_NMS windows 5 / 7.

  * og_flip_merge_heads_f32 == the reference's torch ops (decoder/factory.py:108-113, :141-144), torch.equal, on the inputs of the
    committed one-head fixtures and on heads_flip.npz (both heads, targets computed by the imported reference); the poses match the
    fixtures with torch.flip / max_pool2d / pad made to raise -- no torch op is left on those routes;
  * the folded flip route (og_generate_limbs_fused_flip_heads_f32) == the unfolded one, limbs torch.equal;
  * og_scale_accumulate_heads_f32 == the float32 numpy restatement of tests/test_heads_tta_cpu.py, np.array_equal; identity; units;
    run_images with both heads over three scales; graph replay == eager.
No tolerance is introduced here: scores are held to the project's 1e-4 where the fixtures are, everything else is exact."""
import argparse

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import GOLDEN, assert_poses_match, jitter_case_inputs, scale_case_inputs, sha, split_poses
from offsetguided_amd import _lib, decoder, evaluate, models, synth
from offsetguided_amd.config import coco_data as cd
from offsetguided_amd.decoder import multiscale
from test_heads_tta_cpu import IDENTITY, np_flip_heads, np_merge_heads
from tools.gen_golden_heads_flip import FLAGS as HF_FLAGS, heads_flip_inputs

pytestmark = pytest.mark.gpu
F32 = np.float32
SCORE_TOL = 1e-4
KP_PERM = cd.heatmap_hflip(cd.COCO_KEYPOINTS)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    _lib.load()
    return torch.device("cuda:0")


def make_proc(batch, topk=32, dist_max=40.0, include_scale=True, include_jitter=True, use_scale=True):
    p = argparse.ArgumentParser()
    decoder.decoder_cli(p)
    a = p.parse_args(['--topk', str(topk), '--thre-hmp', '0.04', '--person-thre', '0.04', '--dist-max', str(dist_max), '--min-len', '0.5',
                      '--use-scale', str(use_scale), '--use-jitter-offset', 'True'])
    a.headnets, a.strides, a.batch_size = ['hmp', 'omp'], [4, 4], batch
    a.include_scale, a.include_jitter_offset = include_scale, include_jitter
    return decoder.decoder_factory(a)


def feats_of(dev, hm, off, scl=None, jit=None):
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    return [([None, t(hm)], [[], []], [None, t(jit)] if jit is not None else [[], []]),
            ([None, t(off)], [[], []], [None, t(scl)] if scl is not None else [[], []])]


def torch_flip_heads(scl, jit):
    """The torch ops flip_augment ran before (and the reference runs), on CPU tensors."""
    so = jo = None
    if scl is not None:
        n = scl.shape[0] // 2
        so = (scl[:n] + torch.flip(scl[n:], [-1])[:, KP_PERM]) / 2
    if jit is not None:
        n = jit.shape[0] // 2
        fl = torch.flip(jit[n:], [-1])
        fl[:, ::2] *= -1
        jo = (jit[:n] + fl) / 2
    return so, jo


def forbid_torch_ops(monkeypatch):
    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f'{name} called: a torch op is left on the decoder route')
        return f
    monkeypatch.setattr(torch, 'flip', refuse('torch.flip'))
    monkeypatch.setattr(F, 'max_pool2d', refuse('F.max_pool2d'))
    monkeypatch.setattr(F, 'pad', refuse('F.pad'))


# ---------------------------------------------------------------------------------- 1. flip merge of the heads
def test_flip_merge_heads_on_the_one_head_fixtures(dev, monkeypatch):
    """scale256_flip / jitter256_flip (fixtures from the imported reference, one head each): the kernel == the torch-op merge on their
    inputs, and the poses match the fixtures with the torch ops unreachable."""
    gs, gj = np.load(f"{GOLDEN}/scale256_flip.npz"), np.load(f"{GOLDEN}/jitter256_flip.npz")
    hm_s, off_s, scl = scale_case_inputs(gs)
    hm_j, off_j, jit = jitter_case_inputs(gj)
    exp_s, _ = torch_flip_heads(torch.from_numpy(scl), None)
    _, exp_j = torch_flip_heads(None, torch.from_numpy(jit))
    forbid_torch_ops(monkeypatch)
    ps = make_proc(int(gs["batch"]), dist_max=6.0, include_jitter=False)
    pj = make_proc(int(gj["batch"]), include_scale=False)
    t = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
    _, _, _, got_s, _ = ps.flip_augment(t(hm_s), [], t(off_s), t(scl), False, 2)
    _, got_j, _, _, _ = pj.flip_augment(t(hm_j), t(jit), t(off_j), [], False, 2)
    assert torch.equal(got_s.cpu(), exp_s) and torch.equal(got_j.cpu(), exp_j)
    for fold in (True, False):
        ps.fold_flip = pj.fold_flip = fold
        assert_poses_match(split_poses(gs), ps.generate_poses(feats_of(dev, hm_s, off_s, scl=scl), flip_test=True), SCORE_TOL)
        assert_poses_match(split_poses(gj), pj.generate_poses(feats_of(dev, hm_j, off_j, jit=jit), flip_test=True), SCORE_TOL)


def heads_flip_case():
    g = np.load(f"{GOLDEN}/heads_flip.npz", allow_pickle=False)
    hm, off, scl, jit = heads_flip_inputs(int(g["seed"]), int(g["batch"]), int(g["size"]), int(g["n_persons"]))
    assert [sha(hm), sha(off), sha(scl), sha(jit)] == list(g["in_sha"]), "synthetic input generator drifted (not a parity failure)"
    return g, hm, off, scl, jit


def test_flip_merge_heads_both_heads_against_the_reference(dev):
    """heads_flip.npz: both heads in one launch == the reference's flip_augment outputs, bit for bit; one head at a time as well."""
    g, hm, off, scl, jit = heads_flip_case()
    proc = make_proc(int(g["batch"]), dist_max=HF_FLAGS['dist_max'])
    t = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
    _, got_j, _, got_s, _ = proc.flip_augment(t(hm), t(jit), t(off), t(scl), False, 2)
    assert np.array_equal(got_s.cpu().numpy(), g["scmps_merged"]) and np.array_equal(got_j.cpu().numpy(), g["jomps_merged"])
    _, none_j, _, only_s, _ = proc.flip_augment(t(hm), [], t(off), t(scl), False, 2)
    assert none_j == [] and np.array_equal(only_s.cpu().numpy(), g["scmps_merged"])
    _, only_j, _, none_s, _ = proc.flip_augment(t(hm), t(jit), t(off), [], False, 2)
    assert none_s == [] and np.array_equal(only_j.cpu().numpy(), g["jomps_merged"])


# ---------------------------------------------------------------------------------- 2. no torch op left
@pytest.mark.parametrize("fold", [True, False])
def test_no_torch_op_left_with_both_heads(dev, monkeypatch, fold):
    """generate_poses(flip_test=True) with both heads and use_scale=True == the reference's poses (heads_flip.npz) while torch.flip,
    max_pool2d and pad raise."""
    g, hm, off, scl, jit = heads_flip_case()
    proc = make_proc(int(g["batch"]), dist_max=HF_FLAGS['dist_max'])
    proc.fold_flip = fold
    forbid_torch_ops(monkeypatch)
    poses = proc.generate_poses(feats_of(dev, hm, off, scl, jit), flip_test=True)
    assert all(len(p) >= 1 for p in poses)
    assert_poses_match(split_poses(g), poses, SCORE_TOL)
    for r, m in zip(split_poses(g), poses):
        assert (r[..., 3] == m[..., 3]).all()          # the scale column comes straight from the merged, sampled maps


def nms_reference(heat, kernel):
    pad = (kernel - 1) // 2
    return heat * (F.max_pool2d(F.pad(heat, [pad] * 4), (kernel, kernel), stride=1) == heat).float()


@pytest.mark.parametrize("kernel", [5, 7])
def test_hmp_nms_windows_5_and_7_on_hip(dev, monkeypatch, kernel):
    """The torch-CPU formula of test_hmp_nms_other_windows on its input (plateau, negative plane) and on a plane wider and taller than
    a workgroup's 64 x 16 tile (plateaus and peaks across the tile borders), sign bits included, with the torch ops unreachable."""
    g = torch.Generator().manual_seed(kernel)
    heat = torch.randn(2, 3, 37, 53, generator=g)
    heat[0, 0, 5:9, 5:9] = 2.0
    heat[1, 1] = -heat[1, 1].abs()
    wide = torch.randn(1, 2, 45, 200, generator=g)
    wide[0, 0, 14:18, 60:68] = 3.0                  # a plateau over the corner of four tiles
    wide[0, 1] = -wide[0, 1].abs()
    wide[0, 1, 15, 63] = -0.0
    cases = [(x, nms_reference(x, kernel)) for x in (heat, wide)]
    forbid_torch_ops(monkeypatch)
    for x, ref in cases:
        got = decoder.hmp_NMS(x.to(dev), kernel).cpu()
        assert torch.equal(got, ref) and torch.equal(torch.signbit(got), torch.signbit(ref))


# ---------------------------------------------------------------------------------- 3. folded == unfolded
def limbs_both_routes(dev, proc, feats, scored_off):
    out = []
    for fold in (True, False):
        proc.fold_flip = fold
        stages = {}
        _lib.profile_start()
        try:
            limbs = proc.generate_limbs(feats, flip_test=True, scored_off=scored_off)
            torch.cuda.synchronize()
        finally:
            stages = _lib.profile_stop()
        out.append((limbs, set(stages)))
    return out


@pytest.mark.parametrize("scored_off", [False, True])
@pytest.mark.parametrize("topk", [32, 48])
def test_folded_equals_unfolded_square_both_heads(dev, topk, scored_off):
    hm, off, scl, jit = heads_flip_inputs(31 + topk, 3, 256, 7)
    proc = make_proc(3, topk=topk)
    (folded, st_f), (unfolded, st_u) = limbs_both_routes(dev, proc, feats_of(dev, hm, off, scl, jit), scored_off)
    assert 'k0_flip_merge' not in st_f and 'k0_flip_merge_heads' not in st_f, st_f       # the folded route ran no merge pass
    assert {'k0_flip_merge', 'k0_flip_merge_heads'} <= st_u, st_u
    assert torch.equal(folded, unfolded)
    # each head alone takes the heads form as well
    for kw in (dict(scl=scl), dict(jit=jit)):
        (a, _), (b, _) = limbs_both_routes(dev, proc, feats_of(dev, hm, off, **kw), scored_off)
        assert torch.equal(a, b)


@pytest.mark.parametrize("scored_off", [False, True])
def test_folded_equals_unfolded_non_square_scale_head(dev, scored_off):
    """A non-square input with the scale head only (the jitter head needs square inputs, decoder/collect.py:158)."""
    rng_hm, rng_off = synth.synth_batch(77, 2, 192, 320, flip=True, n_persons=6)
    scl = (synth.noise_batch(82, (4, 17, 48, 80)) * 20 + 25).astype(F32)
    proc = make_proc(2, include_jitter=False)
    (a, st_f), (b, _) = limbs_both_routes(dev, proc, feats_of(dev, rng_hm, rng_off, scl=scl), scored_off)
    assert 'k0_flip_merge' not in st_f and torch.equal(a, b)
    jit = ((synth.noise_batch(83, (4, 2, 48, 80)) - 0.5) * 3.0).astype(F32)
    pj = make_proc(2)
    for fold in (True, False):
        pj.fold_flip = fold
        with pytest.raises(NotImplementedError, match='square'):
            pj.generate_limbs(feats_of(dev, rng_hm, rng_off, scl, jit), flip_test=True)


def test_folded_falls_back_above_its_lds_limit(dev):
    """topk 240 at 640 x 640 does not fit the merge-and-pair stage of the folded form (OG_EUNSUPPORTED): the unfolded route is taken,
    not an error, with the same limbs as fold_flip=False."""
    hm, off, scl, jit = heads_flip_inputs(5, 1, 640, 10)
    proc = make_proc(1, topk=240)
    with pytest.raises(_lib.OgError, match=f'code {_lib.OG_EUNSUPPORTED}'):
        proc.limb_collect.generate_limbs_fused_flip(*[torch.from_numpy(x).to(dev) for x in (hm, off)], KP_PERM, proc.limbs_flips[0],
                                                    [1 if l in proc.limbs_flips[1] else 0 for l in range(19)],
                                                    scmps_pair_lr=torch.from_numpy(scl).to(dev), jomps_pair_lr=torch.from_numpy(jit).to(dev))
    (a, st_f), (b, _) = limbs_both_routes(dev, proc, feats_of(dev, hm, off, scl, jit), False)
    assert 'k0_flip_merge_heads' in st_f, st_f
    assert torch.equal(a, b)


def test_folded_bilinear_scale_sampling_through_the_c_entry(dev):
    """scales_mode 3 of the heads form (PostProcess folds only with the bicubic resize): == merge passes + og_generate_limbs_fused_f32
    with the bilinear scale sampling."""
    hm, off, scl, jit = heads_flip_inputs(9, 2, 256, 6)
    proc = make_proc(2)
    lc = proc.limb_collect
    t = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
    keep = [1 if l in proc.limbs_flips[1] else 0 for l in range(19)]
    a = lc.generate_limbs_fused_flip(t(hm), t(off), KP_PERM, proc.limbs_flips[0], keep, scmps_pair_lr=t(scl), scale_inter='bilinear',
                                     jomps_pair_lr=t(jit))
    mh, mj, mo, ms, _ = proc.flip_augment(t(hm), t(jit), t(off), t(scl), False, 2)
    b = lc.generate_limbs_fused(mh, mo, 2, ms, 'bilinear', mj)
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------- 4. multi-scale with the heads
def dev_maps4(seed, n, C, L, hs, ws):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, C, hs, ws, generator=g), torch.randn(n, 2 * L, hs, ws, generator=g) * 8,
            torch.rand(n, C, hs, ws, generator=g) * 40 + 5, torch.randn(n, 2, hs, ws, generator=g) * 1.5)


def random_affines(seed, N, hs, ws, h, w):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(N):
        ax, ay = (ws - 1) / max(w - 1, 1) * rng.uniform(0.9, 1.1), (hs - 1) / max(h - 1, 1) * rng.uniform(0.9, 1.1)
        rows.append([ax, rng.uniform(-1.5, 1.5), ay, rng.uniform(-1.5, 1.5), 1 / ax, 1 / ay])
    return np.array(rows, F32)


def test_merge_scales_takes_four_tuples(dev):
    """(a) merge_scales with (hm, off, scl, jit) over three scales returns the maps, in the reference nesting."""
    N, C, L = 2, 17, 19
    sizes = [(12, 16), (24, 32), (36, 48)]
    outs = [dev_maps4(s, 2 * N, C, L, *hw) for s, hw in enumerate(sizes)]
    affs = [random_affines(5 + s, N, *hw, 24, 32) for s, hw in enumerate(sizes)]
    feats = multiscale.merge_scales([tuple(x.to(dev) for x in o) for o in outs], affs, True, base_hw=(24, 32))
    es, ej = np_merge_heads([(o[2].numpy(), o[3].numpy()) for o in outs], affs, 24, 32, True)
    assert np.array_equal(feats[1][2][-1].cpu().numpy(), es) and np.array_equal(feats[0][2][-1].cpu().numpy(), ej)
    plain = multiscale.merge_scales([tuple(x.to(dev) for x in o[:2]) for o in outs], affs, True, base_hw=(24, 32))
    assert torch.equal(plain[0][0][-1], feats[0][0][-1]) and torch.equal(plain[1][0][-1], feats[1][0][-1])     # hm / off as without heads
    assert feats[0][1] == [[]] and feats[1][1] == [[]]
    only_jit = multiscale.merge_scales([(o[0].to(dev), o[1].to(dev), None, o[3].to(dev)) for o in outs], affs, True, base_hw=(24, 32))
    assert only_jit[1][2] == [[]] and np.array_equal(only_jit[0][2][-1].cpu().numpy(), ej)


KERNEL_CASES = [
    # N, (hs, ws), (h, w), flip: the (src, dst) grids of tests/test_gpu_multiscale.py
    (1, (40, 37), (20, 18), False),
    (8, (16, 24), (32, 48), False),
    (2, (33, 50), (48, 31), True),
    (8, (24, 24), (40, 40), True),
    (3, (21, 30), (16, 16), True),
    (2, (21, 30), (29, 35), False),
    (2, (33, 50), (48, 31), False),
    (1, (40, 37), (20, 18), True),
]


@pytest.mark.parametrize("N,src,dst,flip", KERNEL_CASES)
def test_heads_kernel_matches_numpy_bit_for_bit(dev, N, src, dst, flip):
    """(b) the three modes, scale and jitter accumulators == the float32 restatement, np.array_equal."""
    C, L, Fl = 17, 19, 2 if flip else 1
    (hs, ws), (h, w) = src, dst
    outs = [dev_maps4(10 * k + N, Fl * N, C, L, hs + k, ws + 2 * k) for k in range(3)]
    affs = [random_affines(k, N, hs + k, ws + 2 * k, h, w) for k in range(3)]
    nan = lambda ch: torch.full((N, ch, h, w), float('nan'), device=dev)  # noqa: E731
    acc = (nan(C), nan(2 * L), nan(C), nan(2))
    inv = float(F32(1) / F32(3))
    heads = [(o[2].numpy(), o[3].numpy()) for o in outs]
    for k, mode in enumerate((multiscale.MODE_WRITE, multiscale.MODE_ADD, multiscale.MODE_ADD_SCALE)):
        hm, off, scl, jit = (x.to(dev) for x in outs[k])
        multiscale.accumulate_scale(hm, off, torch.from_numpy(affs[k]).to(dev), acc, mode, inv, flip, scl=scl, jit=jit)
        es, ej = np_merge_heads(heads[:k + 1], affs[:k + 1], h, w, flip, last_scales=(mode != multiscale.MODE_ADD))
        torch.cuda.synchronize()
        assert np.array_equal(acc[2].cpu().numpy(), es), f'scale maps, mode {mode}'
        assert np.array_equal(acc[3].cpu().numpy(), ej), f'jitter maps, mode {mode}'
    # hm / off of the same launches == the two-map entry
    ref = (nan(C), nan(2 * L))
    for k, mode in enumerate((multiscale.MODE_WRITE, multiscale.MODE_ADD, multiscale.MODE_ADD_SCALE)):
        multiscale.accumulate_scale(outs[k][0].to(dev), outs[k][1].to(dev), torch.from_numpy(affs[k]).to(dev), ref, mode, inv, flip)
    assert torch.equal(acc[0], ref[0]) and torch.equal(acc[1], ref[1])


@pytest.mark.parametrize("flip", [False, True])
def test_base_scale_reproduces_the_heads(dev, flip):
    """(c) S = 1 with the exact identity table: the maps come back bit-identical (with flip: og_flip_merge_heads_f32's merge)."""
    N, C, L, h, w = 3, 17, 19, 20, 27
    hm, off, scl, jit = dev_maps4(7, (2 if flip else 1) * N, C, L, h, w)
    feats = multiscale.merge_scales([(hm.to(dev), off.to(dev), scl.to(dev), jit.to(dev))], [np.repeat(IDENTITY, N, 0)], flip, base_hw=(h, w))
    if flip:
        es, ej = torch_flip_heads(scl, jit)
        proc = make_proc(N)
        _, kj, _, ks, _ = proc.flip_augment(hm.to(dev), jit.to(dev), off.to(dev), scl.to(dev), False, 2)
        assert torch.equal(ks.cpu(), es) and torch.equal(kj.cpu(), ej)
    else:
        es, ej = scl, jit
    assert torch.equal(feats[1][2][-1].cpu(), es) and torch.equal(feats[0][2][-1].cpu(), ej)


def test_head_units(dev):
    """(d) constant maps at a scale that is 2x the base along x and 8x along y (inv_a = 1/2, 1/8): jitter (3, -5) -> (1.5, -0.625),
    keypoint scale 12 -> 12 * sqrt(1/16) = 3, exactly."""
    N, C, L, h, w = 2, 17, 19, 8, 24
    base = [{'offset': np.zeros(2), 'scale': np.array([1.0, 1.0])}] * N
    scaled = [{'offset': np.zeros(2), 'scale': np.array([2.0, 8.0])}] * N
    aff = multiscale.scale_affines(base, scaled, (h, w), (8 * h, 2 * w))
    assert np.array_equal(aff[:, [0, 2, 4, 5]], np.tile(F32([2, 8, 0.5, 0.125]), (N, 1)))
    hm, off = torch.rand(N, C, 8 * h, 2 * w), torch.rand(N, 2 * L, 8 * h, 2 * w)
    scl = torch.full((N, C, 8 * h, 2 * w), 12.0)
    jit = torch.empty(N, 2, 8 * h, 2 * w)
    jit[:, 0], jit[:, 1] = 3.0, -5.0
    feats = multiscale.merge_scales([tuple(x.to(dev) for x in (hm, off, scl, jit))], [aff], False, base_hw=(h, w))
    s, j = feats[1][2][-1].cpu().numpy(), feats[0][2][-1].cpu().numpy()
    assert (s == 3.0).all() and (j[:, 0] == 1.5).all() and (j[:, 1] == -0.625).all()


def _raw_loader():
    rng = np.random.default_rng(11)
    sizes = [(120, 200), (333, 250), (256, 256), (90, 64), (301, 177)]
    raw = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    return [(raw[0:2], [None] * 2, [{'image_id': 1}, {'image_id': 2}]), (raw[2:4], [None] * 2, [{'image_id': 3}, {'image_id': 4}]),
            (raw[4:5], [None], [{'image_id': 5}])]


@pytest.mark.parametrize("flip", [False, True])
def test_run_images_multi_scale_with_both_heads(dev, monkeypatch, flip):
    """(e) --test-scales 0.5 1 1.5 --include-scale --include-jitter-offset on raw uint8 images: strict engines (no torch convolution),
    every merge launch carries four maps, and the maps it decodes are the restatement's merge of the engines' head outputs."""
    torch.manual_seed(0)
    a = evaluate.evaluate_cli(['--no-pretrain', '--initialize-whole', 'False', '--topk', '32', '--thre-hmp', '0.04', '--person-thre', '0.04',
                               '--dist-max', '40', '--long-edge', '256', '--batch-size', '2', '--print-freq', '1', '--test-scales', '0.5',
                               '1', '1.5', '--include-scale', '--include-jitter-offset'] + (['--flip-test'] if flip else []))
    assert a.include_scale is True and a.include_jitter_offset is True
    model, _ = models.model_factory(a)
    seen, merged = [], []
    real = multiscale.accumulate_scale

    def spy(hm, off, aff, out, mode, inv_count, flip_test, keypoints, skeleton, scl=None, jit=None):
        assert scl is not None and jit is not None and len(out) == 4
        seen.append((scl.cpu().numpy().copy(), jit.cpu().numpy().copy(), aff.cpu().numpy().copy(), mode))
        real(hm, off, aff, out, mode, inv_count, flip_test, keypoints, skeleton, scl, jit)
        if mode == multiscale.MODE_ADD_SCALE:
            merged.append((out[2].cpu().numpy().copy(), out[3].cpu().numpy().copy()))
    monkeypatch.setattr(multiscale, 'accumulate_scale', spy)
    stats = {}
    results, ids = evaluate.run_images(a, data_loader=_raw_loader(), model=model, stats=stats)
    assert ids == [1, 2, 3, 4, 5] and len(seen) == 9 and len(merged) == 3
    assert stats['torch_conv_calls'] == 0 and stats['test_scales'] == [0.5, 1.0, 1.5]
    assert all(isinstance(r['keypoints'], list) for r in results)
    for b in range(3):
        rec = seen[3 * b:3 * b + 3]
        assert [r[3] for r in rec] == [0, 1, 2]
        es, ej = np_merge_heads([(r[0], r[1]) for r in rec], [r[2] for r in rec], 64, 64, flip)
        assert np.array_equal(merged[b][0], es) and np.array_equal(merged[b][1], ej)


def test_heads_merge_launch_replays_from_a_graph(dev):
    N, C, L, h, w = 2, 17, 19, 32, 40
    hm, off, scl, jit = [t.to(dev) for t in dev_maps4(3, 2 * N, C, L, 48, 60)]
    aff = torch.from_numpy(random_affines(9, N, 48, 60, h, w)).to(dev)
    zeros = lambda: tuple(torch.zeros(N, ch, h, w, device=dev) for ch in (C, 2 * L, C, 2))  # noqa: E731
    eager, acc = zeros(), zeros()
    multiscale.accumulate_scale(hm, off, aff, eager, multiscale.MODE_WRITE, 1.0, True, scl=scl, jit=jit)
    multiscale.accumulate_scale(hm, off, aff, eager, multiscale.MODE_ADD_SCALE, 0.5, True, scl=scl, jit=jit)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        multiscale.accumulate_scale(hm, off, aff, acc, multiscale.MODE_WRITE, 1.0, True, scl=scl, jit=jit)     # warm-up: the flip tables
    torch.cuda.current_stream(dev).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        multiscale.accumulate_scale(hm, off, aff, acc, multiscale.MODE_WRITE, 1.0, True, scl=scl, jit=jit)
        multiscale.accumulate_scale(hm, off, aff, acc, multiscale.MODE_ADD_SCALE, 0.5, True, scl=scl, jit=jit)
    for t in acc:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(acc, eager))
    assert bool(acc[2].abs().sum() > 0) and bool(acc[3].abs().sum() > 0)
