"""scored_off on HIP kernels: og_scored_offset_f32 (bit patterns of the reference's CPU result), the refinement inside the pairing
(og_generate_limbs_fused[_flip]_scored_f32: limbs bit-identical to "stand-alone kernel, then the unrefined decode"), the drop-in
surface (generate_poses / run_images --scored-off) with no torch pooling on the path."""
import argparse

import numpy as np
import pytest
import torch

from offsetguided_amd import _lib, decoder, evaluate, models, synth, transforms
from offsetguided_amd.config import coco_data as cd
from offsetguided_amd.decoder.offset import pack_jtypes, scored_offset
from helpers import FLAGS, GOLDEN, assert_poses_match, scale_case_inputs, sha, split_poses

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-4      # the project's pose limb-score tolerance (tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    _lib.load()
    return torch.device("cuda:0")


def processor(batch=2, headnet='omp', include_scale=False, **over):
    p = argparse.ArgumentParser()
    decoder.decoder_cli(p)
    f = dict(FLAGS, **over)
    a = p.parse_args(['--topk', str(f['topk']), '--thre-hmp', str(f['thre_hmp']), '--person-thre', str(f['person_thre']),
                      '--dist-max', str(f['dist_max']), '--min-len', str(f['min_len'])])
    a.headnets, a.strides, a.batch_size = ['hmp', headnet], [4, 4], batch
    a.include_scale, a.include_jitter_offset = include_scale, False
    return decoder.decoder_factory(a)


def features(hm, off, dev, scl=None):
    t = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
    return [([None, t(hm)], [[], []], [[], []]), ([None, t(off)], [[], []], [None, t(scl)] if scl is not None else [[], []])]


def scored256():
    g = np.load(f"{GOLDEN}/scored256.npz")
    hm, off = synth.synth_batch(int(g["seed"]), int(g["batch"]), int(g["size"]), int(g["size"]), n_persons=6)
    assert [sha(hm), sha(off)] == list(g["in_sha"]), "synthetic input generator drifted (not a parity failure)"
    return g, hm, off


def scored256_flip():
    g = np.load(f"{GOLDEN}/scored256_flip.npz")
    hm, off = synth.synth_batch(int(g["seed"]), int(g["batch"]), int(g["size"]), int(g["size"]), flip=True,
                                n_persons=int(g["n_persons"]))
    assert [sha(hm), sha(off)] == list(g["in_sha"]), "synthetic input generator drifted (not a parity failure)"
    return g, hm, off


def kernel(hm, off, jf, ks, dev):
    return scored_offset(torch.from_numpy(hm).to(dev), torch.from_numpy(off).to(dev), jf, None, kernel_size=ks).cpu().numpy()


# ------------------------------------------------------------------ 1. the stand-alone kernel against the reference's bit patterns
def test_kernel_reproduces_the_reference_sha(dev):
    g, hm, off = scored256()
    jf, _ = pack_jtypes(cd.COCO_PERSON_SKELETON)
    assert sha(kernel(hm, off, jf, 3, dev)) == str(g["scored_sha"])


@pytest.mark.parametrize("case", [0, 1])
@pytest.mark.parametrize("ks", [1, 5, 7])
def test_kernel_other_windows_reference_sha(dev, case, ks):
    from tools.gen_golden_scored import fn_inputs
    g = np.load(f"{GOLDEN}/scored_fn.npz")
    hm, off = fn_inputs(tuple(int(v) for v in g["shapes"][case]), 700 + 10 * case)
    assert [sha(hm), sha(off)] == list(g[f"in_sha_{case}"]), "synthetic input generator drifted (not a parity failure)"
    jf, _ = pack_jtypes(cd.COCO_PERSON_SKELETON)
    assert sha(kernel(hm, off, jf, ks, dev)) == str(g[f"sha_{case}_k{ks}"])


# ------------------------------------------------------------------ 2. ... and against the CPU formulation on many shapes
SHAPES = [(1, 1, 1), (1, 1, 2), (2, 1, 1), (1, 2, 7), (2, 7, 2), (1, 3, 3), (2, 5, 5), (1, 4, 9), (2, 6, 61), (1, 7, 61), (2, 24, 40),
          (1, 33, 37), (1, 2, 130), (1, 40, 4), (2, 9, 250), (1, 3, 300), (1, 50, 258), (1, 64, 64), (1, 23, 518)]


@pytest.mark.parametrize("ks", [1, 3, 5, 7])
def test_kernel_matches_cpu_formulation_bitwise(dev, ks):
    skel = cd.COCO_PERSON_SKELETON
    jf, jt = pack_jtypes(skel)
    for i, (n, h, w) in enumerate(SHAPES):
        hm = synth.noise_batch(40 + i, (n, 17, h, w), 0.3)
        hm[:, 3] = 0.0                                    # den = 0: 0 / 1e-6
        off = synth.noise_batch(90 + i, (n, 2 * len(skel), h, w), 4.0)
        if i % 5 == 2:                                    # non-finite cells propagate through their windows alike
            off[0, 4, h // 2, w // 2] = np.inf
            hm[0, jf[7], 0, 0] = np.nan
        exp = scored_offset(torch.from_numpy(hm), torch.from_numpy(off), jf, jt, kernel_size=ks).numpy()
        got = kernel(hm, off, jf, ks, dev)
        nan = np.isnan(exp)
        assert np.array_equal(np.isnan(got), nan), (n, h, w)
        assert np.array_equal(got.view(np.uint32)[~nan], exp.view(np.uint32)[~nan]), (n, h, w)


@pytest.mark.parametrize("skel,n,h,w", [(cd.COCO_PERSON_SKELETON, 2, 160, 160), (cd.DENSER_COCO_PERSON_SKELETON, 1, 64, 64),
                                        (cd.DENSER_COCO_PERSON_SKELETON, 2, 37, 53)])
def test_kernel_large_and_denser_skeleton(dev, skel, n, h, w):
    jf, jt = pack_jtypes(skel)
    hm = synth.noise_batch(7, (n, 17, h, w), 0.3)
    off = synth.noise_batch(8, (n, 2 * len(skel), h, w), 4.0)
    exp = scored_offset(torch.from_numpy(hm), torch.from_numpy(off), jf, jt, kernel_size=3).numpy()
    assert np.array_equal(kernel(hm, off, jf, 3, dev).view(np.uint32), exp.view(np.uint32))


@pytest.mark.parametrize("ks", [0, 2, 9, -3])
def test_kernel_refuses_other_windows(dev, ks):
    lib = _lib.load()
    hm, off = torch.zeros(1, 17, 8, 8, device=dev), torch.zeros(1, 38, 8, 8, device=dev)
    out = torch.empty_like(off)
    jf = _lib.int_table(pack_jtypes(cd.COCO_PERSON_SKELETON)[0], dev)
    rc = lib.og_scored_offset_f32(_lib.ptr(hm), _lib.ptr(off), 1, 17, 19, 8, 8, _lib.ptr(jf), ks, _lib.ptr(out), _lib.stream_ptr(dev))
    assert rc == _lib.OG_EINVAL and b"ksize" in lib.og_last_error()
    with pytest.raises(_lib.OgError, match="ksize"):
        scored_offset(hm, off, pack_jtypes(cd.COCO_PERSON_SKELETON)[0], None, kernel_size=ks)


# ------------------------------------------------------------------ 3. generate_poses(scored_off=True): golden, no torch pooling
@pytest.mark.parametrize("fused", [True, False])
def test_generate_poses_scored_golden_without_torch_pooling(dev, monkeypatch, fused):
    g, hm, off = scored256()

    def no_pooling(*a, **k):
        raise AssertionError("torch pooling on the scored_off path")
    monkeypatch.setattr(torch.nn.functional, 'avg_pool2d', no_pooling)
    proc = processor(int(g["batch"]))
    proc.fused_upsample = fused
    assert proc.scored_kernel_size == 3
    poses = proc.generate_poses(features(hm, off, dev), scored_off=True)
    assert_poses_match(split_poses(g), poses, SCORE_TOL)


# ------------------------------------------------------------------ 4. in-pairing form == stand-alone kernel + unrefined decode
def _refined_then_plain(proc, hm, off, dev, flip, scl=None):
    """The limbs of `stand-alone kernel (after K0 with flip), then the unrefined decode`."""
    thm, toff = torch.from_numpy(hm).to(dev), torch.from_numpy(off).to(dev)
    if flip:
        thm, _, toff, _, _ = proc.flip_augment(thm, [], toff, [], False, 2)
    jf, _ = pack_jtypes(proc.skeleton)
    ref_off = scored_offset(thm, toff, jf, None, kernel_size=proc.scored_kernel_size)
    t = None if scl is None else torch.from_numpy(scl).to(dev)
    if flip and t is not None:
        t = (t[:len(t) // 2] + torch.flip(t[len(t) // 2:], [-1])[:, proc.keypoints_flips]) / 2
    feats = [([None, thm], [[], []], [[], []]), ([None, ref_off], [[], []], [None, t] if t is not None else [[], []])]
    return proc.generate_limbs(feats, scored_off=False)


@pytest.mark.parametrize("case", ["plain", "flip_folded", "flip_unfolded", "topk48", "omp44", "scale256"])
def test_in_pairing_limbs_bit_identical_to_kernel_then_decode(dev, case):
    flip = case.startswith("flip")
    headnet, over, scl = 'omp', {}, None
    if case == "topk48":
        over = dict(topk=48)
    if case == "omp44":
        headnet = 'omp44'
    if case == "scale256":
        g = np.load(f"{GOLDEN}/scale256.npz")
        hm, off, scl = scale_case_inputs(g)
    else:
        skel = decoder.factory.parse_heads(headnet, 4)['skeleton']
        hm, off = synth.synth_batch(77, 2, 256, 256, flip=flip, n_persons=7, skeleton=skel)
    proc = processor(2, headnet, include_scale=scl is not None, **over)
    proc.fold_flip = case != "flip_unfolded"
    assert proc.fused_upsample
    got = proc.generate_limbs(features(hm, off, dev, scl), flip_test=flip, scored_off=True)
    exp = _refined_then_plain(proc, hm, off, dev, flip, scl)
    plain = proc.generate_limbs(features(hm, off, dev, scl), flip_test=flip, scored_off=False)
    torch.cuda.synchronize()
    assert got.shape == exp.shape and torch.equal(got.view(torch.int32), exp.view(torch.int32))     # all 13 columns, bit for bit
    assert not torch.equal(got, plain), "the refinement changes nothing here: the comparison would be vacuous"


# ------------------------------------------------------------------ 5. flip-test + scored_off against the reference's poses
@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("fused", [True, False])
def test_flip_scored_golden(dev, monkeypatch, fold, fused):
    g, hm, off = scored256_flip()
    proc = processor(int(g["batch"]))
    proc.fold_flip, proc.fused_upsample = fold, fused
    lib = _lib.load()
    k0 = []
    real = lib.og_flip_merge_f32
    monkeypatch.setattr(lib, 'og_flip_merge_f32', lambda *a: (k0.append(1), real(*a))[1], raising=False)
    poses = proc.generate_poses(features(hm, off, dev), flip_test=True, scored_off=True)
    assert_poses_match(split_poses(g), poses, SCORE_TOL)
    if fold and fused:
        assert k0 == [], "the folded run launched a K0 pass"
    else:
        assert k0 == [1]


def test_flip_merged_refined_offsets_reference_sha(dev):
    """K0 + the stand-alone kernel = the bit pattern of the reference's scored_offset on its flip_augment's maps."""
    g, hm, off = scored256_flip()
    proc = processor(int(g["batch"]))
    thm, _, toff, _, _ = proc.flip_augment(torch.from_numpy(hm).to(dev), [], torch.from_numpy(off).to(dev), [], False, 2)
    out = scored_offset(thm, toff, pack_jtypes(proc.skeleton)[0], None, kernel_size=3)
    assert sha(out.cpu().numpy()) == str(g["scored_sha"])


# ------------------------------------------------------------------ 6. the harness
def _raw_loader():
    rng = np.random.default_rng(11)
    sizes = [(120, 200), (333, 250), (256, 256), (90, 64), (301, 177)]
    raw = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    return [(raw[0:2], [None] * 2, [{'image_id': 1}, {'image_id': 2}]), (raw[2:4], [None] * 2, [{'image_id': 3}, {'image_id': 4}]),
            (raw[4:5], [None], [{'image_id': 5}])]


def _cli(extra=()):
    return evaluate.evaluate_cli(['--no-pretrain', '--initialize-whole', 'False', '--topk', '32', '--thre-hmp', '0.04',
                                  '--person-thre', '0.04', '--dist-max', '40', '--long-edge', '256', '--batch-size', '2',
                                  '--print-freq', '1', *extra])


def _spy_submit(monkeypatch, seen):
    real = decoder.factory.PostProcess.submit

    def spy(self, features, flip_test=False, cat_flip_offs=False, scored_off=False):
        hm, off = features[self.hmp_index][0][self.feat_stage], features[self.omp_index][0][self.feat_stage]
        seen.append((hm.clone(), off.clone(), flip_test, scored_off))
        return real(self, features, flip_test=flip_test, cat_flip_offs=cat_flip_offs, scored_off=scored_off)
    monkeypatch.setattr(decoder.factory.PostProcess, 'submit', spy)


@pytest.mark.parametrize("scales", [(), ('0.5', '1', '1.5')])
@pytest.mark.parametrize("flip", [False, True])
def test_run_images_scored_off(dev, monkeypatch, scales, flip):
    """--scored-off reaches submit() on both paths; the results are those of generate_poses(scored_off=True) on the maps the
    harness decoded (single scale: the engine outputs; --test-scales: what merge_scales left in the accumulators)."""
    torch.manual_seed(0)
    extra = (['--flip-test'] if flip else []) + (['--test-scales', *scales] if scales else [])
    a = _cli(['--scored-off'] + extra)
    model, _ = models.model_factory(a)
    seen = []
    _spy_submit(monkeypatch, seen)
    loader = _raw_loader()
    results, ids = evaluate.run_images(a, data_loader=loader, model=model)
    assert ids == [1, 2, 3, 4, 5] and len(seen) == len(loader)
    assert all(s[3] is True and s[2] == (flip and not scales) for s in seen)
    proc = decoder.decoder_factory(a)
    pre = transforms.EvalPreprocess(256)
    exp_results, exp_ids = [], []
    for (imgs, _, metas), (hm, off, flip_test, _) in zip(loader, seen):
        if scales:
            base_metas = pre.multi_scale(list(imgs), [float(s) for s in scales], image_ids=[m['image_id'] for m in metas])[1][1]
        else:
            base_metas = pre(list(imgs), image_ids=[m['image_id'] for m in metas])[1]
        feats = [([hm], [[]], [[]]), ([off], [[]], [[]])]
        poses = proc.generate_poses(feats, flip_test=flip_test, scored_off=True)
        for image_poses, meta in zip(poses, base_metas):
            evaluate.poses_to_results(image_poses, meta, exp_results, exp_ids)
    assert exp_ids == ids and results == exp_results
    # without the flag: submit() is told scored_off=False and the result dicts are those of the unrefined decode
    seen.clear()
    plain, ids0 = evaluate.run_images(_cli(extra), data_loader=_raw_loader(), model=model)
    assert ids0 == ids and all(s[3] is False for s in seen)
    exp_plain, exp_ids = [], []
    for (imgs, _, metas), (hm, off, flip_test, _) in zip(loader, seen):
        ids_ = [m['image_id'] for m in metas]
        base_metas = pre.multi_scale(list(imgs), [float(s) for s in scales], image_ids=ids_)[1][1] if scales else pre(list(imgs), image_ids=ids_)[1]
        for image_poses, meta in zip(proc.generate_poses([([hm], [[]], [[]]), ([off], [[]], [[]])], flip_test=flip_test), base_metas):
            evaluate.poses_to_results(image_poses, meta, exp_plain, exp_ids)
    assert plain == exp_plain


def test_multi_scale_scored_equals_merge_then_decode(dev):
    """merge_scales + generate_poses(scored_off=True) is the ordinary decode of the merged maps: in-pairing == kernel + decode."""
    proc = processor(2)
    rng = np.random.default_rng(5)
    hm, off = synth.synth_batch(91, 2, 256, 256, n_persons=6)
    acc = (torch.from_numpy(hm).to(dev), torch.from_numpy(off + rng.normal(0, 0.3, off.shape).astype(np.float32)).to(dev))
    feats = [([acc[0]], [[]], [[]]), ([acc[1]], [[]], [[]])]
    got = proc.generate_limbs(feats, scored_off=True)
    ref_off = scored_offset(acc[0], acc[1], pack_jtypes(proc.skeleton)[0], None, kernel_size=3)
    exp = proc.generate_limbs([([acc[0]], [[]], [[]]), ([ref_off], [[]], [[]])], scored_off=False)
    assert torch.equal(got.view(torch.int32), exp.view(torch.int32))


# ------------------------------------------------------------------ 7. what stays refused
@pytest.mark.parametrize("fold", [True, False])
def test_scored_with_cat_flip_offs_still_raises(dev, fold):
    g, hm, off = scored256_flip()
    proc = processor(int(g["batch"]))
    proc.fold_flip = fold
    with pytest.raises(NotImplementedError):
        proc.generate_poses(features(hm, off, dev), flip_test=True, cat_flip_offs=True, scored_off=True)


def test_scored_entry_points_validate(dev):
    lib = _lib.load()
    proc = processor(2)
    hm, off = torch.zeros(2, 17, 64, 64, device=dev), torch.zeros(2, 38, 64, 64, device=dev)
    with pytest.raises(_lib.OgError, match="ksize"):
        proc.limb_collect.generate_limbs_fused(hm, off, scored_ks=4)
    with pytest.raises(NotImplementedError):
        proc.limb_collect.generate_limbs_fused(hm, off, vector_nd=4, scored_ks=3)
    assert lib.og_abi_version() == 4
