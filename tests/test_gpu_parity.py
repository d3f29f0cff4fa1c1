"""GPU parity: the HIP kernels (through the C ABI / the drop-in Python API) against the CPU oracle
and the committed golden vectors.  Bit-exact for indices, coordinates, grouping; <= 1e-4 for scores
(tolerance stated by the north star; observed ~1e-7, the device exp() differs from Sleef by <= 1 ulp)."""
import argparse

import numpy as np
import pytest
import torch

import oracle
from offsetguided_amd import _lib, decoder, synth
from offsetguided_amd.config import coco_data as cd
from helpers import (FLAGS, SKELETON_CASES, case_flags, case_headnet, case_skeleton, GOLDEN, PIPE_CASES, assert_limbs_match, assert_poses_match, flip_tables, is_cat, load_case, jitter_case_inputs, scale_case_inputs,
                     split_poses)

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    _lib.load()
    return torch.device("cuda:0")


def processor(batch=2, headnet='omp', **over):
    p = argparse.ArgumentParser()
    decoder.decoder_cli(p)
    f = dict(FLAGS, **over)
    a = p.parse_args(['--topk', str(f['topk']), '--thre-hmp', str(f['thre_hmp']), '--person-thre',
                      str(f['person_thre']), '--dist-max', str(f['dist_max']), '--min-len', str(f['min_len'])])
    a.headnets, a.strides, a.batch_size = ['hmp', headnet], [4, 4], batch
    a.include_scale = a.include_jitter_offset = False
    return decoder.decoder_factory(a)


def case_processor(g):
    """The processor a pipeline fixture was generated with: its offset head (skeleton) and --topk."""
    return processor(int(g["batch"]), case_headnet(g), topk=case_flags(g)["topk"])


def features(hm, off, dev):
    hm, off = torch.from_numpy(hm).to(dev), torch.from_numpy(off).to(dev)
    return [([hm * 0, hm], [[], []], [[], []]), ([off * 0, off], [[], []], [[], []])]


# ------------------------------------------------------------------ upsampling (a5)
@pytest.mark.parametrize("shape", [(2, 3, 24, 40), (1, 2, 7, 61), (1, 1, 1, 1), (1, 2, 5, 130), (2, 17, 160, 160)])
def test_bicubic_bit_exact(dev, shape):
    x = synth.noise_batch(21, shape)
    got = decoder.factory.upsample4(torch.from_numpy(x).to(dev), 'bicubic').cpu().numpy()
    assert (got == oracle.bicubic4(x)).all()


@pytest.mark.parametrize("shape", [(2, 3, 24, 40), (1, 2, 7, 61), (1, 1, 1, 1), (1, 38, 64, 64)])
def test_bilinear_bit_exact(dev, shape):
    x = synth.noise_batch(22, shape)
    got = decoder.factory.upsample4(torch.from_numpy(x).to(dev), 'bilinear').cpu().numpy()
    assert (got == oracle.bilinear4(x)).all()


# ------------------------------------------------------------------ NMS / top-k (a6-a8)
NMS_SHAPES = [(2, 3, 37, 53), (1, 2, 64, 64), (1, 1, 3, 250), (1, 2, 33, 252), (1, 1, 70, 640), (1, 1, 9, 1000)]


@pytest.mark.parametrize("shape", NMS_SHAPES)
def test_hmp_nms_exact(dev, shape):
    z = synth.noise_batch(23, shape)
    got = decoder.hmp_NMS(torch.from_numpy(z).to(dev)).cpu().numpy()
    ref = oracle.hmp_nms(z)
    assert (got == ref).all() and (np.signbit(got) == np.signbit(ref)).all()


@pytest.mark.parametrize("shape", NMS_SHAPES)
@pytest.mark.parametrize("k", [1, 9, 32, 100])
def test_topk_channel_exact(dev, shape, k):
    z = synth.noise_batch(24, shape)
    if k > shape[2] * shape[3]:
        pytest.skip("k > plane")
    for inp in (z, oracle.hmp_nms(z)):  # plain noise, and an NMS map (mostly +-0 -> index tie rule)
        s, i, ys, xs = decoder.topK_channel(torch.from_numpy(inp).to(dev), K=k)
        rs, ri, ry, rx = oracle.topk(inp, k)
        assert (s.cpu().numpy() == rs).all() and (i.cpu().numpy() == ri).all()
        assert (ys.cpu().numpy() == ry).all() and (xs.cpu().numpy() == rx).all()


@pytest.mark.parametrize("shape", NMS_SHAPES)
@pytest.mark.parametrize("k", [1, 32, 48, 200])
def test_joint_dets_exact(dev, shape, k):
    # (each geometry once, behind another one: the COLD kernel -- the warm one is pinned in test_gpu_nms_topk_warm.py)
    z = synth.noise_batch(25, shape)
    if k > 2 * (shape[2] + shape[3]) - 4:
        pytest.skip("plane border smaller than k")
    s, i, ys, xs = decoder.joint_dets(torch.from_numpy(z).to(dev), k)
    rs, ri, ry, rx = oracle.nms_topk(z, k)
    assert (s.cpu().numpy() == rs).all() and (i.cpu().numpy() == ri).all()
    assert (ys.cpu().numpy() == ry).all() and (xs.cpu().numpy() == rx).all()


def test_joint_dets_degenerate_planes(dev):
    """All-zero, constant, negative-only and plateau planes: filler order = lowest zero-valued index."""
    H, W, k = 40, 48, 32
    planes = np.zeros((1, 6, H, W), np.float32)
    planes[0, 1] = 0.5                                   # constant positive: every pixel is a peak (ties by index)
    planes[0, 2] = -1.0                                  # constant negative: interior kept (negative), border -> -0
    planes[0, 3, 10:14, 20:30] = 0.7                     # plateau
    planes[0, 4] = -np.abs(synth.noise_batch(3, (H, W)))  # negative noise with negative interior peaks
    planes[0, 5, 0, :5] = [0.3, 0.0, 0.2, 0.0, 0.1]      # peaks on the first row, zeros between
    s, i, _, _ = decoder.joint_dets(torch.from_numpy(planes).to(dev), k)
    rs, ri, _, _ = oracle.nms_topk(planes, k)
    assert (s.cpu().numpy() == rs).all() and (i.cpu().numpy() == ri).all()


def test_joint_dets_histogram_state_reuse(dev):
    """K1 keeps a per-plane score histogram in its workspace between calls (self-validated by a
    shape-encoding magic word): repeated calls, changing shapes and plain top-k calls in between must
    all stay exact."""
    seq = [((1, 3, 96, 128), 31), ((1, 3, 96, 128), 32), ((2, 2, 64, 64), 33), ((1, 3, 96, 128), 34),
           ((1, 3, 96, 128), 35)]
    for shape, seed in seq:
        hm = oracle.bicubic4(synth.synth_batch(seed, shape[0], shape[2], shape[3], n_persons=3)[0][:, :shape[1]])
        s, i, _, _ = decoder.joint_dets(torch.from_numpy(hm).to(dev), 32)
        rs, ri, _, _ = oracle.nms_topk(hm, 32)
        assert (s.cpu().numpy() == rs).all() and (i.cpu().numpy() == ri).all()
        if seed == 33:  # plain top-k shares the workspace and must invalidate the histogram state
            z = synth.noise_batch(5, (1, 3, 96, 128))
            s2, i2, _, _ = decoder.topK_channel(torch.from_numpy(z).to(dev), K=32)
            r2 = oracle.topk(z, 32)
            assert (s2.cpu().numpy() == r2[0]).all() and (i2.cpu().numpy() == r2[1]).all()


@pytest.mark.parametrize("shape", [(2, 3, 24, 40), (1, 2, 7, 61), (1, 1, 160, 160), (1, 3, 20, 250), (2, 17, 64, 64)])
@pytest.mark.parametrize("k", [1, 32, 48])
def test_joint_dets_lowres_fused_exact(dev, shape, k):
    """K1-fused (bicubic inside the NMS kernel) == joint_dets on the materialised upsample, bit for bit."""
    x = synth.noise_batch(26, shape, 0.05)
    x[..., : shape[2] // 2, :] = np.abs(x[..., : shape[2] // 2, :])       # mixed-sign and positive regions
    if k > 2 * 4 * (shape[2] + shape[3]) - 4:
        pytest.skip("plane border smaller than k")
    for rep in range(2):                                                   # second call: slot-table thresholds active
        s, i, ys, xs = decoder.joint_dets_lowres(torch.from_numpy(x).to(dev), k)
        rs, ri, ry, rx = oracle.nms_topk(oracle.bicubic4(x), k)
        assert (s.cpu().numpy() == rs).all() and (i.cpu().numpy() == ri).all()
        assert (ys.cpu().numpy() == ry).all() and (xs.cpu().numpy() == rx).all()


def test_joint_dets_lowres_degenerate(dev):
    x = np.zeros((1, 3, 16, 20), np.float32)
    x[0, 1] = 0.25
    x[0, 2, 5, 7] = 1.0
    s, i, _, _ = decoder.joint_dets_lowres(torch.from_numpy(x).to(dev), 32)
    rs, ri, _, _ = oracle.nms_topk(oracle.bicubic4(x), 32)
    assert (s.cpu().numpy() == rs).all() and (i.cpu().numpy() == ri).all()


@pytest.mark.parametrize("name", PIPE_CASES)
def test_generate_poses_fused_golden(dev, name):
    g, hm, off = load_case(name)
    proc = case_processor(g)
    proc.fused_upsample = True
    feats = features(hm, off, dev)
    limbs = proc.generate_limbs(feats, flip_test=bool(g["flip"]), cat_flip_offs=is_cat(g)).cpu().numpy()
    assert_limbs_match(g["limbs"], limbs, SCORE_TOL)
    assert_poses_match(split_poses(g), proc.generate_poses(feats, flip_test=bool(g["flip"]), cat_flip_offs=is_cat(g)),
                       SCORE_TOL)


def test_topk_errors(dev):
    z = torch.zeros(1, 1, 4, 5, device=dev)
    with pytest.raises(RuntimeError):
        decoder.topK_channel(z, K=21)
    with pytest.raises(_lib.OgError):
        decoder.joint_dets(torch.zeros(1, 1, 4, 5), 2)   # CPU tensor: no fallback


# ------------------------------------------------------------------ limbs (a9-a10)
@pytest.mark.parametrize("name", ["pipe256_p6", "pipe256_p20", "pipe640", "pipe256_omp31_p6", "pipe256_omp44_k48_p20"])
def test_collect_limbs_both_offset_forms(dev, name):
    g, hm, off = load_case(name)
    proc = case_processor(g)
    hr = oracle.bicubic4(hm)
    ohr = oracle.bilinear4(off)
    t_hr = torch.from_numpy(hr).to(dev)
    l_hi = proc.limb_collect.generate_limbs(t_hr, [], torch.from_numpy(ohr).to(dev), []).cpu().numpy()
    l_lo = proc.limb_collect.generate_limbs_lowres(t_hr, torch.from_numpy(off).to(dev)).cpu().numpy()
    assert (l_hi == l_lo).all()
    assert_limbs_match(g["limbs"], l_hi, SCORE_TOL)


def test_collect_spatial_mismatch_asserts(dev):
    proc = processor()
    with pytest.raises(AssertionError):
        proc.limb_collect.generate_limbs(torch.zeros(1, 17, 64, 64, device=dev), [],
                                         torch.zeros(1, 38, 32, 32, device=dev), [])


# ------------------------------------------------------------------ grouping (a12)
def test_grouping_golden_adversarial(dev):
    g = np.load(f"{GOLDEN}/grouping_adversarial.npz")
    for si, sk_name in enumerate(g["skeleton_names"]):
        sk = getattr(cd, str(sk_name))
        o = 0
        for limbs, (K, M), cfg in zip(g[f"limbs_{si}"], g[f"kn_{si}"], g[f"cfg_{si}"]):
            thre, dmax, use_scale, sort_dim = g["cfg_table"][cfg]
            G = decoder.GreedyGroup(thre, sort_dim=int(sort_dim), dist_max=dmax, use_scale=bool(use_scale), skeleton=sk)
            got = G.group_skeletons(np.ascontiguousarray(limbs[:, :K]))
            ref = g[f"poses_{si}"][o:o + M]
            o += M
            assert got.shape == ref.shape and (got == ref).all(), f"{sk_name} case"


@pytest.mark.parametrize("sk_name", ["COCO_PERSON_SKELETON", "DENSER_COCO_PERSON_SKELETON"])
def test_grouping_fuzz_vs_oracle(dev, sk_name):
    sk = getattr(cd, sk_name)
    cases = []
    for i in range(96):
        rng = synth.HashRng(880000 + i)
        K = int(rng.integers(1, 2, 12)[0])
        cases.append(_adversarial(rng, K, sk))
    G = decoder.GreedyGroup(0.04, sort_dim=2, dist_max=40.0, use_scale=False, skeleton=sk)
    for K in sorted({c.shape[1] for c in cases}):
        batch = np.stack([c for c in cases if c.shape[1] == K])
        got = G.group_batch(torch.from_numpy(batch).to(dev))
        for lim, p in zip(batch, got):
            ref = oracle.greedy_group(lim, sk, 17, 0.04, 40.0)
            assert p.shape == ref.shape and (p == ref).all()


def _adversarial(rng, K, skeleton, hw=4096):
    """Same collision-heavy generator as tools/gen_golden.py (mode 1), self-contained for the GPU box."""
    L = len(skeleton)
    pool = int(rng.integers(1, 1, 3)[0])
    cand_xy = rng.uniform(17 * pool * 2, 1.0, 200.0).reshape(17, pool, 2).round()
    cand_v = rng.uniform(17 * pool, 0.05, 1.0).reshape(17, pool)
    P = int(rng.integers(1, 2, 5)[0])
    pid = rng.integers(P * 17, 0, pool - 1).reshape(P, 17)
    limbs = np.zeros((L, K, 13), np.float32)
    for l, (a, b) in enumerate(skeleton):
        order = np.argsort(rng.uniform(P))
        take, cross, other = rng.uniform(P) < 0.8, rng.uniform(P) < 0.3, rng.integers(P, 0, P - 1)
        fl, tl = [], []
        for p in order:
            if take[p] and pid[p, a] not in fl:
                fl.append(pid[p, a])
                tl.append(pid[other[p], b] if cross[p] else pid[p, b])
        fl, tl = fl[:K], tl[:K]
        sc = rng.uniform(K, 0.01, 1.0) * 10.0 ** -float(rng.integers(1, 0, 2)[0])
        dist = rng.uniform(K, 0.0, 45.0)
        for k in range(K):
            if k < len(fl):
                f, t = fl[k], tl[k]
                limbs[l, k] = [cand_xy[a, f, 0], cand_xy[a, f, 1], cand_v[a, f], cand_xy[b, t, 0], cand_xy[b, t, 1],
                               cand_v[b, t], a * hw + f, b * hw + t, dist[k], 10.0, sc[k], 4.0, 4.0]
            else:
                limbs[l, k] = [-99990.0, -99980.0, 0.001, -99970.0, -99960.0, 0.002, a * hw + pool + k,
                               b * hw + pool + k, 5.0, 10.0, 1e-6 * (k + 1), 4.0, 4.0]
    return limbs


@pytest.mark.parametrize("sk_name,K,variant", [("COCO_PERSON_SKELETON", 32, "lds"), ("DENSER_COCO_PERSON_SKELETON", 48, "table in the workspace"),
                                               ("DENSER_COCO_PERSON_SKELETON", 64, "table + staged rows in the workspace"),
                                               ("COCO_PERSON_WITH_REDUNDANT_SKELETON", 128, "table + staged rows in the workspace"),
                                               ("KINEMATIC_TREE_SKELETON", 200, "table + staged rows in the workspace")])
def test_grouping_any_skeleton_any_topk(dev, sk_name, K, variant):
    """K3 serves every skeleton the reference defines at any realistic --topk (the reference's GreedyGroup has no limit,
    decoder/group.py:39-240; its CLI default is 48, decoder/factory.py:154): when L*k does not fit in LDS the partial-skeleton table,
    then the staged candidate rows, live in the caller's workspace.  Collision-heavy limbs with many candidates per type, vs
    the oracle, bit for bit."""
    sk = getattr(cd, sk_name)
    cases = []
    for i in range(6):
        rng = synth.HashRng(990000 + 17 * K + i)
        lim = _adversarial(rng, K, sk)
        # fill the tail rows (sub-threshold fillers in _adversarial) with more real candidates so that many rows survive
        rng2 = synth.HashRng(991000 + 17 * K + i)
        P = 14
        xy = rng2.uniform(P * 17 * 2, 1.0, 400.0).reshape(P, 17, 2).round()
        v = rng2.uniform(P * 17, 0.05, 1.0).reshape(P, 17)
        for l, (a, b) in enumerate(sk):
            sc = rng2.uniform(P, 0.01, 1.0)
            swap = rng2.integers(P, 0, P - 1)
            for q in range(min(P, K)):
                t = int(swap[q]) if q % 3 == 0 else q
                lim[l, K - 1 - q] = [xy[q, a, 0], xy[q, a, 1], v[q, a], xy[t, b, 0], xy[t, b, 1], v[t, b],
                                     a * 4096 + 100 + q, b * 4096 + 100 + t, 3.0, 10.0, sc[q], 4.0, 4.0]
        cases.append(lim)
    G = decoder.GreedyGroup(0.04, sort_dim=2, dist_max=40.0, use_scale=False, skeleton=sk)
    got = G.group_batch(torch.from_numpy(np.stack(cases)).to(dev))
    for lim, p in zip(cases, got):
        ref = oracle.greedy_group(lim, sk, 17, 0.04, 40.0)
        assert len(ref) > 0 and p.shape == ref.shape and (p == ref).all(), variant


def test_grouping_capacity_limit_is_an_error(dev):
    """Beyond the documented capacity (16 B of LDS per candidate + 108 B per table row) K3 refuses with
    OG_EUNSUPPORTED and a message -- never a wrong result, never a silent CPU path."""
    sk = cd.DENSER_COCO_PERSON_SKELETON
    G = decoder.GreedyGroup(0.04, dist_max=40.0, skeleton=sk)
    with pytest.raises(_lib.OgError, match="LDS"):
        G.group_device(torch.zeros(1, len(sk), 256, 13, device=dev))


def test_grouping_table_overflow_retry(dev):
    """More live partial skeletons than the LDS table holds -> flagged, retried with a larger table."""
    sk = cd.COCO_PERSON_SKELETON
    K = 40
    limbs = np.zeros((len(sk), K, 13), np.float32)
    for l, (a, b) in enumerate(sk):          # every limb row is an isolated 2-keypoint skeleton
        for k in range(K):
            uid = l * K + k
            limbs[l, k] = [1 + uid, 2 + uid, 0.5, 3 + uid, 4 + uid, 0.6, a * 500000 + uid, b * 500000 + uid,
                           1.0, 10.0, 0.3 + 1e-4 * uid, 4.0, 4.0]
    G = decoder.GreedyGroup(0.04, dist_max=40.0, skeleton=sk)
    got = G.group_skeletons(limbs)
    ref = oracle.greedy_group(limbs, sk, 17, 0.04, 40.0)
    assert len(ref) > G.MMAX
    assert got.shape == ref.shape and (got == ref).all()


# ------------------------------------------------------------------ flip merge (a4) + whole pipeline
@pytest.mark.parametrize("name", ["pipe256_flip_p6", "pipe640_flip", "pipe256_flipcat_p6", "pipe640_flipcat"] +
                         [c for c in SKELETON_CASES if "_flip" in c])
def test_flip_merge_exact(dev, name):
    g, hm, off = load_case(name)
    proc = case_processor(g)
    cat = is_cat(g)
    mh, _, mo, _, nd = proc.flip_augment(torch.from_numpy(hm).to(dev), [], torch.from_numpy(off).to(dev), [], cat, 2)
    rh, ro = (oracle.flip_cat if cat else oracle.flip_merge)(hm, off, *flip_tables(case_skeleton(g)))
    assert nd == (4 if cat else 2)
    assert mo.shape == ((hm.shape[0], off.shape[1]) + hm.shape[2:] if cat else ro.shape)  # factory.py:127 view
    assert (mh.cpu().numpy() == rh).all() and (mo.cpu().numpy().ravel() == ro.ravel()).all()


@pytest.mark.parametrize("shape,headnet,topk", [((2, 256, 256), "omp", 32), ((8, 640, 640), "omp", 32), ((3, 384, 512), "omp", 32),
                                                ((2, 256, 256), "omp16", 32), ((2, 256, 320), "omp31", 48),
                                                ((2, 256, 256), "omp44", 48), ((3, 192, 256), "omp25", 20)])
def test_flip_fold_equals_flip_merge(dev, shape, headnet, topk):
    """flip_augment folded into its consumers (og_upsample_bicubic4_flip_f32, og_generate_limbs_flip_f32: the merge of
    decoder/factory.py:98-146 computed on the loads) == og_flip_merge_f32 followed by the plain kernels, bit for bit: the hi-res
    heatmaps, the limbs (every column) and the poses; and the folded pipeline against the oracle on two images."""
    n, h, w = shape
    skel = decoder.factory.parse_heads(headnet, 4)["skeleton"]
    hm, off = synth.synth_batch(31 + n, n, h, w, flip=True, skeleton=skel)
    t_hm, t_off = torch.from_numpy(hm).to(dev), torch.from_numpy(off).to(dev)
    proc = processor(n, headnet, topk=topk)
    assert proc.fold_flip
    kp_perm, (limb_perm, reserve) = proc.keypoints_flips, proc.limbs_flips
    mh, _, mo, _, _ = proc.flip_augment(t_hm, [], t_off, [], False, 2)
    hr_ref = decoder.factory.upsample4(mh, 'bicubic')
    hr = decoder.factory.upsample4_flip(t_hm, kp_perm)
    assert torch.equal(hr, hr_ref)
    keep = [1 if l in reserve else 0 for l in range(len(limb_perm))]
    l_ref = proc.limb_collect.generate_limbs_lowres(hr_ref, mo)
    l_fold = proc.limb_collect.generate_limbs_flip(hr, t_off, limb_perm, keep)
    assert torch.equal(l_fold, l_ref)
    # K1-fused with the merge folded into its source loads and its offset taps (og_generate_limbs_fused_flip_f32) == the same limbs
    l_ffold = proc.limb_collect.generate_limbs_fused_flip(t_hm, t_off, kp_perm, limb_perm, keep)
    assert torch.equal(l_ffold, l_ref)
    l_fsep = proc.limb_collect.generate_limbs_fused(mh, mo)
    assert torch.equal(l_fsep, l_ref)
    feats = [([None, t_hm], [[], []], [[], []]), ([None, t_off], [[], []], [[], []])]
    for fused in (True, False):
        proc.fused_upsample, proc.fold_flip = fused, True
        poses_fold = proc.generate_poses(feats, flip_test=True)
        proc.fold_flip = False
        poses_ref = proc.generate_poses(feats, flip_test=True)
        assert len(poses_fold) == len(poses_ref) == n and all(np.array_equal(a_, b_) for a_, b_ in zip(poses_fold, poses_ref))
    sel = [0, 1, n, n + 1]
    ref, _ = oracle.decode(hm[sel], off[sel], skel, topk_k=topk, thre_hmp=FLAGS["thre_hmp"],
                           min_len=FLAGS["min_len"], person_thre=FLAGS["person_thre"], dist_max=FLAGS["dist_max"],
                           flip=flip_tables(skel))
    assert_poses_match(ref, poses_fold[:2], SCORE_TOL)


def test_folded_flip_beyond_the_lds_limit_takes_the_unfolded_route(dev):
    """--topk beyond what the folded K1-fused form's merge + pairing stage holds in LDS (about k = 226 at 640 x 640): the C side answers
    OG_EUNSUPPORTED and generate_limbs falls back to flip_augment as its own pass + K1-fused -- the same limbs, bit for bit, as with the
    fold switched off, and below the limit the fold is taken."""
    n, size, k = 1, 640, 240
    hm, off = synth.synth_batch(77, n, size, size, flip=True)
    t_hm, t_off = torch.from_numpy(hm).to(dev), torch.from_numpy(off).to(dev)
    feats = [([None, t_hm], [[], []], [[], []]), ([None, t_off], [[], []], [[], []])]
    proc = processor(n, topk=k)
    assert proc.fold_flip and proc.fused_upsample
    kp_perm, (limb_perm, reserve) = proc.keypoints_flips, proc.limbs_flips
    keep = [1 if l in reserve else 0 for l in range(len(limb_perm))]
    with pytest.raises(_lib.OgError, match=r'code -4'):
        proc.limb_collect.generate_limbs_fused_flip(t_hm, t_off, kp_perm, limb_perm, keep)
    got = proc.generate_limbs(feats, flip_test=True).clone()
    proc.fold_flip = False
    ref = proc.generate_limbs(feats, flip_test=True)
    assert got.shape == (n, 19, k, 13) and torch.equal(got, ref)


def test_fused_flip_fold_few_peaks(dev):
    """The folded flip in K1-fused where a plane has FEWER than k positive peaks: the merge stage then fills the list with the lowest
    zero-output indices, evaluating the x4 bicubic of the MERGED source at single points (merge_plane's zero-fill path with the
    mirrored partner plane) -- bit-equal to og_flip_merge_f32 followed by the fused kernel, and to the oracle."""
    n, h, w = 2, 96, 128
    hm, off = synth.synth_batch(77, n, h, w, flip=True, n_persons=2)
    hm[:, 3] = -np.abs(hm[:, 3])                   # a plane without positive values
    hm[:, 5] = 0.0                                 # an all-zero plane
    hm[:, 7] *= (np.abs(hm[:, 7]) > 0.3)           # a plane with one or two blobs and exact zeros elsewhere
    t_hm, t_off = torch.from_numpy(hm).to(dev), torch.from_numpy(off).to(dev)
    proc = processor(n)
    kp_perm, (limb_perm, reserve) = proc.keypoints_flips, proc.limbs_flips
    keep = [1 if l in reserve else 0 for l in range(len(limb_perm))]
    mh, _, mo, _, _ = proc.flip_augment(t_hm, [], t_off, [], False, 2)
    l_sep = proc.limb_collect.generate_limbs_fused(mh, mo)
    l_fold = proc.limb_collect.generate_limbs_fused_flip(t_hm, t_off, kp_perm, limb_perm, keep)
    assert torch.equal(l_fold, l_sep)
    l_hr = proc.limb_collect.generate_limbs_lowres(decoder.factory.upsample4(mh, 'bicubic'), mo)
    assert torch.equal(l_fold, l_hr)
    ref, _ = oracle.decode(hm, off, cd.COCO_PERSON_SKELETON, topk_k=FLAGS["topk"], thre_hmp=FLAGS["thre_hmp"], min_len=FLAGS["min_len"],
                           person_thre=FLAGS["person_thre"], dist_max=FLAGS["dist_max"], flip=flip_tables())
    assert_poses_match(ref, proc.generate_poses(features(hm, off, dev), flip_test=True), SCORE_TOL)


def test_decoder_forms_fuzz(dev):
    """The four ways through the limb stage with flip-test -- K0 pass + K1a + K1, the flip folded into K1a / K1, K0 pass + K1-fused, the
    flip folded into K1-fused (production) -- on 100 random configurations (batch, non-square sizes, k, every skeleton; planes without
    positive values, exact zeros with few peaks, thousands of peaks): bit-identical limbs, every column."""
    rng = np.random.default_rng(123)
    done = 0
    for it in range(100):
        n, h, w = int(rng.integers(1, 4)), int(rng.integers(8, 60)) * 4, int(rng.integers(8, 90)) * 4
        k, headnet = int(rng.choice([1, 7, 20, 32, 48])), str(rng.choice(['omp', 'omp16', 'omp31', 'omp44', 'omp25']))
        if k > 2 * (h + w) - 4:
            continue
        proc = processor(n, headnet, topk=k)
        hm, off = synth.synth_batch(int(rng.integers(1 << 30)), n, h, w, flip=True, n_persons=int(rng.integers(0, 6)), skeleton=proc.skeleton)
        mode = it % 4
        if mode == 1:
            hm[:, ::3] = -np.abs(hm[:, ::3])
        elif mode == 2:
            hm *= (np.abs(hm) > 0.25)
        elif mode == 3:
            hm += rng.normal(0, 0.2, hm.shape).astype(np.float32)
        t_hm, t_off = torch.from_numpy(hm).to(dev), torch.from_numpy(off).to(dev)
        kp, (lp, rs) = proc.keypoints_flips, proc.limbs_flips
        keep = [1 if l in rs else 0 for l in range(len(lp))]
        mh, _, mo, _, _ = proc.flip_augment(t_hm, [], t_off, [], False, 2)
        ref = proc.limb_collect.generate_limbs_lowres(decoder.factory.upsample4(mh, 'bicubic'), mo)
        assert torch.equal(ref, proc.limb_collect.generate_limbs_fused(mh, mo)), (it, n, h, w, k, headnet, mode, 'K0 + K1-fused')
        assert torch.equal(ref, proc.limb_collect.generate_limbs_fused_flip(t_hm, t_off, kp, lp, keep)), (it, n, h, w, k, headnet, mode, 'folded K1-fused')
        assert torch.equal(ref, proc.limb_collect.generate_limbs_flip(decoder.factory.upsample4_flip(t_hm, kp), t_off, lp, keep)), (it, 'folded K1a / K1')
        done += 1
    assert done >= 80


@pytest.mark.parametrize("name", ["pipe256_flipcat_p6", "pipe640_flipcat", "pipe256_omp16_flipcat_p6", "pipe256_omp44_flipcat_p6"])
def test_collect_limbs_4d_offsets_hires_form(dev, name):
    """The reference's own call (collect.py:62 with vector_nd=4 on materialised hi-res offsets) == low-res sampling."""
    g, hm, off = load_case(name)
    proc = case_processor(g)
    mh, _, mo, _, nd = proc.flip_augment(torch.from_numpy(hm).to(dev), [], torch.from_numpy(off).to(dev), [], True, 2)
    hr = decoder.factory.upsample4(mh, 'bicubic')
    ohr = decoder.factory.upsample4(mo, 'bilinear')
    limbs = proc.limb_collect.generate_limbs(hr, [], ohr, [], nd).cpu().numpy()
    assert_limbs_match(g["limbs"], limbs, SCORE_TOL)


@pytest.mark.parametrize("name", PIPE_CASES)
def test_generate_poses_golden(dev, name):
    """Drop-in surface: decoder_factory(args).generate_poses(features, flip_test) vs the reference's output."""
    g, hm, off = load_case(name)
    proc = case_processor(g)
    assert proc.fused_upsample                       # the production default (K1-fused) is test_generate_poses_fused_golden's
    proc.fused_upsample = False                      # here: K1a + K1 on the materialised hi-res maps (the reference's structure)
    feats = features(hm, off, dev)
    limbs = proc.generate_limbs(feats, flip_test=bool(g["flip"]), cat_flip_offs=is_cat(g)).cpu().numpy()
    assert_limbs_match(g["limbs"], limbs, SCORE_TOL)
    poses = proc.generate_poses(feats, flip_test=bool(g["flip"]), cat_flip_offs=is_cat(g))
    assert all(p.dtype == np.float32 for p in poses)
    assert_poses_match(split_poses(g), poses, SCORE_TOL)


@pytest.mark.parametrize("name", ["jitter256", "jitter256_flip"])
@pytest.mark.parametrize("fused", [False, True])
def test_jitter_head_golden(dev, name, fused):
    """include_jitter_offset / use_jitter_offset: K2 refines the guide point (at the reference's [x][y] index) and moves
    the limb end points by the jitter vectors sampled from the stride-4 head output."""
    g = np.load(f"{GOLDEN}/{name}.npz")
    hm, off, jit = jitter_case_inputs(g)
    p = argparse.ArgumentParser()
    decoder.decoder_cli(p)
    a = p.parse_args(['--topk', str(FLAGS['topk']), '--thre-hmp', str(FLAGS['thre_hmp']), '--person-thre',
                      str(FLAGS['person_thre']), '--dist-max', str(FLAGS['dist_max']), '--min-len', str(FLAGS['min_len']),
                      '--use-jitter-offset', 'True'])
    a.headnets, a.strides, a.batch_size = ['hmp', 'omp'], [4, 4], int(g["batch"])
    a.include_scale, a.include_jitter_offset = False, True
    proc = decoder.decoder_factory(a)
    proc.fused_upsample = fused
    t = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
    feats = [([None, t(hm)], [[], []], [None, t(jit)]), ([None, t(off)], [[], []], [[], []])]
    poses = proc.generate_poses(feats, flip_test=bool(g["flip"]))
    assert_poses_match(split_poses(g), poses, SCORE_TOL)
    # without use_jitter_offset the head is ignored (collect.py:154, :212): same poses as without the head
    proc.limb_collect.use_jitter_offset = False
    plain = processor(int(g["batch"]))
    a_ = proc.generate_poses(feats, flip_test=bool(g["flip"]))
    b_ = plain.generate_poses(features(hm, off, dev), flip_test=bool(g["flip"]))
    assert all(np.array_equal(x, y) for x, y in zip(a_, b_))


def test_scored_offset_golden(dev):
    """generate_poses(scored_off=True): heatmap-weighted offsets (torch ops on the device) feeding the HIP decoder."""
    g = np.load(f"{GOLDEN}/scored256.npz")
    hm, off = synth.synth_batch(int(g["seed"]), int(g["batch"]), int(g["size"]), int(g["size"]), n_persons=6)
    proc = processor(int(g["batch"]))
    poses = proc.generate_poses(features(hm, off, dev), scored_off=True)
    assert_poses_match(split_poses(g), poses, SCORE_TOL)


@pytest.mark.parametrize("name", ["scale256", "scale256_flip"])
@pytest.mark.parametrize("fused", [False, True])
def test_scale_head_golden(dev, name, fused):
    """include_scale / use_scale: scale maps sampled at the peaks from the stride-4 head output (K2), scale-dependent
    rejection radius in K3; the poses' scale column is exact."""
    g = np.load(f"{GOLDEN}/{name}.npz")
    hm, off, scl = scale_case_inputs(g)
    p = argparse.ArgumentParser()
    decoder.decoder_cli(p)
    a = p.parse_args(['--topk', str(FLAGS['topk']), '--thre-hmp', str(FLAGS['thre_hmp']), '--person-thre',
                      str(FLAGS['person_thre']), '--dist-max', '6', '--min-len', str(FLAGS['min_len']), '--use-scale', 'True'])
    a.headnets, a.strides, a.batch_size = ['hmp', 'omp'], [4, 4], int(g["batch"])
    a.include_scale, a.include_jitter_offset = True, False
    proc = decoder.decoder_factory(a)
    proc.fused_upsample = fused
    t = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
    feats = [([None, t(hm)], [[], []], [[], []]), ([None, t(off)], [[], []], [None, t(scl)])]
    poses = proc.generate_poses(feats, flip_test=bool(g["flip"]))
    assert_poses_match(split_poses(g), poses, SCORE_TOL)
    for r, m in zip(split_poses(g), poses):
        assert (r[..., 3] == m[..., 3]).all()
    # the reference's own LimbsCollect call on maps at input resolution gathers the same scales
    if not bool(g["flip"]):
        hr = decoder.factory.upsample4(t(hm), 'bicubic')
        limbs_hr = proc.limb_collect.generate_limbs(hr, [], decoder.factory.upsample4(t(off), 'bilinear'),
                                                    decoder.factory.upsample4(t(scl), 'bicubic')).cpu().numpy()
        limbs_lr = proc.generate_limbs(feats).cpu().numpy()
        assert (limbs_hr[..., 11:] == limbs_lr[..., 11:]).all()


@pytest.mark.parametrize("name", ["bilinear256", "bilinear256_flip", "bilinear256_scale", "bilinear256_scale_flip"])
@pytest.mark.parametrize("fused", [False, True])
def test_resize_mode_bilinear_golden(dev, name, fused):
    """generate_poses composed with --resize-mode bilinear (PostProcess.inter_mode; decoder/factory.py:151-153, :74-75,
    :80-82), with and without the keypoint-scale head (include_scale + use_scale) and flip-test: vs the poses of the
    reference run with that flag, and vs the oracle.  (fused_upsample only applies to bicubic: both settings must take the
    K1a + K1 route here and agree.)"""
    from helpers import bilinear_case_inputs
    g = np.load(f"{GOLDEN}/{name}.npz")
    hm, off, scl = bilinear_case_inputs(g)
    with_scale, flip = scl is not None, bool(g["flip"])
    p = argparse.ArgumentParser()
    decoder.decoder_cli(p)
    a = p.parse_args(['--resize-mode', 'bilinear', '--topk', str(FLAGS['topk']), '--thre-hmp', str(FLAGS['thre_hmp']),
                      '--person-thre', str(FLAGS['person_thre']), '--dist-max', str(float(g["dist_max"])), '--min-len',
                      str(FLAGS['min_len']), '--use-scale', str(with_scale)])
    a.headnets, a.strides, a.batch_size = ['hmp', 'omp'], [4, 4], int(g["batch"])
    a.include_scale, a.include_jitter_offset = with_scale, False
    proc = decoder.decoder_factory(a)
    assert proc.inter_mode == 'bilinear'
    proc.fused_upsample = fused
    t = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
    feats = [([None, t(hm)], [[], []], [[], []]), ([None, t(off)], [[], []], [None, t(scl)] if with_scale else [[], []])]
    poses = proc.generate_poses(feats, flip_test=flip)
    assert_poses_match(split_poses(g), poses, SCORE_TOL)
    ref, _ = oracle.decode(hm, off, cd.COCO_PERSON_SKELETON, topk_k=FLAGS["topk"], thre_hmp=FLAGS["thre_hmp"],
                           min_len=FLAGS["min_len"], person_thre=FLAGS["person_thre"], dist_max=float(g["dist_max"]),
                           use_scale=with_scale, flip=flip_tables() if flip else None, scales_lr=scl, inter_mode='bilinear')
    assert_poses_match(ref, poses, SCORE_TOL)
    if with_scale:
        for r, m in zip(split_poses(g), poses):
            assert (r[..., 3] == m[..., 3]).all()


@pytest.mark.parametrize("order", [(0, 1, 2, 3), (3, 1, 0, 2), (2, 3, 1, 0)])
def test_submit_handles_outstanding(dev, order):
    """PostProcess.submit with several unread handles (the synchronous contract of decoder/factory.py:91-96 per batch):
    four batches are queued before the first result() and resolved in and out of order; every handle returns ITS batch
    (each owns a pinned slot until read), a second result() returns the same poses, and read slots are reused."""
    proc = processor(2)
    batches = [synth.synth_batch(900 + i, 2, 256, 256, n_persons=3 + 2 * i) for i in range(4)]
    refs = [proc.generate_poses(features(hm, off, dev)) for hm, off in batches]
    assert len({tuple(len(p) for p in r) for r in refs}) > 1     # the batches are distinguishable
    handles = [proc.submit(features(hm, off, dev)) for hm, off in batches]
    for i in order:
        got = handles[i].result()
        for r, m in zip(refs[i], got):
            assert r.shape == m.shape and (r == m).all()
        again = handles[i].result()
        assert all((x == y).all() for x, y in zip(got, again))
    pools = list(proc._pinned.values())
    assert len(pools) == 1 and len(pools[0]) == 4 and not any(sl.busy for sl in pools[0])
    more = [proc.submit(features(hm, off, dev)) for hm, off in batches[:2]]      # read slots are taken again
    assert len(pools[0]) == 4
    for h, r in zip(more, refs[:2]):
        assert all((x == y).all() for x, y in zip(r, h.result()))
    dropped = proc.submit(features(*batches[3], dev))     # a handle dropped unread gives its slot back as well: at once if its copy
    del dropped                                            # has landed, else at the first submit() after that (no wait in __del__)
    torch.cuda.synchronize()
    last = proc.submit(features(*batches[0], dev))
    assert len(pools[0]) == 4 and sum(sl.busy for sl in pools[0]) == 1
    assert all((x == y).all() for x, y in zip(refs[0], last.result()))
    assert not any(sl.busy for sl in pools[0])


@pytest.mark.parametrize("size,batch,k,flip", [((384, 512), 3, 48, False), ((128, 640), 2, 16, True), ((512, 256), 1, 32, False)])
def test_generate_poses_nonsquare_vs_oracle(dev, size, batch, k, flip):
    """Non-square inputs, other batch sizes and top-k values (CLI default 48), fused and unfused, vs the oracle."""
    H, W = size
    hm, off = synth.synth_batch(300 + H, batch, H, W, flip=flip, n_persons=4)
    proc = processor(batch, topk=k)
    feats = features(hm, off, dev)
    ref, _ = oracle.decode(hm, off, cd.COCO_PERSON_SKELETON, topk_k=k, thre_hmp=FLAGS["thre_hmp"], min_len=FLAGS["min_len"],
                           person_thre=FLAGS["person_thre"], dist_max=FLAGS["dist_max"], flip=flip_tables() if flip else None)
    for fused in (False, True):
        proc.fused_upsample = fused
        assert_poses_match(ref, proc.generate_poses(feats, flip_test=flip), SCORE_TOL)
        assert_poses_match(ref, proc.submit(feats, flip_test=flip).result(), SCORE_TOL)


@pytest.mark.parametrize("kernel", [1, 5, 7])
def test_hmp_nms_other_windows(dev, kernel):
    """hmp_NMS accepts any odd window like the reference (decoder/heatmap.py:15-35); 3 is the HIP kernel, the others run the
    reference's ops on the device: same result as those ops on the CPU, and window 3 through both routes agrees."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(kernel)
    heat = torch.randn(2, 3, 37, 53, generator=g)
    heat[0, 0, 5:9, 5:9] = 2.0                     # a plateau
    heat[1, 1] = -heat[1, 1].abs()                 # a negative plane (zero padding wins on the border)
    pad = (kernel - 1) // 2
    ref = heat * (F.max_pool2d(F.pad(heat, [pad] * 4), (kernel, kernel), stride=1) == heat).float()
    got = decoder.hmp_NMS(heat.to(dev), kernel).cpu()
    assert torch.equal(got, ref) and torch.equal(torch.signbit(got), torch.signbit(ref))
    ref3 = heat * (F.max_pool2d(F.pad(heat, [1] * 4), (3, 3), stride=1) == heat).float()
    assert torch.equal(decoder.hmp_NMS(heat.to(dev)).cpu(), ref3)
    with pytest.raises(RuntimeError):
        decoder.hmp_NMS(heat.to(dev), 4)           # even window: shapes no longer match, as in the reference


def test_global_indices_beyond_2_pow_24(dev):
    """1024x1024 inputs: C * H * W = 17.8 M > 2^24, so the GLOBAL peak indices the limbs carry as fp32 (reference
    decoder/collect.py:194-199,227-228: `ind + jtype * h * w` cast to float) are rounded to even for the upper channels, and the
    grouping compares the rounded values (group.py:87-109).  The reference rounds the same way, so parity is well defined: the
    HIP pipeline must reproduce the oracle bit for bit there too -- limbs (every column) and poses."""
    hm, off = synth.synth_batch(11, 1, 1024, 1024, n_persons=14)
    assert hm.shape == (1, 17, 256, 256)
    proc = processor(1)
    feats = features(hm, off, dev)
    limbs = proc.generate_limbs(feats).cpu().numpy()
    ref_poses, mid = oracle.decode(hm, off, cd.COCO_PERSON_SKELETON, topk_k=FLAGS["topk"], thre_hmp=FLAGS["thre_hmp"],
                                   min_len=FLAGS["min_len"], person_thre=FLAGS["person_thre"], dist_max=FLAGS["dist_max"])
    assert_limbs_match(mid["limbs"], limbs, SCORE_TOL, valid_only_thre=FLAGS["thre_hmp"])
    valid = (limbs[..., 2] >= FLAGS["thre_hmp"]) & (limbs[..., 5] >= FLAGS["thre_hmp"])
    ind = limbs[..., 6:8][valid]
    assert (ind >= 2 ** 24).any(), 'the case must reach the rounded index range'
    assert (ind[ind >= 2 ** 24] % 2 == 0).all()          # fp32 spacing is 2 there: odd indices do not exist
    poses = proc.generate_poses(feats)
    assert_poses_match(ref_poses, poses, SCORE_TOL)
    assert len(poses[0]) >= 5


def test_full_size_batch_properties(dev):
    """bs8 640x640 (BASELINE config 2): size-independent properties + oracle on the same maps."""
    hm, off = synth.synth_batch(7, 8, 640, 640)
    proc = processor(8)
    t_hr = decoder.factory.upsample4(torch.from_numpy(hm).to(dev), 'bicubic')
    s, i, ys, xs = decoder.joint_dets(t_hr, 32)
    s_h, i_h = s.cpu().numpy(), i.cpu().numpy()
    assert (np.diff(s_h, axis=-1) <= 0).all()                                  # sorted descending
    assert all(len(set(r)) == 32 for r in i_h.reshape(-1, 32))                 # distinct pixels
    flat = t_hr.view(8, 17, -1)
    assert (torch.gather(flat, 2, i) == s).all()                              # scores are the map values there
    nms = decoder.hmp_NMS(t_hr)
    assert (torch.gather(nms.view(8, 17, -1), 2, i) == s).all()               # and they are NMS survivors
    s2, i2, _, _ = decoder.topK_channel(nms, K=32)                             # fused == unfused
    assert (s2 == s).all() and (i2 == i).all()
    nms2 = decoder.hmp_NMS(nms)                                                # idempotent on the positive peaks
    assert ((nms2 == nms) | (nms < 0)).all() and ((nms2 > 0) == (nms > 0)).all()
    rs, ri, _, _ = oracle.nms_topk(oracle.bicubic4(hm[:2]), 32)                # oracle on two images
    assert (s_h[:2] == rs).all() and (i_h[:2] == ri).all()
    poses = proc.generate_poses(features(hm, off, dev))
    ref_poses, _ = oracle.decode(hm[:2], off[:2], cd.COCO_PERSON_SKELETON, topk_k=32, thre_hmp=FLAGS["thre_hmp"],
                                 min_len=FLAGS["min_len"], person_thre=FLAGS["person_thre"], dist_max=FLAGS["dist_max"])
    assert_poses_match(ref_poses, poses[:2], SCORE_TOL)
    assert len(poses) == 8
