"""GPU: the multi-scale test (--test-scales, decoder/multiscale.py, og_scale_accumulate_f32).

  * the kernel == a numpy fp32 restatement of its operation order, bit for bit (up / down sampling, non-square, ws % 4 != 0, N = 1 and
    8, the three modes, with and without flip -- the flip pair merged by oracle.flip_merge first --, a non-COCO skeleton);
  * identity: the base scale (once or twice) reproduces its input; --test-scales 1 is today's run_images;
  * units: a constant offset field of a scale that is 2x (x) / 4x (y) the base comes out as c/2, c/4;
  * planted persons rendered at scales (0.5, 1, 2) decode, after the merge, to the planted keypoints (catches a wrong direction in the
    affine or the offset units that a restatement sharing the mistake would not);
  * the strict engines at the shapes the scales imply run no torch convolution;
  * run_images with --test-scales 0.5 1 1.5 (flip off / on, one and two lanes) == numpy merge of the engine outputs -> oracle.decode
    -> poses_to_results with the scale-1 metas;
  * the merge launch replays from a captured graph with the eager results."""
import argparse

import numpy as np
import pytest
import torch

import oracle
from offsetguided_amd import _lib, decoder, evaluate, models, synth, transforms
from offsetguided_amd.config import coco_data as cd
from offsetguided_amd.decoder import multiscale

pytestmark = pytest.mark.gpu
OFLAGS = dict(topk_k=32, thre_hmp=0.04, min_len=0.5, person_thre=0.04, dist_max=40.0)
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    _lib.load()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------- numpy restatement
def np_resample(hm, off, aff, h, w):
    """One scale's (merged) maps (N, C, hs, ws) / (N, 2L, hs, ws) onto the (h, w) base grid, fp32, the kernel's operation order."""
    N, C, hs, ws = hm.shape
    ho, oo = np.empty((N, C, h, w), F32), np.empty((N, off.shape[1], h, w), F32)
    for n in range(N):
        Ax, Bx, Ay, By, ix, iy = [F32(v) for v in aff[n]]
        u = Ax * np.arange(w, dtype=F32)
        u = np.minimum(np.maximum(u + Bx, F32(0)), F32(ws - 1))
        r = Ay * np.arange(h, dtype=F32)
        r = np.minimum(np.maximum(r + By, F32(0)), F32(hs - 1))
        x0, y0 = np.floor(u).astype(np.int64), np.floor(r).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, ws - 1), np.minimum(y0 + 1, hs - 1)
        fx, fy = u - x0.astype(F32), (r - y0.astype(F32))[:, None]
        gx, gy = F32(1) - fx, F32(1) - fy
        for src, dst in ((hm[n], ho[n]), (off[n], oo[n])):
            p00, p01 = src[:, y0[:, None], x0[None, :]], src[:, y0[:, None], x1[None, :]]
            p10, p11 = src[:, y1[:, None], x0[None, :]], src[:, y1[:, None], x1[None, :]]
            top = p00 * gx + p01 * fx
            bot = p10 * gx + p11 * fx
            dst[:] = top * gy + bot * fy
        oo[n, 0::2] *= ix
        oo[n, 1::2] *= iy
    return ho, oo


def np_merge(outputs, affs, h, w, flip, skeleton=cd.COCO_PERSON_SKELETON):
    """merge_scales restated: flip pair merged by the oracle, resampled, summed in list order, times 1/S at the last scale."""
    S = len(outputs)
    inv = F32(1) / F32(S)
    acc = None
    for s, ((hm, off), aff) in enumerate(zip(outputs, affs)):
        hm, off = np.asarray(hm, F32), np.asarray(off, F32)
        if flip:
            perm, rev = cd.offset_hflip(cd.COCO_KEYPOINTS, skeleton)
            hm, off = oracle.flip_merge(hm, off, cd.heatmap_hflip(cd.COCO_KEYPOINTS), perm, rev)
        v = np_resample(hm, off, aff, h, w)
        if s == 0:
            acc = [v[0].copy(), v[1].copy()]
        else:
            acc = [a + b for a, b in zip(acc, v)]
            if s == S - 1:
                acc = [a * inv for a in acc]
    return acc


def dev_maps(seed, n, C, L, hs, ws):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, C, hs, ws, generator=g), torch.randn(n, 2 * L, hs, ws, generator=g) * 8


def random_affines(seed, N, hs, ws, h, w):
    """Tables that map the base grid over (and a little past) the source grid: up- or down-sampling by the size ratio, shifted."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(N):
        ax, ay = (ws - 1) / max(w - 1, 1) * rng.uniform(0.9, 1.1), (hs - 1) / max(h - 1, 1) * rng.uniform(0.9, 1.1)
        rows.append([ax, rng.uniform(-1.5, 1.5), ay, rng.uniform(-1.5, 1.5), 1 / ax, 1 / ay])
    return np.array(rows, F32)


# ---------------------------------------------------------------------------------- kernel vs numpy
KERNEL_CASES = [
    # N, (hs, ws), (h, w), flip, skeleton
    (1, (40, 37), (20, 18), False, cd.COCO_PERSON_SKELETON),        # down, ws % 4 != 0
    (8, (16, 24), (32, 48), False, cd.COCO_PERSON_SKELETON),        # up
    (2, (33, 50), (48, 31), True, cd.COCO_PERSON_SKELETON),         # non-square, mixed directions, flip
    (8, (24, 24), (40, 40), True, cd.COCO_PERSON_SKELETON),
    (3, (21, 30), (16, 16), True, cd.KINEMATIC_TREE_SKELETON),      # non-COCO skeleton (16 limbs) with flip
    (2, (21, 30), (29, 35), False, cd.DENSER_COCO_PERSON_SKELETON),
]


@pytest.mark.parametrize("N,src,dst,flip,skeleton", KERNEL_CASES)
def test_kernel_matches_numpy_bit_for_bit(dev, N, src, dst, flip, skeleton):
    C, L, F = 17, len(skeleton), 2 if flip else 1
    (hs, ws), (h, w) = src, dst
    outs = [dev_maps(10 * k + N, F * N, C, L, hs + k, ws + 2 * k) for k in range(3)]      # three scales of different sizes
    affs = [random_affines(k, N, hs + k, ws + 2 * k, h, w) for k in range(3)]
    hm_acc = torch.full((N, C, h, w), float('nan'), device=dev)
    off_acc = torch.full((N, 2 * L, h, w), float('nan'), device=dev)
    inv = float(F32(1) / F32(3))
    for k, mode in enumerate((multiscale.MODE_WRITE, multiscale.MODE_ADD, multiscale.MODE_ADD_SCALE)):
        hm, off = outs[k]
        multiscale.accumulate_scale(hm.to(dev), off.to(dev), torch.from_numpy(affs[k]).to(dev), (hm_acc, off_acc), mode, inv, flip,
                                    cd.COCO_KEYPOINTS, skeleton)
        exp = np_merge([(o[0].numpy(), o[1].numpy()) for o in outs[:k + 1]], affs[:k + 1], h, w, flip, skeleton)
        if mode == multiscale.MODE_ADD:      # np_merge scales at its last entry; mode 1 alone leaves the plain sum
            exp = np_merge([(o[0].numpy(), o[1].numpy()) for o in outs[:1]], affs[:1], h, w, flip, skeleton)
            v = np_merge([(o[0].numpy(), o[1].numpy()) for o in outs[1:2]], affs[1:2], h, w, flip, skeleton)
            exp = [a + b for a, b in zip(exp, v)]
        torch.cuda.synchronize()
        assert np.array_equal(hm_acc.cpu().numpy(), exp[0]), f'heatmaps, mode {mode}'
        assert np.array_equal(off_acc.cpu().numpy(), exp[1]), f'offsets, mode {mode}'


def test_merge_scales_matches_numpy(dev):
    """merge_scales over three scales (host tables, new accumulators) == np_merge, flip on."""
    N, C, L = 2, 17, 19
    sizes = [(12, 16), (24, 32), (36, 48)]
    outs = [dev_maps(s, 2 * N, C, L, *hw) for s, hw in enumerate(sizes)]
    affs = [random_affines(5 + s, N, *hw, 24, 32) for s, hw in enumerate(sizes)]
    feats = multiscale.merge_scales([(a.to(dev), b.to(dev)) for a, b in outs], affs, True, base_hw=(24, 32))
    exp = np_merge([(a.numpy(), b.numpy()) for a, b in outs], affs, 24, 32, True)
    assert np.array_equal(feats[0][0][-1].cpu().numpy(), exp[0]) and np.array_equal(feats[1][0][-1].cpu().numpy(), exp[1])
    assert feats[0][1] == [[]] and feats[1][2] == [[]]


# ---------------------------------------------------------------------------------- identity, units
IDENTITY = np.array([[1, 0, 1, 0, 1, 1]], F32)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("n_scales", [1, 2])
def test_base_scale_reproduces_its_input(dev, flip, n_scales):
    N, C, L, h, w = 3, 17, 19, 20, 27
    hm, off = dev_maps(7, (2 if flip else 1) * N, C, L, h, w)
    feats = multiscale.merge_scales([(hm.to(dev), off.to(dev))] * n_scales, [np.repeat(IDENTITY, N, 0)] * n_scales, flip,
                                    base_hw=(h, w))
    if flip:
        perm, rev = cd.offset_hflip(cd.COCO_KEYPOINTS, cd.COCO_PERSON_SKELETON)
        ehm, eoff = oracle.flip_merge(hm.numpy(), off.numpy(), cd.heatmap_hflip(cd.COCO_KEYPOINTS), perm, rev)
    else:
        ehm, eoff = hm.numpy(), off.numpy()
    assert np.array_equal(feats[0][0][-1].cpu().numpy(), ehm) and np.array_equal(feats[1][0][-1].cpu().numpy(), eoff)


def test_offset_units(dev):
    """A constant offset field (cx, cy) at a scale that is 2x the base along x and 4x along y merges to exactly (cx/2, cy/4)."""
    N, C, L, h, w = 2, 17, 19, 16, 24
    base = [{'offset': np.zeros(2), 'scale': np.array([1.0, 1.0])}] * N
    scaled = [{'offset': np.zeros(2), 'scale': np.array([2.0, 4.0])}] * N
    aff = multiscale.scale_affines(base, scaled, (h, w), (4 * h, 2 * w))
    assert np.array_equal(aff[:, [0, 2, 4, 5]], np.tile(F32([2, 4, 0.5, 0.25]), (N, 1)))
    hm = torch.rand(N, C, 4 * h, 2 * w)
    off = torch.empty(N, 2 * L, 4 * h, 2 * w)
    off[:, 0::2], off[:, 1::2] = 3.0, -5.0
    feats = multiscale.merge_scales([(hm.to(dev), off.to(dev))], [aff], False, base_hw=(h, w))
    o = feats[1][0][-1].cpu().numpy()
    assert (o[:, 0::2] == 1.5).all() and (o[:, 1::2] == -1.25).all()


# ---------------------------------------------------------------------------------- planted persons
def _decoder(batch):
    p = argparse.ArgumentParser()
    decoder.decoder_cli(p)
    a = p.parse_args('--topk 32 --thre-hmp 0.04 --person-thre 0.04 --dist-max 40'.split())
    a.headnets, a.strides, a.batch_size = ['hmp', 'omp'], [4, 4], batch
    a.include_scale = a.include_jitter_offset = False
    return decoder.decoder_factory(a)


@pytest.mark.parametrize("scales", [(0.5, 1.0, 2.0), (2.0,)])
def test_planted_persons_come_back_at_the_base_grid(dev, scales):
    """Scenes planted on a 256 x 256 base input, rendered at each scale with the coordinates of that scale's input (metas: scale s,
    pad offsets (-s, -2s)); merged onto the base grid and decoded by the production decoder (K1-fused + K3): every planted visible
    keypoint comes back within 1.5 base pixels, one pose per planted person.  One person per image, the body keypoints (5..16)
    visible: the face keypoints of a synthetic person lie 3-7 px apart and melt into one blob at scale 0.5 (sigma 7 input pixels),
    and persons that overlap split differently at each scale -- neither is what this test is about."""
    N, H = 5, 256
    proc = _decoder(N)
    base_metas = [{'offset': np.array([0.0, 0.0]), 'scale': np.array([1.0, 1.0])}] * N
    scenes = []
    for i in range(N):
        xy, _, amp = synth.make_scene(synth.HashRng(10 * i + 40), H, H, n_persons=1)
        inside = (xy[..., 0] > 2) & (xy[..., 0] < H - 3) & (xy[..., 1] > 2) & (xy[..., 1] < H - 3)
        scenes.append((xy, inside & (np.arange(17) >= 5), amp))
    outs, affs = [], []
    for s in scales:
        meta = {'offset': np.array([-1.0 * s, -2.0 * s]), 'scale': np.array([s, s])}
        Hs = int(H * s)
        maps = []
        for i, (xy, vis, amp) in enumerate(scenes):
            xy_s = xy * s - meta['offset']                                  # X_s = x * sc_s - off_s
            maps.append(synth.render_maps(synth.HashRng(7 + i), xy_s, vis, amp, Hs, Hs, hm_noise=0.002, off_noise=0.1))
        outs.append((torch.from_numpy(np.stack([m[0] for m in maps])).to(dev), torch.from_numpy(np.stack([m[1] for m in maps])).to(dev)))
        affs.append(multiscale.scale_affines(base_metas, [meta] * N, (H // 4, H // 4), (Hs // 4, Hs // 4)))
    feats = multiscale.merge_scales(outs, affs, False, base_hw=(H // 4, H // 4))
    poses = proc.generate_poses(feats, flip_test=False)
    for (xy, vis, _), got in zip(scenes, poses):
        assert len(got) == len(xy), f'{len(got)} poses for {len(xy)} planted persons'
        for p in range(len(xy)):
            d = np.hypot(got[:, :, 0] - xy[p, :, 0], got[:, :, 1] - xy[p, :, 1])        # (poses, 17)
            best = np.argmin(np.where(vis[p], d, 0).sum(1))
            assert (d[best][vis[p]] <= 1.5).all(), (p, d[best][vis[p]].max())


# ---------------------------------------------------------------------------------- strict engines at the new shapes
@pytest.mark.parametrize("shape", [(8, 384, 384), (8, 1024, 1024), (16, 1024, 1024), (8, 1280, 1280)])
def test_engines_at_the_scale_shapes_run_no_torch_convolution(dev, shape):
    p = argparse.ArgumentParser()
    models.net_cli(p)
    model, _ = models.model_factory(p.parse_args(['--no-pretrain']))
    model = model.to(dev).eval()
    eng = models.InferenceEngine(model, *shape, device=dev)
    assert eng.strict and eng.torch_conv_calls == []
    hm, off = eng.forward_raw(torch.randn(shape[0], 3, shape[1], shape[2], device=dev))[:2]
    torch.cuda.synchronize()
    assert eng.torch_conv_calls == [] and tuple(hm.shape) == (shape[0], 17, shape[1] // 4, shape[2] // 4)
    assert bool(torch.isfinite(hm).all()) and bool(torch.isfinite(off).all())
    del eng, hm, off
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------- run_images end to end
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


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("in_flight", [1, 2])
def test_run_images_multi_scale(dev, monkeypatch, flip, in_flight):
    monkeypatch.setattr(evaluate, 'IN_FLIGHT', in_flight)
    scales = [0.5, 1.0, 1.5]
    torch.manual_seed(0)
    a = _cli(['--test-scales', *map(str, scales)] + (['--flip-test'] if flip else []))
    model, _ = models.model_factory(a)
    seen = []
    real = multiscale.accumulate_scale

    def spy(hm, off, aff, out, mode, inv_count, flip_test, *rest):
        seen.append((hm.cpu().numpy().copy(), off.cpu().numpy().copy(), aff.cpu().numpy().copy(), mode))
        return real(hm, off, aff, out, mode, inv_count, flip_test, *rest)
    monkeypatch.setattr(multiscale, 'accumulate_scale', spy)
    loader = _raw_loader()
    stats = {}
    results, ids = evaluate.run_images(a, data_loader=loader, model=model, stats=stats)
    assert ids == [1, 2, 3, 4, 5] and len(seen) == 3 * len(loader)
    assert stats['test_scales'] == scales and stats['torch_conv_calls'] == 0
    F = 2 if flip else 1
    assert sorted(stats['engines_per_shape']) == sorted(f'{2 * F}x3x{P}x{P}' for P in (128, 256, 384))
    pre = transforms.EvalPreprocess(256)
    exp_results, exp_ids = [], []
    for b, (imgs, _, metas) in enumerate(loader):
        per_scale = pre.multi_scale(list(imgs), scales, image_ids=[m['image_id'] for m in metas])
        base_metas = per_scale[1][1]
        rec = seen[3 * b:3 * b + 3]
        assert [r[3] for r in rec] == [0, 1, 2]
        affs = []
        for (x, metas_s), r in zip(per_scale, rec):
            aff = multiscale.scale_affines(base_metas, metas_s, (64, 64), (x.shape[2] // 4, x.shape[3] // 4))
            aff = np.concatenate((aff, np.repeat(aff[-1:], 2 - len(aff), 0)))   # the ragged batch's filler image
            assert np.array_equal(r[2], aff)
            assert r[0].shape == (2 * F, 17, x.shape[2] // 4, x.shape[3] // 4)
            affs.append(aff)
        hm, off = np_merge([(r[0], r[1]) for r in rec], affs, 64, 64, flip)
        poses, _ = oracle.decode(hm, off, cd.COCO_PERSON_SKELETON, **OFLAGS)
        for image_poses, meta in zip(poses, base_metas):
            evaluate.poses_to_results(image_poses, meta, exp_results, exp_ids)
    assert exp_ids == ids and len(results) == len(exp_results)
    for got, exp in zip(results, exp_results):
        assert got['image_id'] == exp['image_id'] and got['keypoints'] == exp['keypoints'] and abs(got['score'] - exp['score']) <= 1e-6


def test_run_images_with_scale_one_is_todays_path(dev, monkeypatch):
    calls = []
    monkeypatch.setattr(multiscale, 'accumulate_scale', lambda *a, **k: calls.append(1))
    torch.manual_seed(0)
    a0 = _cli(['--flip-test'])
    model, _ = models.model_factory(a0)
    r0, i0 = evaluate.run_images(a0, data_loader=_raw_loader(), model=model)
    r1, i1 = evaluate.run_images(_cli(['--flip-test', '--test-scales', '1']), data_loader=_raw_loader(), model=model)
    assert calls == [] and i0 == i1 == [1, 2, 3, 4, 5] and r0 == r1


def test_multi_scale_needs_raw_images(dev):
    a = _cli(['--test-scales', '0.5', '1'])
    model, _ = models.model_factory(a)
    with pytest.raises(ValueError, match='raw'):
        evaluate.run_images(a, model=model, n_synthetic_batches=1)


# ---------------------------------------------------------------------------------- graph capture
def test_merge_launch_replays_from_a_graph(dev):
    N, C, L, h, w = 2, 17, 19, 32, 40
    hm, off = [t.to(dev) for t in dev_maps(3, 2 * N, C, L, 48, 60)]
    aff = torch.from_numpy(random_affines(9, N, 48, 60, h, w)).to(dev)
    eager = (torch.zeros(N, C, h, w, device=dev), torch.zeros(N, 2 * L, h, w, device=dev))
    multiscale.accumulate_scale(hm, off, aff, eager, multiscale.MODE_WRITE, 1.0, True)
    multiscale.accumulate_scale(hm, off, aff, eager, multiscale.MODE_ADD_SCALE, 0.5, True)
    acc = (torch.zeros(N, C, h, w, device=dev), torch.zeros(N, 2 * L, h, w, device=dev))
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        multiscale.accumulate_scale(hm, off, aff, acc, multiscale.MODE_WRITE, 1.0, True)     # warm-up: the flip tables
    torch.cuda.current_stream(dev).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        multiscale.accumulate_scale(hm, off, aff, acc, multiscale.MODE_WRITE, 1.0, True)
        multiscale.accumulate_scale(hm, off, aff, acc, multiscale.MODE_ADD_SCALE, 0.5, True)
    acc[0].zero_()
    acc[1].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(acc[0], eager[0]) and torch.equal(acc[1], eager[1])
