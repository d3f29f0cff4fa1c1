"""GPU: the training augmentation (csrc/augment.hip: og_warp_affine_batch_u8, og_warp_affine_mask_u8, og_affine_joints_f32;
transforms.DeviceAugment; train_dist --augment).

Every kernel case asserts equality with the numpy restatement of the header's specification (tests/augment_common.py): integer
arithmetic, and float64 / fp32 operations that are each correctly rounded in a fixed order on both sides, so no tolerance applies.
Shapes are tiny: destination squares of 64 and 50 pixels (50 is neither a multiple of the tile nor of 4: the scalar-store path and a
partly filled last tile), three sources of different sizes in one launch."""
import ctypes as C
import json
import math
import random

import numpy as np
import pytest
import torch

import augment_common as ac
from offsetguided_amd import _lib, encoder, transforms
from offsetguided_amd.models import networks

pytestmark = pytest.mark.gpu
SIDES = (64, 50)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sources(dev):
    """The three source images and mask planes, on the host and packed back to back on the device."""
    images, masks = ac.source_images()
    raw = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])).to(dev)
    planes = torch.from_numpy(np.concatenate([m.reshape(-1) for m in masks])).to(dev)
    return images, masks, raw, planes


def _tables(sizes, channels):
    n = len(sizes)
    offs, hw4, o = (C.c_long * n)(), (C.c_int * (4 * n))(), 0
    for i, (h, w) in enumerate(sizes):
        offs[i] = o
        hw4[4 * i:4 * i + 4] = [h, w, 0, 0]
        o += h * w * channels
    return offs, hw4


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _warp(dev, raw, planes, sizes, D, S):
    """Both entry points for forward-inverse rows D (n,2,3) -> (fp32 NCHW, uint8 NHWC, mask planes), each pre-filled with a sentinel."""
    lib = _lib.load()
    n = len(sizes)
    D = np.ascontiguousarray(np.asarray(D, np.float64).reshape(n, 6))
    out = torch.full((n, 3, S, S), -77.0, dtype=torch.float32, device=dev)
    u8 = torch.full((n, S, S, 3), 7, dtype=torch.uint8, device=dev)
    mask = torch.full((n, S, S), 7, dtype=torch.uint8, device=dev)
    offs, hw4 = _tables(sizes, 3)
    _lib.check(lib.og_warp_affine_batch_u8(_lib.ptr(raw), offs, hw4, n, D.ctypes.data_as(C.c_void_p), S, (C.c_ubyte * 3)(*ac.BORDER),
                                           _f3(ac.MEAN), _f3(ac.STD), _lib.ptr(out), _lib.ptr(u8), _lib.stream_ptr(dev)), lib)
    moffs, _ = _tables(sizes, 1)
    _lib.check(lib.og_warp_affine_mask_u8(_lib.ptr(planes), moffs, hw4, n, D.ctypes.data_as(C.c_void_p), S, 255, _lib.ptr(mask),
                                          _lib.stream_ptr(dev)), lib)
    return out, u8, mask


def _check(dev, sources, mats, S, what):
    images, masks, raw, planes = sources
    D = [ac.inverse_rows(m) for m in mats]
    out, u8, mask = _warp(dev, raw, planes, ac.SIZES, D, S)
    u8, mask = u8.cpu().numpy(), mask.cpu().numpy()
    for i, (im, m) in enumerate(zip(images, masks)):
        ref = ac.warp_u8(im, D[i], S, ac.BORDER)
        bad = np.argwhere((u8[i] != ref).any(axis=-1))
        assert np.array_equal(u8[i], ref), f'{what}, image {i}: {len(bad)} pixels differ, first (row, col) {bad[:5].tolist()}'
        assert torch.equal(out[i].cpu(), torch.from_numpy(ac.normalize(ref))), f'{what}, image {i}: fp32 output'
        assert np.array_equal(mask[i], ac.warp_u8(m, D[i], S, 255)), f'{what}, image {i}: mask'
    return u8


@pytest.mark.parametrize('S', SIDES)
@pytest.mark.parametrize('name', sorted(ac.fixed_cases(64)))
def test_warp_equals_the_restatement(dev, sources, name, S):
    u8 = _check(dev, sources, ac.fixed_cases(S)[name], S, name)
    border = np.array(ac.BORDER, np.uint8)
    is_border = (u8 == border).all(axis=-1)
    if name == 'all_border':
        assert is_border.all()
    elif name == 'identity':
        for i, (h, w) in enumerate(ac.SIZES):
            hh, ww = min(h, S), min(w, S)
            assert np.array_equal(u8[i, :hh, :ww], sources[0][i][:hh, :ww]) and is_border[i, hh:].all() and is_border[i, :, ww:].all()
    elif name == 'rotate45_scale_half':
        assert is_border.mean() > 0.5 and not is_border.all()   # most of the square is border round the shrunken sources
    else:
        assert not is_border.all() and not is_border[:, S // 2 - 4:S // 2 + 4, S // 2 - 4:S // 2 + 4].all()


@pytest.mark.parametrize('S', SIDES)
def test_warp_equals_the_restatement_on_random_draws(dev, sources, S):
    """20 seeds of the default parameter draws (most of them move the tiny sources far: border, edges and interior all occur)."""
    seen_inside = 0
    for seed, mats in enumerate(ac.random_cases(S, 20)):
        u8 = _check(dev, sources, mats, S, f'seed {seed}')
        seen_inside += int(not (u8 == np.array(ac.BORDER, np.uint8)).all())
    assert seen_inside >= 5


def test_more_images_than_one_launch_carries(dev, sources):
    """35 images: the descriptor table of a launch holds 32."""
    images, masks, raw, planes = sources
    S, n = 50, 35
    sizes = [ac.SIZES[i % 3] for i in range(n)]
    rs = np.random.RandomState(2)
    mats = [np.array([[1, 0, rs.uniform(-9, 9)], [0, 1, rs.uniform(-9, 9)], [0, 0, 1.]]) for _ in range(n)]
    D = [ac.inverse_rows(m) for m in mats]
    lib = _lib.load()
    Dc = np.ascontiguousarray(np.asarray(D).reshape(n, 6))
    offs, hw4 = _tables(ac.SIZES, 3)
    moffs, _ = _tables(ac.SIZES, 1)
    offs_n, moffs_n, hw4_n = (C.c_long * n)(), (C.c_long * n)(), (C.c_int * (4 * n))()
    for i in range(n):
        offs_n[i], moffs_n[i] = offs[i % 3], moffs[i % 3]
        hw4_n[4 * i:4 * i + 4] = hw4[4 * (i % 3):4 * (i % 3) + 4]
    out = torch.empty((n, 3, S, S), dtype=torch.float32, device=dev)
    u8 = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev)
    mask = torch.empty((n, S, S), dtype=torch.uint8, device=dev)
    _lib.check(lib.og_warp_affine_batch_u8(_lib.ptr(raw), offs_n, hw4_n, n, Dc.ctypes.data_as(C.c_void_p), S, (C.c_ubyte * 3)(*ac.BORDER),
                                           _f3(ac.MEAN), _f3(ac.STD), _lib.ptr(out), _lib.ptr(u8), _lib.stream_ptr(dev)), lib)
    _lib.check(lib.og_warp_affine_mask_u8(_lib.ptr(planes), moffs_n, hw4_n, n, Dc.ctypes.data_as(C.c_void_p), S, 255, _lib.ptr(mask),
                                          _lib.stream_ptr(dev)), lib)
    u8, mask, out = u8.cpu().numpy(), mask.cpu().numpy(), out.cpu()
    for i in (0, 1, 2, 31, 32, 33, 34):
        ref = ac.warp_u8(images[i % 3], D[i], S, ac.BORDER)
        assert np.array_equal(u8[i], ref) and torch.equal(out[i], torch.from_numpy(ac.normalize(ref))), i
        assert np.array_equal(mask[i], ac.warp_u8(masks[i % 3], D[i], S, 255)), i


def test_argument_errors_are_status_codes(dev, sources):
    """Host-side refusals only: nothing is launched, the outputs keep their sentinel."""
    images, masks, raw, planes = sources
    lib = _lib.load()
    S = 64
    offs, hw4 = _tables(ac.SIZES, 3)
    out = torch.full((3, 3, S, S), -77.0, dtype=torch.float32, device=dev)
    mask = torch.full((3, S, S), 7, dtype=torch.uint8, device=dev)
    border, mean, std = (C.c_ubyte * 3)(*ac.BORDER), _f3(ac.MEAN), _f3(ac.STD)

    def batch(D, S=S, raw_ptr=_lib.ptr(raw), hw=hw4):
        D = np.ascontiguousarray(np.asarray(D, np.float64).reshape(3, 6))
        return lib.og_warp_affine_batch_u8(raw_ptr, offs, hw, 3, D.ctypes.data_as(C.c_void_p), S, border, mean, std, _lib.ptr(out), None,
                                           _lib.stream_ptr(dev))

    ident = [np.eye(3)[:2]] * 3
    assert batch(ident, raw_ptr=None) == _lib.OG_EINVAL and b'null pointer' in lib.og_last_error()
    assert batch(ident, S=0) == _lib.OG_EINVAL
    bad_hw = (C.c_int * 12)(*hw4)
    bad_hw[5] = 0
    assert batch(ident, hw=bad_hw) == _lib.OG_EINVAL and b'image 1' in lib.og_last_error()
    far = [np.eye(3)[:2], np.array([[2.0 ** 14, 0, 0], [0, 1, 0.]]), np.eye(3)[:2]]                # 2^14 * 64 = 2^20
    assert batch(far) == _lib.OG_EINVAL and b'2^20' in lib.og_last_error()
    assert batch([np.eye(3)[:2], np.array([[1, 0, np.nan], [0, 1, 0.]]), np.eye(3)[:2]]) == _lib.OG_EINVAL
    D = np.ascontiguousarray(np.asarray(far).reshape(3, 6))
    moffs, _ = _tables(ac.SIZES, 1)
    assert lib.og_warp_affine_mask_u8(_lib.ptr(planes), moffs, hw4, 3, D.ctypes.data_as(C.c_void_p), S, 255, _lib.ptr(mask),
                                      _lib.stream_ptr(dev)) == _lib.OG_EINVAL
    Di = np.ascontiguousarray(np.asarray(ident).reshape(3, 6))
    assert lib.og_warp_affine_mask_u8(_lib.ptr(planes), moffs, hw4, 3, Di.ctypes.data_as(C.c_void_p), S, 256, _lib.ptr(mask),
                                      _lib.stream_ptr(dev)) == _lib.OG_EINVAL
    torch.cuda.synchronize()
    assert bool((out == -77.0).all()) and bool((mask == 7).all())


# ----------------------------------------------------------------------------------------------------------------- keypoints
def _joints_call(dev, joints, n_persons, M, flips, scales, S_w, S_h):
    lib = _lib.load()
    n, P, K, _ = joints.shape
    jd = torch.from_numpy(joints).to(dev)
    nd = torch.from_numpy(n_persons).to(dev)
    out = torch.full(joints.shape, -77.0, dtype=torch.float32, device=dev)
    M = np.ascontiguousarray(np.asarray(M, np.float64).reshape(n, 6))
    _lib.check(lib.og_affine_joints_f32(_lib.ptr(jd), _lib.ptr(nd), n, P, K, M.ctypes.data_as(C.c_void_p), (C.c_int * n)(*flips),
                                        (C.c_double * n)(*scales), float(S_w), float(S_h), (C.c_int * 8)(*ac.LEFT), (C.c_int * 8)(*ac.RIGHT),
                                        8, _lib.ptr(out), _lib.stream_ptr(dev)), lib)
    return out.cpu()


def test_joints_equal_the_restatement_on_the_fixture(dev):
    """The fixture's 64 cases as ONE batch (two launches' worth of descriptors): bit for bit the restatement, visibility and
    left / right swap included; the padding rows beyond n_persons carry a sentinel and come back untouched."""
    z = np.load(ac.GOLDEN)
    joints, n_persons, params = z['joints'].copy(), z['n_persons'], z['params']
    for c in range(64):
        joints[c, n_persons[c]:] = 123.25
    flips = [int(p[0]) for p in params]
    scales = [math.sqrt((p[3] * p[2]) * (p[4] * p[2])) for p in params]
    got = _joints_call(dev, joints, n_persons, z['mat'][:, :2], flips, scales, 512, 512)
    for c in range(64):
        ref = ac.affine_joints(joints[c], int(n_persons[c]), z['mat'][c][:2], flips[c], scales[c], 512, 512)
        assert torch.equal(got[c], torch.from_numpy(ref)), c
        assert bool((got[c, n_persons[c]:] == 123.25).all())
        # and the reference itself: visibility exact
        assert np.array_equal(got[c, :n_persons[c], :, 2].numpy(), z['out'][c, :n_persons[c], :, 2]), c
    assert sum(flips) > 0 and bool((got[..., 2] == 0).any()) and bool((got[..., 2] > 0).any())


def test_joints_visibility_uses_both_sides(dev):
    """S_w != S_h: x is compared with S_w, y with S_h; a coordinate equal to the side stays, equal to 0 goes."""
    joints = np.zeros((1, 1, 17, 4), np.float32)
    joints[0, 0, :, 2] = 2
    joints[0, 0, :6, 0] = [0, 40, 40.5, 10, 10, -1]
    joints[0, 0, :6, 1] = [5, 5, 5, 30, 30.5, 5]
    joints[0, 0, 6:, :2] = 3
    M = np.eye(3)[None, :2]
    got = _joints_call(dev, joints, np.ones(1, np.int32), M, [0], [1.0], 40, 30)
    assert got[0, 0, :6, 2].tolist() == [0, 2, 0, 2, 0, 0] and bool((got[0, 0, 6:, 2] == 2).all())
    assert torch.equal(got[0], torch.from_numpy(ac.affine_joints(joints[0], 1, M[0], 0, 1.0, 40, 30)))


# ------------------------------------------------------------------------------------------------------------- DeviceAugment
def test_device_augment_end_to_end(dev, sources):
    images, masks, raw, planes = sources
    S = 64
    rs = np.random.RandomState(4)
    joints = np.zeros((3, 3, 17, 4), np.float32)
    for i, (h, w) in enumerate(ac.SIZES):
        joints[i, :, :, 0] = np.round(rs.uniform(2, w - 3, (3, 17)) * 4) / 4
        joints[i, :, :, 1] = np.round(rs.uniform(2, h - 3, (3, 17)) * 4) / 4
    joints[:, :, :, 2] = (rs.uniform(0, 1, (3, 3, 17)) > 0.2) * 2
    joints[:, :, :, 3] = rs.uniform(1, 9, (3, 3, 17))
    n_persons = np.array([3, 1, 0], np.int32)
    aug = transforms.DeviceAugment(S, transforms.AugParams(max_translate=8), device=dev)
    for _ in range(3):                                                    # allocator, the three pinned staging buffers, library warm-up
        aug(images, joints, n_persons, masks, rng=random.Random(1))
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode('error')
        out, jout, mout, mats = aug(images, joints, n_persons, masks, rng=random.Random(11))
        out_nomask = aug(images, joints, n_persons, rng=random.Random(11))
    finally:
        torch.cuda.set_sync_debug_mode(before)
    # the matrices are affine_matrix(...) of the same draws
    rng = random.Random(11)
    params = [aug.transform.draw(rng) for _ in range(3)]
    assert params == aug.last_params
    exp = np.stack([transforms.affine_matrix(p, transforms.roi_center(joints[i], n_persons[i], np.array([w, h])), np.array([w, h]), S)
                    for i, (p, (h, w)) in enumerate(zip(params, ac.SIZES))])
    assert mats.dtype == np.float64 and np.array_equal(mats, exp)
    # the outputs are the entry points called by hand (and so the restatement)
    D = [transforms.inverse_rows(m, S) for m in mats]
    o2, _, m2 = _warp(dev, raw, planes, ac.SIZES, D, S)
    assert out.shape == (3, 3, S, S) and torch.equal(out, o2) and mout.dtype == torch.uint8 and torch.equal(mout, m2)
    assert out_nomask[2] is None and torch.equal(out_nomask[0], out)
    for i in range(3):
        assert torch.equal(out[i].cpu(), torch.from_numpy(ac.normalize(ac.warp_u8(images[i], D[i], S, ac.BORDER)))), i
    flips = [int(p[0]) for p in params]
    scales = [math.sqrt((p[3] * p[2]) * (p[4] * p[2])) for p in params]
    j2 = _joints_call(dev, joints, n_persons, mats[:, :2], flips, scales, S, S)
    ref = np.stack([ac.affine_joints(joints[i], int(n_persons[i]), mats[i][:2], flips[i], scales[i], S, S) for i in range(3)])
    assert jout.shape == joints.shape and torch.equal(jout.cpu(), j2) and torch.equal(j2, torch.from_numpy(ref))
    # its joints feed the GT encoder
    enc = encoder.HeatMaps(S, 4, dev)
    nd = torch.from_numpy(n_persons).to(dev)
    hm_a = enc.encode_batch(jout, nd)[0]
    hm_b = enc.encode_batch(torch.from_numpy(ref).to(dev), nd)[0]
    assert hm_a.shape == (3, 17, 16, 16) and torch.equal(hm_a, hm_b) and float(hm_a.max()) > 0.5
    with pytest.raises(ValueError):
        aug.apply(images, joints, n_persons, np.stack([np.diag([0., 1, 1])] * 3), params)


# ---------------------------------------------------------------------------------------------------------------- train_dist
def test_train_dist_augment(dev, tmp_path, monkeypatch, capsys):
    """Two timed steps of train_dist --bench --augment at 256 x 256, batch 2: finite losses, a new crop in every step, augment_us.
    (256, the size of every GPU training test of the Hourglass-104: at 128 x 128 its innermost level is 1 x 1 pixel, and torch's
    training-mode batch norm on those maps crashed the process on the GPU -- in torch, outside this package's code.)"""
    from offsetguided_amd import train_dist
    monkeypatch.setattr(networks.torch, 'save', lambda data, path: None)
    seen = []
    real_step = train_dist.train_step

    def spy(model, criterion, optimizer, images, annos, *a, **k):
        loss, parts = real_step(model, criterion, optimizer, images, annos, *a, **k)
        seen.append((images.detach().clone(), float(loss)))
        return loss, parts

    monkeypatch.setattr(train_dist, 'train_step', spy)
    train_dist.main(['--no-pretrain', '--square-length', '256', '--batch-size', '2', '--checkpoint-path', str(tmp_path), '--augment',
                     '--bench', '--bench-steps', '2', '--bench-warmup', '1'])
    line = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1])
    assert line['augment_us'] > 0 and line['data'] == 'synthetic raw images, augmented and encoded on the device'
    assert line['steps'] == 2 and line['value'] > 0
    assert len(seen) == 3 and all(np.isfinite(loss) for _, loss in seen)
    (_, _), (im1, _), (im2, _) = seen
    assert im1.shape == (2, 3, 256, 256) and not torch.equal(im1, im2)
    assert bool(torch.isfinite(im1).all()) and float(im1.std()) > 0.05
